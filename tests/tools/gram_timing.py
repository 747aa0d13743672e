"""fd_deform_gram_dev beside the adjoint and against torch, and a whole fd_fit_deltas, timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, rig_deltas x 1, no dist2, omega = 1.  Between two events on one
stream, alternating rounds in one process, medians of 25:
  gram      fd_deform_gram_dev without projection frames: 1 component, both launches;
  gram6     the same with projection frames: 6 components;
  adjoint   fd_deform_adjoint_dev on the same mesh (the first-order term of a fit);
  torch     an fp64 formulation of gram on the same GPU: Psi formed in chunks of vertices, H += Psi^T @ Psi per chunk.
The rate counts 2 (C+4)^2 N flop per component -- the full square, as the issue that asked for the operator costs it -- against
the 78.6 TFLOP/s fp64 matrix peak at 2.4 GHz; the clock the launches held is not read here.  fd_fit_deltas (host arrays, S
given) is timed by its own report, medians of 5.  The torch result is compared with the call's, for the record; nothing is
asserted on time.
   python tests/tools/gram_timing.py [--out profiles/gram_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]
CHUNK = 1 << 14
PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gram_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    ap.add_argument("--fits", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gram_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    tu, tv, nrm = synth.tangent_frames(P)
    G = np.random.default_rng(11).standard_normal(P.shape).astype(np.float32)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, rig_deltas x 1, no dist2, omega = 1; ms between two "
             f"events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each",
             f"# gram / gram6: fd_deform_gram_dev without / with projection frames; adjoint: fd_deform_adjoint_dev; torch: fp64, Psi in "
             f"chunks of {CHUNK} vertices, H += Psi^T @ Psi; rate: 2 (C+4)^2 N flop per component, of {PEAK / 1e12:.1f} TFLOP/s"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        _, radii = e.get_weights()
        nn = M + 4
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev); d_G = torch.from_numpy(G).to(dev)
            d_tu, d_tv, d_nrm = (torch.from_numpy(a).to(dev) for a in (tu, tv, nrm))
            d_H = torch.empty((1, nn, nn), dtype=torch.float64, device=dev)
            d_H6 = torch.empty((6, nn, nn), dtype=torch.float64, device=dev)
            d_grad = torch.empty((nn, 3), dtype=torch.float64, device=dev)
            d_ref = torch.empty((nn, nn), dtype=torch.float64, device=dev)
            d_c = torch.from_numpy(rest.astype(np.float64)).to(dev)
            d_r2 = torch.from_numpy(radii ** 2).to(dev)
        S.synchronize()

        def gram():
            e.deform_gram_dev(n, d_P.data_ptr(), d_H.data_ptr())

        def gram6():
            e.deform_gram_dev(n, d_P.data_ptr(), d_H6.data_ptr(), 0, 0, d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr())

        def adjoint():
            e.deform_adjoint_dev(n, d_P.data_ptr(), d_G.data_ptr(), d_grad.data_ptr())

        def torch_form():
            with torch.cuda.stream(S):
                d_ref.zero_()
                for a in range(0, n, CHUNK):
                    X = d_P[a:a + CHUNK].double()
                    D = X[:, None, :] - d_c[None]
                    d2 = (D * D).sum(dim=2)
                    if kind == capi.KERNEL_THIN_PLATE:
                        phi = 0.5 * torch.xlogy(d2, d2)
                    else:
                        phi = torch.exp(-d2 / d_r2[None])
                    basis = torch.cat([phi, torch.ones_like(X[:, :1]), X], dim=1)
                    d_ref.add_(basis.T @ basis)

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"gram": gram, "gram6": gram6, "adjoint": adjoint, "torch": torch_form}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        diff = float((d_H[0] - d_ref).abs().max() / d_ref.abs().max())
        first = len(lines)
        lines.append(f"{name}: max |H - torch| / max |torch| = {diff:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:8s} median {med[name_]:8.3f}  min {min(v):8.3f}  max {max(v):8.3f}")
        flop = 2.0 * nn * nn * n
        lines.append(f"  gram {flop / med['gram'] / 1e9:.1f} TFLOP/s = {flop / med['gram'] * 1e3 / PEAK:.3f} of the peak;  "
                     f"gram6 {6 * flop / med['gram6'] / 1e9:.1f} TFLOP/s = {6 * flop / med['gram6'] * 1e3 / PEAK:.3f};  "
                     f"gram / adjoint {med['gram'] / med['adjoint']:.2f}   torch / gram {med['torch'] / med['gram']:.2f}")
        # a whole fit on host arrays, by its own report
        Sop = e.solve_operator()
        T = (P + G * np.float32(0.01)).astype(np.float32)
        reps = [e.fit_deltas(P, T, mu=1e-8 * n, S=Sop)[1] for _ in range(args.fits + 1)][1:]
        parts = {k: float(np.median([getattr(r, k) for r in reps])) for k in ("ms_gram", "ms_adjoint", "ms_compose", "ms_solve")}
        lines.append(f"  fd_fit_deltas (host arrays, S given, order {reps[0].order}), medians of {args.fits}: gram {parts['ms_gram']:.2f}  "
                     f"adjoint {parts['ms_adjoint']:.2f}  compose {parts['ms_compose']:.2f}  solve {parts['ms_solve']:.2f} ms")
        print("\n".join(lines[first:]), flush=True)
        e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
