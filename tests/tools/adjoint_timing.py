"""fd_deform_adjoint_dev against the same pair work in the other orientation and against torch, timed on one device
(DESIGN.md 4.10).

1M head vertices, 256 control points, thin-plate and QNN, rig_deltas x 1, no dist2, no projection; G random normal.  Between
two events on one stream, alternating rounds in one process, medians of 25:
  adjoint  fd_deform_adjoint_dev: the centre-per-lane launch and the launch that adds the partial blocks;
  deform   the same context's fp64 fd_deform_dev: the same N x C pair work, reduced over the centres;
  torch    an fp64 formulation on the same GPU: Phi formed in chunks of vertices, grad += Phi^T @ R per chunk (the kernel
           function in the convention of W; 1, x, y, z appended for the polynomial rows).
The torch result is compared with the call's, for the record; nothing is asserted on time.
   python tests/tools/adjoint_timing.py [--out profiles/adjoint_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]
CHUNK = 1 << 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "adjoint_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    G = np.random.default_rng(11).standard_normal(P.shape).astype(np.float32)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, rig_deltas x 1, no dist2, no projection; ms between two "
             f"events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each",
             f"# adjoint: fd_deform_adjoint_dev; deform: fd_deform_dev(fp64); torch: fp64, Phi in chunks of {CHUNK} vertices, grad += Phi^T @ R"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        _, radii = e.get_weights()
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev); d_G = torch.from_numpy(G).to(dev)
            d_out = torch.empty_like(d_P)
            d_grad = torch.empty((M + 4, 3), dtype=torch.float64, device=dev)
            d_ref = torch.empty_like(d_grad)
            d_c = torch.from_numpy(rest.astype(np.float64)).to(dev)
            d_r2 = torch.from_numpy(radii ** 2).to(dev)
        S.synchronize()

        def adjoint():
            e.deform_adjoint_dev(n, d_P.data_ptr(), d_G.data_ptr(), d_grad.data_ptr())

        def deform():
            e.deform_dev(n, d_P.data_ptr(), d_out.data_ptr())

        def torch_form():
            with torch.cuda.stream(S):
                d_ref.zero_()
                for a in range(0, n, CHUNK):
                    X = d_P[a:a + CHUNK].double(); R = d_G[a:a + CHUNK].double()
                    D = X[:, None, :] - d_c[None]
                    d2 = (D * D).sum(dim=2)
                    if kind == capi.KERNEL_THIN_PLATE:
                        phi = 0.5 * torch.xlogy(d2, d2)
                    else:
                        phi = torch.exp(-d2 / d_r2[None])
                    basis = torch.cat([phi, torch.ones_like(X[:, :1]), X], dim=1)
                    d_ref.add_(basis.T @ R)

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"adjoint": adjoint, "deform": deform, "torch": torch_form}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        diff = float((d_grad - d_ref).abs().max() / d_ref.abs().max())
        lines.append(f"{name}: max |grad_W - torch| / max |torch| = {diff:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:8s} median {med[name_]:8.3f}  min {min(v):8.3f}  max {max(v):8.3f}")
        lines.append(f"  adjoint / deform {med['adjoint'] / med['deform']:.2f}   torch / adjoint {med['torch'] / med['adjoint']:.2f}")
        print("\n".join(lines[-5:]), flush=True)
        e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
