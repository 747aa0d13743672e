"""fd_deform_bake_grad_dev against the two routes a caller had to G before it, timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, no dist2, no frames.  Between two events on one stream, alternating
rounds in one process, medians of 25:
  grad      fd_deform_bake_grad_dev, G alone: the pack kernel and the launch;
  grad32    the same with G32 alone: half the bytes stored;
  both      G and G32;
  poses     route (a): M unit-delta poses -- per group of 32 control points one batched build on deltas that are (1, 1, 1) at
            one point each and one fd_batch_deform_vectors_shared_fp64_dev call that writes the Jacobians, whose first rows
            less (1, 0, 0) are 32 columns of G (fp32);
  torch     route (b): fp64 on the same GPU, dPsi formed in chunks of vertices, G[:, a, :] = dPsi_a @ S per chunk.
The rate counts 2 . 3 (C+4) M N flop against the 78.6 TFLOP/s fp64 matrix peak at 2.4 GHz; the clock the launches held is not
read here.  The torch result and one group of the poses' are compared with the call's, for the record; nothing is asserted.
   python tests/tools/bake_grad_timing.py [--out profiles/bake_grad_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]
CHUNK = 1 << 14
PEAK = 78.6e12
GROUP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "bake_grad_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vertices", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bake_grad_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, no dist2, no frames; ms between two events on one "
             f"stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each",
             f"# grad / grad32 / both: fd_deform_bake_grad_dev writing G / G32 / both; poses: {M // GROUP} x (batched build of {GROUP} "
             f"unit-delta rigs + fd_batch_deform_vectors_shared_fp64_dev with Jacobians); torch: fp64, dPsi in chunks of {CHUNK} "
             f"vertices, G[:, a, :] = dPsi_a @ S; rate: 6 (C+4) M N flop of {PEAK / 1e12:.1f} TFLOP/s; the clock was not read"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        _, radii = e.get_weights()
        Sop = e.solve_operator()
        nn = M + 4
        # route (a): 32 contexts on the one rest rig, unit deltas
        helpers = []
        for _ in range(GROUP):
            h = capi.Engine(device=0, precision=capi.EVAL_FP64)
            h.set_kernel(kind, params); h.set_term(capi.TERM_LINEAR)
            helpers.append(h)
        batch = capi.Batch(helpers)
        unit = np.zeros((M, M, 3), np.float32)
        unit[np.arange(M), np.arange(M), :] = 1
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev)
            d_S = torch.from_numpy(Sop).to(dev)
            d_G = torch.empty((n, 3, M), dtype=torch.float64, device=dev)
            d_G32 = torch.empty((n, 3, M), dtype=torch.float32, device=dev)
            d_ref = torch.empty((n, 3, M), dtype=torch.float64, device=dev)
            d_c = torch.from_numpy(rest.astype(np.float64)).to(dev)
            d_r2 = torch.from_numpy(radii ** 2).to(dev)
            d_rest = torch.from_numpy(rest).to(dev)
            d_unit = torch.from_numpy(unit).to(dev)
            d_out = torch.empty((GROUP, n, 3), dtype=torch.float32, device=dev)
            d_jac = torch.empty((GROUP, n, 9), dtype=torch.float32, device=dev)
            zero = torch.zeros((1, 1), dtype=torch.float64, device=dev)
            eye = torch.eye(3, dtype=torch.float64, device=dev)
        S.synchronize()

        def grad():
            e.deform_bake_grad_dev(n, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr())

        def grad32():
            e.deform_bake_grad_dev(n, d_P.data_ptr(), d_S.data_ptr(), 0, d_G32.data_ptr())

        def both():
            e.deform_bake_grad_dev(n, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr(), d_G32.data_ptr())

        def poses(groups=M // GROUP):
            for g in range(groups):
                batch.set_points_dev([d_rest.data_ptr()] * GROUP, [d_unit[g * GROUP + i].data_ptr() for i in range(GROUP)], M)
                batch.build_async(S.cuda_stream)
                batch.deform_vectors_shared_fp64_dev(n, d_P.data_ptr(), [d_out[i].data_ptr() for i in range(GROUP)],
                                                     d_jacobian=[d_jac[i].data_ptr() for i in range(GROUP)],
                                                     stream_ptr=S.cuda_stream)

        def torch_form():
            with torch.cuda.stream(S):
                for a in range(0, n, CHUNK):
                    X = d_P[a:a + CHUNK].double()
                    D = X[:, None, :] - d_c[None]
                    d2 = (D * D).sum(dim=2)
                    if kind == capi.KERNEL_THIN_PLATE:
                        s = torch.where(d2 > 0, torch.log(d2) + 1.0, torch.zeros_like(d2))
                    else:
                        s = -2.0 / d_r2[None] * torch.exp(-d2 / d_r2[None])
                    for c in range(3):
                        basis = torch.cat([s * D[:, :, c], zero.expand(X.shape[0], 1), eye[c][None].expand(X.shape[0], 3)], dim=1)
                        torch.matmul(basis, d_S, out=d_ref[a:a + CHUNK, c])

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"grad": grad, "grad32": grad32, "both": both, "poses": poses, "torch": torch_form}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        scale = float(d_ref.abs().max())
        diff = float((d_G - d_ref).abs().max()) / scale
        poses(1); S.synchronize()                                   # the first group again: columns 0..31
        first_row = d_jac[:, :, 0:3].double()                       # A[0][a] of every pose: delta_0a + G[v][a][i]
        first_row[:, :, 0] -= 1.0
        diff_a = float((d_G[:, :, :GROUP] - first_row.permute(1, 2, 0)).abs().max()) / scale
        first = len(lines)
        lines.append(f"{name}: max |G - torch| / max |torch| = {diff:.2e}; max |G[:, :, :32] - poses (fp32)| / max |torch| = {diff_a:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:8s} median {med[name_]:9.3f}  min {min(v):9.3f}  max {max(v):9.3f}")
        flop = 6.0 * nn * M * n
        lines.append(f"  grad {flop / med['grad'] / 1e9:.1f} TFLOP/s = {flop / med['grad'] * 1e3 / PEAK:.3f} of the peak;  "
                     f"grad32 {flop / med['grad32'] * 1e3 / PEAK:.3f};  poses / grad {med['poses'] / med['grad']:.1f}   "
                     f"torch / grad {med['torch'] / med['grad']:.2f}")
        print("\n".join(lines[first:]), flush=True)
        batch.close()
        for h in helpers:
            h.close()
        e.set_stream(None); e.close()
        del d_G, d_G32, d_ref, d_out, d_jac
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
