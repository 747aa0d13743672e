"""fd_deform_bake_dev against the two routes a caller had to B before it, timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, no dist2, no frames.  Between two events on one stream, alternating
rounds in one process, medians of 25:
  bake      fd_deform_bake_dev, B alone: the pack kernel and the launch;
  bake32    the same with B32 alone: half the bytes stored;
  both      B and B32;
  poses     route (a): M unit-delta poses -- per group of 32 control points one batched build on deltas that are (1, 1, 1) at
            one point each and one fd_batch_deform_shared_fp64_dev launch with FD_OUTPUT_DISPLACEMENT, whose x components are
            32 columns of B;
  torch     route (b): fp64 on the same GPU, Psi formed in chunks of vertices, B = Psi @ S per chunk.
The rate counts 2 (C+4) M N flop against the 78.6 TFLOP/s fp64 matrix peak at 2.4 GHz; the clock the launches held is not read
here.  The torch result and one group of the poses' are compared with the call's, for the record; nothing is asserted on time.
   python tests/tools/bake_timing.py [--out profiles/bake_timing.txt] [--rounds 5] [--per-round 5]"""
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
    ap.add_argument("--out", default=os.path.join("profiles", "bake_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vertices", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bake_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, no dist2, no frames; ms between two events on one "
             f"stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each",
             f"# bake / bake32 / both: fd_deform_bake_dev writing B / B32 / both; poses: {M // GROUP} x (batched build of {GROUP} unit-delta "
             f"rigs + fd_batch_deform_shared_fp64_dev); torch: fp64, Psi in chunks of {CHUNK} vertices, B = Psi @ S; rate: "
             f"2 (C+4) M N flop of {PEAK / 1e12:.1f} TFLOP/s; the clock was not read"]
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
            h.set_kernel(kind, params); h.set_term(capi.TERM_LINEAR); h.set_output(capi.OUTPUT_DISPLACEMENT)
            helpers.append(h)
        batch = capi.Batch(helpers)
        unit = np.zeros((M, M, 3), np.float32)
        unit[np.arange(M), np.arange(M), :] = 1
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev)
            d_S = torch.from_numpy(Sop).to(dev)
            d_B = torch.empty((n, M), dtype=torch.float64, device=dev)
            d_B32 = torch.empty((n, M), dtype=torch.float32, device=dev)
            d_ref = torch.empty((n, M), dtype=torch.float64, device=dev)
            d_c = torch.from_numpy(rest.astype(np.float64)).to(dev)
            d_r2 = torch.from_numpy(radii ** 2).to(dev)
            d_rest = torch.from_numpy(rest).to(dev)
            d_unit = torch.from_numpy(unit).to(dev)
            d_out = torch.empty((GROUP, n, 3), dtype=torch.float32, device=dev)
        S.synchronize()

        def bake():
            e.deform_bake_dev(n, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr())

        def bake32():
            e.deform_bake_dev(n, d_P.data_ptr(), d_S.data_ptr(), 0, d_B32.data_ptr())

        def both():
            e.deform_bake_dev(n, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr(), d_B32.data_ptr())

        def poses(groups=M // GROUP):
            for g in range(groups):
                batch.set_points_dev([d_rest.data_ptr()] * GROUP, [d_unit[g * GROUP + i].data_ptr() for i in range(GROUP)], M)
                batch.build_async(S.cuda_stream)
                batch.deform_shared_fp64_dev(n, d_P.data_ptr(), [d_out[i].data_ptr() for i in range(GROUP)], stream_ptr=S.cuda_stream)

        def torch_form():
            with torch.cuda.stream(S):
                for a in range(0, n, CHUNK):
                    X = d_P[a:a + CHUNK].double()
                    D = X[:, None, :] - d_c[None]
                    d2 = (D * D).sum(dim=2)
                    if kind == capi.KERNEL_THIN_PLATE:
                        phi = 0.5 * torch.xlogy(d2, d2)
                    else:
                        phi = torch.exp(-d2 / d_r2[None])
                    basis = torch.cat([phi, torch.ones_like(X[:, :1]), X], dim=1)
                    torch.matmul(basis, d_S, out=d_ref[a:a + CHUNK])

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"bake": bake, "bake32": bake32, "both": both, "poses": poses, "torch": torch_form}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        scale = float(d_ref.abs().max())
        diff = float((d_B - d_ref).abs().max()) / scale
        poses(1); S.synchronize()                                   # the first group again: columns 0..31
        diff_a = float((d_B[:, :GROUP] - d_out[:, :, 0].T.double()).abs().max()) / scale
        first = len(lines)
        lines.append(f"{name}: max |B - torch| / max |torch| = {diff:.2e}; max |B[:, :32] - poses| / max |torch| = {diff_a:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:8s} median {med[name_]:9.3f}  min {min(v):9.3f}  max {max(v):9.3f}")
        flop = 2.0 * nn * M * n
        lines.append(f"  bake {flop / med['bake'] / 1e9:.1f} TFLOP/s = {flop / med['bake'] * 1e3 / PEAK:.3f} of the peak;  "
                     f"bake32 {flop / med['bake32'] * 1e3 / PEAK:.3f};  poses / bake {med['poses'] / med['bake']:.1f}   "
                     f"torch / bake {med['torch'] / med['bake']:.2f}")
        print("\n".join(lines[first:]), flush=True)
        batch.close()
        for h in helpers:
            h.close()
        e.set_stream(None); e.close()
        del d_B, d_B32, d_ref, d_out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
