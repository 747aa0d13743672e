"""fd_deform_adjoint_points_dev against the same pair work in the forward direction and against the only other route to A^T g,
timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, rig_deltas x 1, no dist2 (no gate), no projection; G random normal.
Between two events on one stream, alternating rounds in one process, medians of 25:
  points    fd_deform_adjoint_points_dev without grad_f: the one launch;
  points_f  the same with grad_f;
  deform    the same context's fp64 fd_deform_dev: the same N x C pair work;
  jacobian  fd_deform_vectors_dev in fp64 with the jacobian output alone (it evaluates the deformation as well: the call has
            no form without it), then torch.einsum for A^T g on the stored fp32 A.
The einsum's result is compared with the call's, for the record; nothing is asserted on time, and the clock the launches held
is not read.
   python tests/tools/adjoint_points_timing.py [--out profiles/adjoint_points_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "adjoint_points_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_points_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    G = np.random.default_rng(11).standard_normal(P.shape).astype(np.float32)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, rig_deltas x 1, no dist2, no projection; ms between two "
             f"events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each; the clock was not read",
             "# points / points_f: fd_deform_adjoint_points_dev without / with grad_f; deform: fd_deform_dev(fp64); "
             "jacobian: fd_deform_vectors_dev(fp64, jacobian) + torch.einsum A^T g"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev); d_G = torch.from_numpy(G).to(dev)
            d_out = torch.empty_like(d_P)
            d_gp = torch.empty((n, 3), dtype=torch.float64, device=dev)
            d_gf = torch.empty((n,), dtype=torch.float64, device=dev)
            d_jac = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
        ref = [None]                                  # the einsum's last result
        S.synchronize()

        def points():
            e.deform_adjoint_points_dev(n, d_P.data_ptr(), d_G.data_ptr(), d_gp.data_ptr())

        def points_f():
            e.deform_adjoint_points_dev(n, d_P.data_ptr(), d_G.data_ptr(), d_gp.data_ptr(), d_gf.data_ptr())

        def deform():
            e.deform_dev(n, d_P.data_ptr(), d_out.data_ptr())

        def jacobian():
            e.deform_vectors_dev(n, d_P.data_ptr(), d_out.data_ptr(), d_jacobian=d_jac.data_ptr())
            with torch.cuda.stream(S):
                ref[0] = torch.einsum("vck,vc->vk", d_jac, d_G)

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"points": points, "points_f": points_f, "deform": deform, "jacobian": jacobian}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        diff = float((d_gp - ref[0].double()).abs().max() / d_gp.abs().max())
        lines.append(f"{name}: max |grad_P - einsum(A, g)| / max |grad_P| = {diff:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:8s} median {med[name_]:8.3f}  min {min(v):8.3f}  max {max(v):8.3f}")
        lines.append(f"  points / deform {med['points'] / med['deform']:.2f}   points_f / points {med['points_f'] / med['points']:.2f}   "
                     f"jacobian / points {med['jacobian'] / med['points']:.2f}")
        print("\n".join(lines[-6:]), flush=True)
        e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
