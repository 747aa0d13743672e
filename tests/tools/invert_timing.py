"""fd_invert_dev against the host-driven Newton loop it replaces, timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, rig_deltas x 1, no dist2, no projection; Y is the engine's own fp64
fd_deform output.  Between two events on one stream, alternating rounds in one process:
  invert      fd_invert_dev, one launch (residual and iters written);
  loop        k x fd_deform_vectors_dev in fp64 with the Jacobian -- per step the deformation's launch and the Jacobian's, which
              deliver F's displacement and A (36 B per vertex), the two launches per step a host-driven Newton needs;
  loop+deform k x (fd_deform_dev in fp64 + fd_deform_vectors_dev in fp64 with the Jacobian), three launches per step;
with k = the largest iters + 1 that fd_invert_dev reports (evaluations of its slowest vertex).  The loops leave out the 3x3
solve and update a host-driven Newton also launches per step, and they evaluate every vertex k times although most converge
sooner: both favour the loops only in the first point.
   python tests/tools/invert_timing.py [--out profiles/invert_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "invert_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("invert_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    rest = synth.control_points(M, "head")
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, rig_deltas x 1, no dist2, no projection; ms between two "
             f"events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each",
             "# invert: fd_invert_dev; loop: k x fd_deform_vectors_dev(fp64, Jacobian); loop+deform: k x (fd_deform_dev(fp64) + the same); "
             "k = largest iters + 1"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        d_P = torch.from_numpy(P).to(dev)
        d_Y, d_X, d_out = torch.empty_like(d_P), torch.empty_like(d_P), torch.empty_like(d_P)
        d_res = torch.empty(n, device=dev); d_its = torch.empty(n, dtype=torch.int32, device=dev)
        d_A = torch.empty((n, 9), device=dev)
        e.deform_dev(n, d_P.data_ptr(), d_Y.data_ptr())
        S.synchronize()

        def invert():
            e.invert_dev(n, d_Y.data_ptr(), d_X.data_ptr(), d_residual=d_res.data_ptr(), d_iters=d_its.data_ptr())

        invert(); S.synchronize()
        its = d_its.cpu().numpy()
        assert (its >= 0).all()
        hist = np.bincount(its)
        k = int(its.max()) + 1
        back = float((d_X - d_P).norm(dim=1).max())          # the round trip, for the record: |X - P| is a few ulp of P

        def loop():
            for _ in range(k):
                e.deform_vectors_dev(n, d_Y.data_ptr(), d_out.data_ptr(), d_jacobian=d_A.data_ptr())

        def loop_deform():
            for _ in range(k):
                e.deform_dev(n, d_Y.data_ptr(), d_out.data_ptr())
                e.deform_vectors_dev(n, d_Y.data_ptr(), d_out.data_ptr(), d_jacobian=d_A.data_ptr())

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        fns = {"invert": invert, "loop": loop, "loop+deform": loop_deform}
        t = {name_: [] for name_ in fns}
        for fn in fns.values():
            timed(fn, args.warmup, False)
        for _ in range(args.rounds):
            for name_, fn in fns.items():
                t[name_] += timed(fn, args.per_round, True)
        med = {name_: float(np.median(v)) for name_, v in t.items()}
        lines.append(f"{name}: iters histogram {dict(enumerate(hist.tolist()))}, k = {k}, max |X - P| = {back:.2e}")
        for name_, v in t.items():
            lines.append(f"  {name_:12s} median {med[name_]:8.3f}  min {min(v):8.3f}  max {max(v):8.3f}")
        lines.append(f"  loop / invert {med['loop'] / med['invert']:.2f}   loop+deform / invert {med['loop+deform'] / med['invert']:.2f}")
        print("\n".join(lines[-5:]), flush=True)
        e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
