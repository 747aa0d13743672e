"""Kernel times of fd_batch_deform_shared_fp64_dev against the per-frame fp64 launches it replaces, for one rocprofv3
--kernel-trace --stats run (no counters in the same run):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o shared_fp64 -- python tools/shared_fp64_profile.py

1M-vertex head mesh, 256 control points, 32 frames of one rest rig, linear term; thin-plate, QNN and cubic.  Every vertex
is live (no dist2), fd_falloff is written, no tangent frames.  Each kind runs `--reps` launches of the new call
(k_pack_shared64 + k_deform64_shared<kind, 6, true> each) and, on the same contexts set to FD_EVAL_FP64, the 32 per-frame
k_deform64<kind, 2> launches of fd_batch_deform_dev, so the stats hold both in one run.  The template arguments tell the
kinds apart in the stats: 0 thin-plate, 3 cubic, 2 the Gaussian kinds (the numbering of include/facedeform_hip.h)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facedeform_amd import capi, synth   # noqa: E402

KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]), ("cubic", capi.KERNEL_CUBIC, [])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    F, M, N = args.frames, args.m, args.n
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(dev)
    deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    d_rest, d_del = torch.from_numpy(rest).to(dev), torch.from_numpy(deltas).to(dev)
    outs = [torch.empty_like(d_P) for _ in range(F)]
    falls = [torch.empty(N, device=dev) for _ in range(F)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    torch.cuda.synchronize()
    for name, kind, params in KINDS:
        engines = []
        for _ in range(F):
            e = capi.Engine(device=0, precision=capi.EVAL_FP64)
            e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
            engines.append(e)
        batch = capi.Batch(engines)
        batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
        batch.build_async()
        assert [r.terminationtype for r in batch.build_result()] == [1] * F
        for rep in range(args.reps):
            batch.deform_shared_fp64_dev(N, d_P.data_ptr(), ptr(outs), d_falloff=ptr(falls))
        torch.cuda.synchronize()
        batch.deform_dev(N, [d_P.data_ptr()] * F, ptr(outs), d_falloff=ptr(falls))
        torch.cuda.synchronize()
        print(f"{name}: {args.reps} launches of the new call ({capi.fd_shared_fp64_kernel_name(M, F, kind)}) and {F} per-frame "
              f"k_deform64 launches, {N} vertices, M = {M}")
        batch.close()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
