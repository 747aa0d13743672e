"""Kernel times of fd_deform_vectors_dev beside the plain deformation, for one rocprofv3 --kernel-trace --stats run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o vectors -- python tools/vectors_profile.py

1M-vertex head mesh, 256 control points, linear term; thin-plate, QNN and cubic, fp32 and fp64.  Every vertex is live
(no dist2), the projection is on, and N, tangentu, tangentv and the Jacobian are all written: the most a call does.
Each configuration runs `--reps` times after one warm-up call; fd_deform_dev alone runs as often, so the stats hold the
deformation kernels (k_deform32 Gaussian-family, k_deform32_tps_mfma, k_deform64) beside k_vectors32_* / k_vectors64_*."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facedeform_amd import capi, synth   # noqa: E402

KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
         ("cubic", capi.KERNEL_CUBIC, [])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(args.n)
    rest = synth.control_points(args.m, "head")
    n0 = P.astype(np.float64) / np.linalg.norm(P, axis=1, keepdims=True)
    u = np.cross(n0, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n0, u)
    d_P, d_tu, d_tv, d_nrm = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (P, u, v, n0))
    d_out = torch.empty_like(d_P)
    d_No, d_tuo, d_tvo = (torch.empty_like(d_P) for _ in range(3))
    d_A = torch.empty((args.n, 9), device=dev)
    for name, kind, params in KINDS:
        e = capi.Engine(device=0)
        e.set_points(rest, synth.smooth_deltas(rest)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        e.build()
        for prec in (capi.EVAL_FP32, capi.EVAL_FP64):
            e.set_eval_precision(prec)
            frames = (d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr())
            for rep in range(args.reps + 1):
                e.deform_dev(args.n, d_P.data_ptr(), d_out.data_ptr(), 0, 0, *frames)
                e.deform_vectors_dev(args.n, d_P.data_ptr(), d_out.data_ptr(), 0, 0, *frames,
                                     d_N=d_nrm.data_ptr(), d_N_out=d_No.data_ptr(), d_vtu=d_tu.data_ptr(),
                                     d_vtu_out=d_tuo.data_ptr(), d_vtv=d_tv.data_ptr(), d_vtv_out=d_tvo.data_ptr(),
                                     d_jacobian=d_A.data_ptr())
            e.synchronize()
            print(f"{name} {'fp64' if prec == capi.EVAL_FP64 else 'fp32'}: {args.reps + 1} calls of each, "
                  f"|A - I| max {float((d_A - torch.eye(3, device=dev).reshape(1, 9)).abs().max()):.3e}")
        e.close()


if __name__ == "__main__":
    main()
