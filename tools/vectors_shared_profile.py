"""Kernel times of fd_batch_deform_vectors_shared_dev against the per-frame launches it replaces, for one rocprofv3
--kernel-trace --stats run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o vectors_shared -- python tools/vectors_shared_profile.py

1M-vertex head mesh, 256 control points, 32 frames of one rest rig, linear term; thin-plate and QNN.  Every vertex is
live (no dist2), the projection is on, N, tangentu and tangentv are written, no Jacobian.  Each kind runs `--reps`
shared calls after one warm-up (k_deform32_shared_w1 + k_vectors32_shared_<kind> per call) and as many rounds of the 32
per-frame fd_deform_vectors_dev launches (k_vectors32_<kind>) on the same arrays, so the stats hold both in one run."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facedeform_amd import capi, synth   # noqa: E402

KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    F, M, N = args.frames, args.m, args.n
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    n0 = P.astype(np.float64) / np.linalg.norm(P, axis=1, keepdims=True)
    u = np.cross(n0, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n0, u)
    d_P, d_tu, d_tv, d_nrm = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (P, u, v, n0))
    deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    d_rest, d_del = torch.from_numpy(rest).to(dev), torch.from_numpy(deltas).to(dev)
    outs = {k: [torch.empty_like(d_P) for _ in range(F)] for k in ("P", "N", "tu", "tv")}
    falls = [torch.empty(N, device=dev) for _ in range(F)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    frames = (d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr())
    for name, kind, params in KINDS:
        engines = []
        for _ in range(F):
            e = capi.Engine(device=0)
            e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
            engines.append(e)
        batch = capi.Batch(engines)
        batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
        batch.build_async()
        assert [r.terminationtype for r in batch.build_result()] == [1] * F
        for rep in range(args.reps + 1):
            batch.deform_vectors_shared_dev(N, d_P.data_ptr(), ptr(outs["P"]), d_falloff=ptr(falls), d_tangents=frames,
                                            d_N=d_nrm.data_ptr(), d_N_out=ptr(outs["N"]), d_vtu=d_tu.data_ptr(),
                                            d_vtu_out=ptr(outs["tu"]), d_vtv=d_tv.data_ptr(), d_vtv_out=ptr(outs["tv"]))
        torch.cuda.synchronize()
        for rep in range(args.reps + 1):
            for f, e in enumerate(engines):
                e.deform_vectors_dev(N, d_P.data_ptr(), outs["P"][f].data_ptr(), 0, 0, *frames, d_N=d_nrm.data_ptr(),
                                     d_N_out=outs["N"][f].data_ptr(), d_vtu=d_tu.data_ptr(), d_vtu_out=outs["tu"][f].data_ptr(),
                                     d_vtv=d_tv.data_ptr(), d_vtv_out=outs["tv"][f].data_ptr())
        torch.cuda.synchronize()
        print(f"{name}: {args.reps + 1} shared calls ({capi.fd_shared_vectors_kernel_name(M, F, kind)}) and as many rounds of "
              f"{F} per-frame launches, {N} vertices, M = {M}")
        batch.close()
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
