"""Kernel times of fd_batch_deform_vectors_shared_fp64_dev's vector launch against the per-context fp64 launches it replaces
(fd_batch_deform_vectors_shared_dev on FD_EVAL_FP64 contexts, minus the position launches), for one rocprofv3
--kernel-trace --stats run (no counters in the same run):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o vectors_shared_fp64 -- python tools/vectors_shared_fp64_profile.py

1M-vertex head mesh, 256 control points, linear term; thin-plate and QNN; F in {1, 4, 12, 13, 32} frames of one rest rig;
dist2, projection frames and all vector outputs (N, tu, tv, A) given.  For each (kind, F) the script runs `--reps` calls of
the new entry point (k_pack_shared64 + k_deform64_shared + k_vectors64_shared<kind, NT, dense> each) and `--reps` calls of the
per-context form (F launches of k_vectors64_<kind> + F of k_deform64 each), so the stats hold both in one run.  In the stats
the template arguments tell the instantiations apart (kind: 0 Gaussian kinds, 2 thin-plate -- the numbering of
include/facedeform_hip.h; NT and dense: F = 1 and F = 4 share <1, false>, 12 is <3, false>, 13 <3, true>, 32 <6, true>), but not
F = 1 from F = 4; so the script also brackets each batch of calls with device events, with the position-only call timed the
same way and subtracted, and prints one line per (kind, F): those are the per-F figures.  --kinds and --frames widen the grid
(the crossover at small F: --kinds thin_plate qnn biharmonic cubic --frames 1 2 3 4, without the profiler)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facedeform_amd import capi, synth   # noqa: E402

KINDS = {"thin_plate": (capi.KERNEL_THIN_PLATE, []), "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
         "biharmonic": (capi.KERNEL_BIHARMONIC, []), "cubic": (capi.KERNEL_CUBIC, [])}
RADIUS2, RATE = 0.36, 1.7


def _frames(P):
    """Projection frames on the head ellipsoid and a dist2 that gates about a third of the vertices (the tests' inputs)."""
    n0 = P.astype(np.float64) / np.array([0.75, 1.0, 0.85]) ** 2
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    u = np.cross(n0, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n0, u)
    dist2 = (np.random.default_rng(5).random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    return (1.3 * u).astype(np.float32), (0.8 * v).astype(np.float32), n0.astype(np.float32), dist2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4, 12, 13, 32])
    ap.add_argument("--kinds", nargs="+", default=["thin_plate", "qnn"], choices=sorted(KINDS))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script only measures")
    dev = torch.device("cuda", 0)
    M, N, Fmax = args.m, args.n, max(args.frames)
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    tu, tv, nrm, dist2 = _frames(P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_P, d_tu, d_tv, d_nrm, d_d2 = (t(a) for a in (P, tu, tv, nrm, dist2))
    d_Nv = t(np.cross(tu, tv).astype(np.float32))
    deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(Fmax)]).astype(np.float32)
    d_rest, d_del = t(rest), t(deltas)
    mk = lambda w: [torch.empty((N, w), device=dev) for _ in range(Fmax)]
    oP, oN, otu, otv, oA = mk(3), mk(3), mk(3), mk(3), mk(9)
    ofall = [torch.empty(N, device=dev) for _ in range(Fmax)]
    ptr = lambda ts, F: [x.data_ptr() for x in ts[:F]]
    stream = torch.cuda.Stream(device=dev)
    for name in args.kinds:
        kind, params = KINDS[name]
        engines = []
        for _ in range(Fmax):
            e = capi.Engine(device=0, precision=capi.EVAL_FP64)
            e.set_stream(stream.cuda_stream)
            e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
            engines.append(e)
        full = capi.Batch(engines)
        full.set_points_dev([d_rest.data_ptr()] * Fmax, [d_del.data_ptr() + f * M * 12 for f in range(Fmax)], M)
        full.build_async(stream.cuda_stream)
        assert [r.terminationtype for r in full.build_result()] == [1] * Fmax
        for F in args.frames:
            batch = capi.Batch(engines[:F])
            common = dict(d_dist2=d_d2.data_ptr(), d_falloff=ptr(ofall, F), d_tangents=(d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr()),
                          radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream.cuda_stream)
            vec = dict(d_N=d_Nv.data_ptr(), d_N_out=ptr(oN, F), d_vtu=d_tu.data_ptr(), d_vtu_out=ptr(otu, F), d_vtv=d_tv.data_ptr(),
                       d_vtv_out=ptr(otv, F), d_jacobian=ptr(oA, F))
            calls = {
                "new": lambda: batch.deform_vectors_shared_fp64_dev(N, d_P.data_ptr(), ptr(oP, F), **common, **vec),
                "new_positions": lambda: batch.deform_shared_fp64_dev(N, d_P.data_ptr(), ptr(oP, F), **common),
                "per_context": lambda: batch.deform_vectors_shared_dev(N, d_P.data_ptr(), ptr(oP, F), **common, **vec),
                "per_context_positions": lambda: batch.deform_shared_dev(N, d_P.data_ptr(), ptr(oP, F), **common),
            }
            ms = {}
            for key, call in calls.items():
                call()                                     # warm-up: code objects, scratch
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(stream)
                for _ in range(args.reps):
                    call()
                ev1.record(stream)
                torch.cuda.synchronize()
                ms[key] = ev0.elapsed_time(ev1) / args.reps
            new_v, old_v = ms["new"] - ms["new_positions"], ms["per_context"] - ms["per_context_positions"]
            print(json.dumps({"kind": name, "N": N, "M": M, "frames": F, "kernel": capi.fd_shared_vectors_fp64_kernel_name(M, F, kind),
                              "ms_per_call": {k: round(v, 4) for k, v in ms.items()}, "vectors_ms_new": round(new_v, 4),
                              "vectors_ms_per_context": round(old_v, 4), "ratio_per_context_over_new": round(old_v / new_v, 3)}), flush=True)
            batch.close()
        full.close()
        for e in engines:
            e.set_stream(None); e.close()


if __name__ == "__main__":
    main()
