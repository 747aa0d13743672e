"""Times of fd_batch_deform_vectors_shared_ml_dev's vector launch (k_vectors32_shared_ml) against the parent's way to the
same result: fd_batch_deform_vectors_shared_dev on the same multilayer batch, which runs k_vectors32_gaussian over the
M L records once per context.

    python tools/vectors_shared_ml_profile.py [--out profiles/vectors_shared_ml_1M_256_events.csv]

1M-vertex head mesh, 256 control points, linear term, the multilayer model with L in {4, 8} layers; F in
{1, 2, 3, 4, 12, 13, 32} frames of one rest rig; dist2, projection frames and all four vector outputs (N, tu, tv, A) given.
Device events on the library's stream, after one warm-up call of every form; the four forms
    new                    fd_batch_deform_vectors_shared_ml_dev     pack + k_deform32_shared_ml + the vector launch
    new_positions          fd_batch_deform_shared_ml_dev             pack + k_deform32_shared_ml
    per_context            fd_batch_deform_vectors_shared_dev        F x (k_vectors32_gaussian + the one-frame position launch)
    per_context_positions  fd_batch_deform_shared_dev                F x the one-frame position launch
alternate within a round, `--rounds` rounds.  A timed window holds as many calls as fill `--window-ms` (at least `--reps`; the
count is taken from a timed second warm-up call and written to the CSV), so the short calls at few frames are timed over
hundreds of calls.  The CSV holds the median and the range of each form over the rounds and the two differences (vectors =
call - its position-only call).

The product library routes frame counts below shared_vectors_ml_min_frames to the per-context launches: there `new` measures
those and the `kernel` column is empty.  --force-launch times the launch itself at every frame count the position launch
takes (two frames and more: at one frame the call is fd_batch_deform_vectors_shared_dev whatever the threshold says), which is
how the threshold is found: it needs a tuning build of the library (FD_EXTRA_HIPCC_FLAGS=-DFD_TUNING python -m
facedeform_amd._build, or FACEDEFORM_HIP_LIB naming one), where FD_VML_MIN_FRAMES=1 puts the threshold at one frame, and refuses
to run on a library that keeps any layer count's threshold above two.

For kernel times by name, run the same script under rocprofv3 --kernel-trace --stats (a run of its own, no counters)."""
import argparse
import csv
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--force-launch" in sys.argv:
    os.environ["FD_VML_MIN_FRAMES"] = "1"            # read by tuning builds only, once, when the threshold is first asked for
from facedeform_amd import capi, synth   # noqa: E402

RADIUS2, RATE = 0.36, 1.7
FORMS = ("new", "new_positions", "per_context", "per_context_positions")


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
    ap.add_argument("--layers", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 2, 3, 4, 12, 13, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--force-launch", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "vectors_shared_ml_1M_256_events.csv"))
    args = ap.parse_args()
    if args.force_launch and any(capi.fd_shared_vectors_ml_kernel_name(args.m, L, 2) == "" for L in range(1, 9)):
        sys.exit("--force-launch needs a tuning build of the library (-DFD_TUNING): this one ignores FD_VML_MIN_FRAMES")
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
    rows = []
    for L in args.layers:
        engines = []
        for _ in range(Fmax):
            e = capi.Engine(device=0)
            e.set_stream(stream.cuda_stream)
            e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [1.0, L, 0.1]); e.set_term(capi.TERM_LINEAR)
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
                "new": lambda: batch.deform_vectors_shared_ml_dev(N, d_P.data_ptr(), ptr(oP, F), **common, **vec),
                "new_positions": lambda: batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr(oP, F), **common),
                "per_context": lambda: batch.deform_vectors_shared_dev(N, d_P.data_ptr(), ptr(oP, F), **common, **vec),
                "per_context_positions": lambda: batch.deform_shared_dev(N, d_P.data_ptr(), ptr(oP, F), **common),
            }
            reps = {}
            for key in FORMS:
                calls[key]()                                   # warm-up: code objects, scratch
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(stream); calls[key](); ev1.record(stream)
                torch.cuda.synchronize()
                reps[key] = max(args.reps, math.ceil(args.window_ms / max(ev0.elapsed_time(ev1), 1e-3)))
            ms = {key: [] for key in FORMS}
            for _ in range(args.rounds):
                for key in FORMS:                              # the forms alternate within a round
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record(stream)
                    for _ in range(reps[key]):
                        calls[key]()
                    ev1.record(stream)
                    torch.cuda.synchronize()
                    ms[key].append(ev0.elapsed_time(ev1) / reps[key])
            med = {k: statistics.median(v) for k, v in ms.items()}
            new_v = med["new"] - med["new_positions"]
            old_v = med["per_context"] - med["per_context_positions"]
            row = {"N": N, "M": M, "layers": L, "frames": F, "kernel": capi.fd_shared_vectors_ml_kernel_name(M, L, F)}
            for k in FORMS:
                row[k + "_reps"] = reps[k]; row[k + "_ms"] = round(med[k], 4); row[k + "_min_ms"] = round(min(ms[k]), 4); row[k + "_max_ms"] = round(max(ms[k]), 4)
            row.update(vectors_new_ms=round(new_v, 4), vectors_per_context_ms=round(old_v, 4), per_context_over_new=round(old_v / new_v, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            batch.close()
        full.close()
        for e in engines:
            e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


if __name__ == "__main__":
    main()
