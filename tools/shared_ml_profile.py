"""Times of fd_batch_deform_shared_ml_dev against the per-context launches fd_batch_deform_shared_dev runs for the same
multilayer batch, in one run -- meant to run under one rocprofv3 --kernel-trace --stats run of its own (no counters in it):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o shared_ml -- python tools/shared_ml_profile.py --csv OUT/shared_ml_grid.csv

1M-vertex head mesh, 256 control points, the SOP's defaults (radius 1, lambda 0.1, linear term); layers in {4, 8}, frames in
{1, 2, 3, 4, 8, 16, 32}.  Every vertex is live (no dist2), fd_falloff is written, no tangent frames.  The kernel names of the
trace do not tell the frame counts apart (one instantiation serves 22..32 frames, and 4 and 8 layers share one), so the grid
is timed here as well, with stream events around `--reps` back-to-back calls of each kind after a warm-up, and written as
CSV: per configuration the microseconds per call of the new launch (its pack kernel included), of the per-context launches,
and their ratio.  Where the call delegates (below its frame threshold) the row has no time of its own."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facedeform_amd import capi, synth   # noqa: E402


def timed(fn, reps, stream, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)            # on the stream the calls are given: events on another stream bracket nothing
        for _ in range(reps):
            fn()
        t1.record(stream)
        torch.cuda.synchronize()
        best.append(t0.elapsed_time(t1) * 1000.0 / reps)
    return sorted(best)[1]          # the median of three batches, microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--layers", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 2, 3, 4, 8, 16, 32])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--csv", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    M, N, Fmax = args.m, args.n, max(args.frames)
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(dev)
    deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(Fmax)]).astype(np.float32)
    d_rest, d_del = torch.from_numpy(rest).to(dev), torch.from_numpy(deltas).to(dev)
    outs = [torch.empty_like(d_P) for _ in range(Fmax)]
    falls = [torch.empty(N, device=dev) for _ in range(Fmax)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    # a stream of its own, handed to every call: torch's current stream is the null stream, whose handle 0 the library reads as
    # "the context's own stream", and events recorded on the null stream would then time the enqueueing, not the launches
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    rows = ["layers,frames,kernel,new_us,per_context_us,speedup,new_us_per_frame,per_context_us_per_frame"]
    for L in args.layers:
        engines = []
        for _ in range(Fmax):
            e = capi.Engine(device=0)
            e.set_stream(s)
            e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [1.0, L, 0.1]); e.set_term(capi.TERM_LINEAR)
            engines.append(e)
        full = capi.Batch(engines)
        full.set_points_dev([d_rest.data_ptr()] * Fmax, [d_del.data_ptr() + f * M * 12 for f in range(Fmax)], M)
        full.build_async(s)
        assert [r.terminationtype for r in full.build_result()] == [1] * Fmax
        for F in args.frames:
            batch = capi.Batch(engines[:F])
            name = capi.fd_shared_ml_kernel_name(M, L, F)
            old = timed(lambda: batch.deform_shared_dev(N, d_P.data_ptr(), ptr(outs[:F]), d_falloff=ptr(falls[:F]), stream_ptr=s), args.reps, stream)
            new = timed(lambda: batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr(outs[:F]), d_falloff=ptr(falls[:F]), stream_ptr=s), args.reps, stream) if name else float("nan")
            rows.append(f"{L},{F},{name},{new:.1f},{old:.1f},{old / new:.2f},{new / F:.1f},{old / F:.1f}")
            print(rows[-1], flush=True)
            batch.close()
        full.close()
        for e in engines:
            e.set_stream(None); e.close()
    if args.csv:
        os.makedirs(os.path.dirname(os.path.abspath(args.csv)), exist_ok=True)
        with open(args.csv, "w") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
