"""fd_deform_adjoint_shot_dev beside F calls of fd_deform_adjoint_dev, and fd_fit_deltas_shot beside F calls of fd_fit_deltas,
timed on one device.

1M head vertices, 256 control points, thin-plate and QNN, rig_deltas x 1, no dist2, no projection frames, omega = 1;
F = 1, 2, 4, 8, 16, 32.
  (a) between two events on one stream, alternating rounds in one process, medians of 25 with min and max:
        shot     fd_deform_adjoint_shot_dev on F cotangents: one matrix-pipe launch and one reduce launch;
        singles  F calls of fd_deform_adjoint_dev, one per cotangent, back to back.
      The rate counts 2 (C+4) 3F N flop against the 78.6 TFLOP/s fp64 matrix peak at 2.4 GHz; the clock the launches held is
      not read here.
  (b) host wall clock around the calls (host arrays, S given), medians of --fits:
        shot     one fd_fit_deltas_shot on F targets, with its report's four stage times;
        singles  F calls of fd_fit_deltas, one per target.
Nothing is asserted on time.
   python tests/tools/fit_shot_timing.py [--out profiles/fit_shot_timing.txt] [--rounds 5] [--per-round 5] [--fits 3]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]
FRAMES = (1, 2, 4, 8, 16, 32)
PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fit_shot_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    ap.add_argument("--fits", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_shot_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    fmax = max(FRAMES)
    P = synth.head_mesh(n)
    G = np.random.default_rng(11).standard_normal((fmax,) + P.shape).astype(np.float32)
    T = (P[None] + G * np.float32(0.01)).astype(np.float32)
    rest = synth.control_points(M, "head")
    nn = M + 4
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, rig_deltas x 1, no dist2, no projection, omega = 1",
             f"# (a) ms between two events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs "
             f"each: median (min .. max).  shot: fd_deform_adjoint_shot_dev; singles: F x fd_deform_adjoint_dev.  rate: 2 (C+4) 3F N flop, "
             f"of {PEAK / 1e12:.1f} TFLOP/s (the clock was not read)",
             f"# (b) host wall clock, ms, medians of {args.fits}, host arrays, S given.  shot: fd_fit_deltas_shot with its report's stage "
             f"times; singles: F x fd_fit_deltas"]
    for name, kind, params in KINDS:
        e = capi.Engine(device=0, precision=capi.EVAL_FP64)
        e.set_stream(S.cuda_stream)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        assert e.build().terminationtype == 1
        with torch.cuda.stream(S):
            d_P = torch.from_numpy(P).to(dev); d_G = torch.from_numpy(G).to(dev)
            d_shot = torch.empty((fmax, nn, 3), dtype=torch.float64, device=dev)
            d_single = torch.empty((fmax, nn, 3), dtype=torch.float64, device=dev)
        S.synchronize()
        frame_bytes = n * 3 * 4

        def timed(fn, reps, keep):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S); fn(); e1.record(S); S.synchronize()
                if keep:
                    ts.append(e0.elapsed_time(e1))
            return ts

        lines.append(f"{name}:")
        print(lines[-1], flush=True)
        ahead = None
        for F in FRAMES:
            def shot():
                e.deform_adjoint_shot_dev(n, F, d_P.data_ptr(), d_G.data_ptr(), d_shot.data_ptr())

            def singles():
                for f in range(F):
                    e.deform_adjoint_dev(n, d_P.data_ptr(), d_G.data_ptr() + f * frame_bytes, d_single.data_ptr() + f * nn * 3 * 8)

            fns = {"shot": shot, "singles": singles}
            t = {k: [] for k in fns}
            for fn in fns.values():
                timed(fn, args.warmup, False)
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    t[k] += timed(fn, args.per_round, True)
            med = {k: float(np.median(v)) for k, v in t.items()}
            diff = float((d_shot[:F] - d_single[:F]).abs().max() / d_single[:F].abs().max())
            flop = 2.0 * nn * 3 * F * n
            if ahead is None and med["shot"] < med["singles"]:
                ahead = F
            lines.append(f"  (a) F = {F:2d}  shot {med['shot']:8.3f} ({min(t['shot']):.3f} .. {max(t['shot']):.3f})   "
                         f"singles {med['singles']:8.3f} ({min(t['singles']):.3f} .. {max(t['singles']):.3f})   singles / shot "
                         f"{med['singles'] / med['shot']:5.2f}   {flop / med['shot'] / 1e9:5.2f} TFLOP/s = {flop / med['shot'] * 1e3 / PEAK:.3f} "
                         f"of the peak   max |shot - singles| / max |singles| = {diff:.1e}")
            print(lines[-1], flush=True)
        lines.append(f"  (a) the shot launch is ahead from F = {ahead}" if ahead else "  (a) the shot launch is ahead at no F measured")
        print(lines[-1], flush=True)
        Sop = e.solve_operator()
        mu = 1e-8 * n
        ahead = None
        for F in FRAMES:
            w_shot, w_single, reps = [], [], []
            for k in range(args.fits + 1):
                t0 = time.perf_counter()
                _, rep = e.fit_deltas_shot(P, T[:F], mu=mu, S=Sop)
                t1 = time.perf_counter()
                for f in range(F):
                    e.fit_deltas(P, T[f], mu=mu, S=Sop)
                t2 = time.perf_counter()
                if k:                                       # the first pass warms the buffers up
                    w_shot.append((t1 - t0) * 1e3); w_single.append((t2 - t1) * 1e3); reps.append(rep[0])
            ms, m1 = float(np.median(w_shot)), float(np.median(w_single))
            parts = {k: float(np.median([getattr(r, k) for r in reps])) for k in ("ms_gram", "ms_adjoint", "ms_compose", "ms_solve")}
            if ahead is None and ms < m1:
                ahead = F
            lines.append(f"  (b) F = {F:2d}  shot {ms:9.2f} (gram {parts['ms_gram']:.2f}  adjoint {parts['ms_adjoint']:.2f}  compose "
                         f"{parts['ms_compose']:.2f}  solve {parts['ms_solve']:.2f})   singles {m1:9.2f}   singles / shot {m1 / ms:5.2f}")
            print(lines[-1], flush=True)
        lines.append(f"  (b) the shot fit is ahead from F = {ahead}" if ahead else "  (b) the shot fit is ahead at no F measured")
        print(lines[-1], flush=True)
        e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
