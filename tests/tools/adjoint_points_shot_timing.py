"""fd_batch_deform_adjoint_points_shared_dev against the two routes to sum_f A_f^T g_f it replaces, timed on one device
(DESIGN.md 4.13b).

1M head vertices, 256 control points, linear term, dist2 (random, below radius2: no vertex gated, every vertex with its own
fall-off) and projection frames; rig_deltas scaled per frame; G random normal.  F in {1, 2, 3, 4, 8, 16, 32} for thin-plate and
QNN, F <= 4 for biharmonic and cubic.  Between two events on one stream, alternating rounds in one process, medians of 25:
  call      fd_batch_deform_adjoint_points_shared_dev as the library routes it (the `route` column says which way);
  per-ctx   (a) F x fd_deform_adjoint_points_dev into F arrays, then the F - 1 additions in frame order (torch, fp64);
  jacobian  (b) fd_batch_deform_vectors_shared_fp64_dev with the Jacobian output alone (it evaluates the positions as well: the
            call has no form without them), then torch.einsum over the stored fp32 A and the sum over the frames.
`spread` is max - min of the 25 times of `call` and of `per-ctx`, whichever is larger.  To time the one launch below the
library's thresholds as well, point FACEDEFORM_HIP_LIB at a library built with FD_EXTRA_HIPCC_FLAGS=-DFD_APS_MIN_FRAMES=1; the
header line records the thresholds of the library that ran.  The results of the three routes are compared, for the record;
nothing is asserted on time, and the clock the launches held is not read.
   python tests/tools/adjoint_points_shot_timing.py [--out profiles/adjoint_points_shot_timing.txt] [--rounds 5] [--per-round 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

N, M = 1_000_000, 256
RADIUS2, RATE = 0.36, 1.7
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, [], (1, 2, 3, 4, 8, 16, 32)), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0], (1, 2, 3, 4, 8, 16, 32)),
         ("biharmonic", capi.KERNEL_BIHARMONIC, [], (1, 2, 3, 4)), ("cubic", capi.KERNEL_CUBIC, [], (1, 2, 3, 4))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "adjoint_points_shot_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=N)
    ap.add_argument("--kinds", default=",".join(k[0] for k in KINDS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_points_shot_timing.py: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    n = args.vertices
    P = synth.head_mesh(n)
    tu, tv, nrm = synth.tangent_frames(P)
    dist2 = (np.random.default_rng(5).random(n) * RADIUS2).astype(np.float32)
    rest = synth.control_points(M, "head")
    rng = np.random.default_rng(11)
    name_of = capi.fd_shared_adjoint_points_kernel_name
    thresholds = {k[0]: next((F for F in range(1, 33) if name_of(M, F, k[1])), None) for k in KINDS}
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} head vertices, {M} control points, linear term, dist2 and projection frames; ms between "
             f"two events on one stream; {args.rounds} alternating rounds of {args.per_round} after {args.warmup} warm-up runs each; the clock "
             f"was not read",
             f"# the library's thresholds (fewest frames of the one launch): {thresholds}",
             "# call: fd_batch_deform_adjoint_points_shared_dev; per-ctx: F x fd_deform_adjoint_points_dev + F - 1 ordered additions; "
             "jacobian: fd_batch_deform_vectors_shared_fp64_dev(jacobian) + einsum + sum",
             f"# {'kind':10s} {'F':>2s} {'route':11s} {'call':>8s} {'min':>8s} {'max':>8s} | {'per-ctx':>8s} {'min':>8s} {'max':>8s} | {'jacobian':>8s} "
             f"{'min':>8s} {'max':>8s} | {'spread':>7s} {'per-ctx/call':>12s} {'jacobian/call':>13s} {'diff a':>8s} {'diff b':>8s}"]
    with torch.cuda.stream(S):
        d_P = torch.from_numpy(P).to(dev); d_d2 = torch.from_numpy(dist2).to(dev)
        d_tu, d_tv, d_nrm = (torch.from_numpy(a).to(dev) for a in (tu, tv, nrm))
    frames = (d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr())
    for name, kind, params, counts in KINDS:
        if name not in args.kinds.split(","):
            continue
        for F in counts:
            deltas = np.stack([synth.rig_deltas(rest, f % 8) * np.float32(0.5 + 0.05 * f) for f in range(F)]).astype(np.float32)
            engines = []
            for _ in range(F):
                e = capi.Engine(device=0)
                e.set_stream(S.cuda_stream)
                e.set_kernel(kind, list(params)); e.set_term(capi.TERM_LINEAR)
                engines.append(e)
            batch = capi.Batch(engines)
            with torch.cuda.stream(S):
                d_rest = torch.from_numpy(rest).to(dev); d_del = torch.from_numpy(deltas).to(dev)
                d_G = torch.from_numpy(rng.standard_normal((F, n, 3)).astype(np.float32)).to(dev)
                d_gp = torch.empty((n, 3), dtype=torch.float64, device=dev)
                d_per = torch.empty((F, n, 3), dtype=torch.float64, device=dev)
                d_pos = torch.empty((F, n, 3), dtype=torch.float32, device=dev)
                d_jac = torch.empty((F, n, 3, 3), dtype=torch.float32, device=dev)
            S.synchronize()
            batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
            batch.build_async(S.cuda_stream)
            assert [r.terminationtype for r in batch.build_result()] == [1] * F
            res = {}

            def call():
                batch.deform_adjoint_points_shared_dev(n, d_P.data_ptr(), d_G.data_ptr(), d_gp.data_ptr(), d_dist2=d_d2.data_ptr(),
                                                       d_tangents=frames, radius2=RADIUS2, falloffrate=RATE, stream_ptr=S.cuda_stream)

            def per_ctx():
                for f, e in enumerate(engines):
                    e.deform_adjoint_points_dev(n, d_P.data_ptr(), d_G[f].data_ptr(), d_per[f].data_ptr(), 0, d_d2.data_ptr(), *frames, RADIUS2, RATE)
                with torch.cuda.stream(S):
                    acc = d_per[0]
                    for f in range(1, F):
                        acc = acc + d_per[f]
                    res["a"] = acc

            def jacobian():
                batch.deform_vectors_shared_fp64_dev(n, d_P.data_ptr(), [d_pos[f].data_ptr() for f in range(F)], d_dist2=d_d2.data_ptr(),
                                                     d_tangents=frames, d_jacobian=[d_jac[f].data_ptr() for f in range(F)], radius2=RADIUS2,
                                                     falloffrate=RATE, stream_ptr=S.cuda_stream)
                with torch.cuda.stream(S):
                    res["b"] = torch.einsum("fvck,fvc->vk", d_jac, d_G)

            def timed(fn, reps, keep):
                ts = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(S); fn(); e1.record(S); S.synchronize()
                    if keep:
                        ts.append(e0.elapsed_time(e1))
                return ts

            fns = {"call": call, "per-ctx": per_ctx, "jacobian": jacobian}
            t = {k: [] for k in fns}
            for fn in fns.values():
                timed(fn, args.warmup, False)
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    t[k] += timed(fn, args.per_round, True)
            med = {k: float(np.median(v)) for k, v in t.items()}
            scale = float(d_gp.abs().max())
            da = float((d_gp - res["a"]).abs().max()) / scale
            db = float((d_gp - res["b"].double()).abs().max()) / scale
            spread = max(max(t["call"]) - min(t["call"]), max(t["per-ctx"]) - min(t["per-ctx"]))
            route = "one launch" if name_of(M, F, kind) else "per context"
            cols = " | ".join(f"{med[k]:8.3f} {min(t[k]):8.3f} {max(t[k]):8.3f}" for k in fns)
            lines.append(f"  {name:10s} {F:2d} {route:11s} {cols} | {spread:7.3f} {med['per-ctx'] / med['call']:12.2f} {med['jacobian'] / med['call']:13.2f} "
                         f"{da:8.1e} {db:8.1e}")
            print(lines[-1], flush=True)
            del d_G, d_per, d_pos, d_jac, res
            batch.close()
            for e in engines:
                e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
