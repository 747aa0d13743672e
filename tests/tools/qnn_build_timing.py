"""Batched builds of a shot of QNN models, timed: fd_batch_set_points_dev + fd_batch_build_async between two events on one
stream, with fd_batch_set_shared_lu on (one LU of the rest rig's kernel block, k_qnn_solve_shared) and off
(every model built on its own: fd_batch_build_async as it was before the switch existed -- the same code, launch for
launch).  Both are taken in the same process on the same device, in alternating rounds.
   python tests/tools/qnn_build_timing.py [--out profiles/qnn_shared_build_timing.txt] [--rounds 5] [--per-round 20]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from facedeform_amd import capi, synth

SIZES = [(M, F) for M in (256, 1000) for F in (2, 4, 8, 16, 32)]
Q, Z = 1.0, 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "qnn_shared_build_timing.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qnn_build_timing.py: no GPU -- a build time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    S = torch.cuda.Stream(device=dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; set_points_dev + build_async between two events on one stream, ms per build of the "
             f"whole batch; {args.rounds} alternating rounds of {args.per_round} builds each after {args.warmup} warm-up builds per path",
             "# off: every model on its own (the per-context chain, captured graph); on: one LU without pivot search + k_qnn_solve_shared",
             f"# {'M':>4} {'F':>3} | {'off median':>10} {'off min':>8} | {'on median':>10} {'on min':>8} | off/on | max |W_on - W_off| / max |W|"]
    for M, F in SIZES:
        rest = synth.control_points(M, "head")
        deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
        d_rest = torch.from_numpy(rest).to(dev); d_del = torch.from_numpy(deltas).to(dev)
        engines = []
        for _ in range(F):
            e = capi.Engine(); e.set_stream(S.cuda_stream)
            e.set_kernel(capi.KERNEL_GAUSSIAN_QNN, [Q, Z, 0.0]); e.set_term(capi.TERM_LINEAR)
            engines.append(e)
        batch = capi.Batch(engines)
        rp, dp = [d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)]
        # the switch-on path is whatever the library takes at this size: below its minimum frame count that is the per-context build
        takes = capi.fd_shared_qnn_build_kernel_name(M, F) != ""

        def build(on, n, timed):
            batch.set_shared_lu(on)
            ts = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(S)
                batch.set_points_dev(rp, dp, M)
                batch.build_async(S.cuda_stream)
                e1.record(S)
                S.synchronize()
                assert batch.last_build_shared_factor() is (on and takes)
                if timed:
                    ts.append(e0.elapsed_time(e1))
            return ts

        W = {}
        for on in (False, True):
            build(on, args.warmup, False)
            assert [r.terminationtype for r in batch.build_result()] == [1] * F
            W[on] = [e.get_weights()[0] for e in engines]
        apart = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(W[True], W[False]))
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                t[on] += build(on, args.per_round, True)
        off, on_ = np.array(t[False]), np.array(t[True])
        lines.append(f"  {M:4d} {F:3d} | {np.median(off):10.4f} {off.min():8.4f} | {np.median(on_):10.4f} {on_.min():8.4f} | "
                     f"{np.median(off) / np.median(on_):6.2f} | {apart:.2e}{'' if takes else '   (below the minimum frame count: per context)'}")
        print(lines[-1], flush=True)
        batch.close()
        for e in engines:
            e.set_stream(None); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
