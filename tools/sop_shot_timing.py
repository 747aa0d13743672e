"""Host-to-host time of FaceDeformSOP.cook_shot against F sequential cooks, in one process.

For N = 1M vertices, M = 256 control points and F in {1, 2, 4, 8, 16, 32, 64}: the wall-clock time of one
cook_shot(F frames) against F cook(..., rig_rest_unchanged=True, mesh_unchanged=True) calls on a node of its own
(unchanged code: the figure a caller had before fdsop_cook_shot), for the node's defaults (QNN, linear term), kernel = 1
(thin-plate) and model = 1 (multilayer), each with page-locked and with pageable output arrays.  Both calls end with the
results in the caller's arrays, so the clock needs no further synchronisation.  The two variants alternate, round by
round; the table prints the median of the rounds and the ratio sequential / shot.

    python tools/sop_shot_timing.py [--out FILE] [--n N] [--m M] [--frames 1,2,4,...] [--rounds R]

DESIGN.md 4.8 holds the table this printed on an MI355X."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facedeform_amd import capi, synth          # noqa: E402
from facedeform_amd.sop import FaceDeformSOP    # noqa: E402

MODELS = (("defaults (QNN)", {}), ("kernel = 1", {"kernel": 1}), ("model = 1", {"model": 1}))


def _node(parms):
    node = FaceDeformSOP()
    for k, v in parms.items():
        node.set(k, v)
    return node


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--frames", default="1,2,4,8,16,32,64")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    Fs = [int(x) for x in args.frames.split(",")]
    Fmax = max(Fs)
    P = synth.head_mesh(args.n)
    rest = synth.control_points(args.m, "head")
    frames = [synth.deformed_rig(rest, k) for k in range(Fmax)]
    N = P.shape[0]
    outs = {"page-locked": ([capi.host_array((N, 3)) for _ in range(Fmax)], [capi.host_array((N,)) for _ in range(Fmax)]),
            "pageable": ([np.empty((N, 3), np.float32) for _ in range(Fmax)], [np.empty(N, np.float32) for _ in range(Fmax)])}
    for o, f in outs.values():           # touch every page before anything is timed
        for a in o + f:
            a.fill(0)
    lines = [f"# N = {N}, M = {args.m}; median of {args.rounds} alternating rounds; ms host to host",
             "model | outputs | F | cook_shot ms | F cooks ms | cooks / shot | ms per frame (shot) | paths"]
    for name, parms in MODELS:
        shot_node, seq_node = _node(parms), _node(parms)
        for memory, (oP, oF) in outs.items():
            # both nodes see the mesh and the rig once, untimed
            shot_node.cook_shot(P, rest, frames[:2], out_P=oP[:2], out_falloff=oF[:2], want_Cd=False)
            seq_node.cook(P, rest, frames[0], out_P=oP[0], out_falloff=oF[0], want_Cd=False)
            for F in Fs:
                t_shot, t_seq, paths = [], [], None
                for r in range(args.rounds + 1):               # round 0 warms this F up
                    t0 = time.perf_counter()
                    res = shot_node.cook_shot(P, rest, frames[:F], out_P=oP[:F], out_falloff=oF[:F], want_Cd=False,
                                              rig_rest_unchanged=True, mesh_unchanged=True)
                    t1 = time.perf_counter()
                    for k in range(F):
                        c = seq_node.cook(P, rest, frames[k], out_P=oP[k], out_falloff=oF[k], want_Cd=False,
                                          rig_rest_unchanged=True, mesh_unchanged=True)
                        assert c.severity < capi.FDSOP_ERROR, c.messages
                    t2 = time.perf_counter()
                    assert res.severity < capi.FDSOP_ERROR, (res.messages, [f.messages for f in res.frames])
                    if r:
                        t_shot.append((t1 - t0) * 1e3); t_seq.append((t2 - t1) * 1e3)
                    paths = res.paths
                a, b = _median(t_shot), _median(t_seq)
                lines.append(f"{name} | {memory} | {F} | {a:.2f} | {b:.2f} | {b / a:.2f} | {a / F:.3f} | "
                             + "; ".join(f"{p[0]}+{p[1]}: build '{p[2]}' eval32 '{p[3]}' x{p[4]} eval64 '{p[5]}' x{p[6]}" for p in paths))
                print(lines[-1], flush=True)
        shot_node.close(); seq_node.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
