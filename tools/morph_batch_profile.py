"""Kernel times of the batched morph-space passes against the per-frame launches they replace, for one rocprofv3
--kernel-trace --stats run (kernel trace only: no counters in the same run), under a time limit of its own:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o morph_batch -- \\
        python tools/morph_batch_profile.py
    python tools/morph_batch_profile.py --summarise OUT/morph_batch_kernel_trace.csv \\
        --out profiles/morph_batch_1M_50_32_kernel_stats.csv

1M-vertex head mesh, 50 synthetic blendshapes (Gaussian bumps), 32 frames that are mixtures of them.  After one warm-up
each, `--reps` rounds of the 32 per-frame calls (k_morph_weights + k_morph_weights_reduce, then k_morph_displace) and
as many batched pairs (k_morph_weights_batch + k_morph_weights_batch_reduce, k_morph_displace_batch) run on the same arrays,
clamp on, no add_delta, so one trace holds both.  --summarise turns the trace into per-kernel medians, the medians of
the per-round sums, the algorithmic bytes of DESIGN.md 6b, the achieved TB/s and its fraction of the 8 TB/s roof."""
import argparse
import csv
import os
import statistics
import sys

ROOF_TBPS = 8.0


def run(args):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from facedeform_amd import capi, synth

    dev = torch.device("cuda", 0)
    N, S, F = args.n, args.shapes, args.frames
    rng = np.random.default_rng(3)
    rest_h = synth.head_mesh(N)
    rest = torch.from_numpy(rest_h).to(dev)
    shapes = []
    for s in range(S):
        centre = torch.from_numpy(rest_h[rng.integers(N)]).to(dev)
        wgt = torch.exp(-((rest - centre) ** 2).sum(dim=1) / 0.05)
        bump = torch.from_numpy((0.1 * rng.normal(size=3)).astype(np.float32)).to(dev)
        shapes.append((rest + wgt[:, None] * bump).contiguous())
    frames = []
    for f in range(F):
        a, b = int(rng.integers(S)), int(rng.integers(S))
        frames.append((rest + float(rng.uniform(-0.6, 0.9)) * (shapes[a] - rest) + float(rng.uniform(-0.6, 0.9)) * (shapes[b] - rest)).contiguous())
    torch.cuda.synchronize()
    m = capi.Morph()
    m.init_dev(N, rest.data_ptr(), [t.data_ptr() for t in shapes])
    ptrs = [t.data_ptr() for t in frames]
    clamp = (-0.5, 0.5)
    for rep in range(args.reps + 1):
        for p in ptrs:
            m.compute_weights_dev(p)
        for p in ptrs:
            m.displace_dev(p, clamp, False, 0.0)
    m.weights()
    for rep in range(args.reps + 1):
        m.compute_weights_batch_dev(ptrs)
        m.displace_batch_dev(ptrs, clamp, False, 0.0)
    w = m.weights_batch()
    print(f"{args.reps + 1} rounds of {F} per-frame weight and displacement calls and as many batched pairs, {N} vertices, "
          f"S = {S}; init {m.last_init_ms:.1f} ms; max|3 w| = {np.abs(3 * w).max():.3f}")
    m.close()


def summarise(args):
    N, S, F = args.n, args.shapes, args.frames
    spans = {}
    with open(args.summarise, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            if "k_morph_" in name:
                spans.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    # names are matched from the most specific: "..._batch_reduce", "..._batch", then the per-frame ones
    def of(key):
        names = [k for k in spans if key in k]
        if not key.endswith("reduce"):
            names = [k for k in names if "reduce" not in k]
        if "batch" not in key:
            names = [k for k in names if "batch" not in k]
        assert len(names) == 1, (key, names)
        return names[0], [d for _, d in sorted(spans[names[0]])]

    rows3 = 3 * N
    bytes_of = {"k_morph_weights": 8 * rows3 * S + 2 * 4 * rows3, "k_morph_displace": 4 * rows3 * S + 2 * 12 * N,
                "k_morph_weights_batch": 8 * rows3 * S + (F + 1) * 4 * rows3, "k_morph_displace_batch": 4 * rows3 * S + (F + 1) * 12 * N}
    out = [["Name", "Calls", "MedianNs", "MinNs", "MaxNs", "AlgorithmicBytes", "TBps", "FractionOfRoof"]]
    med = {}
    for key in ("k_morph_weights", "k_morph_weights_reduce", "k_morph_displace", "k_morph_weights_batch", "k_morph_weights_batch_reduce",
                "k_morph_displace_batch"):
        name, d = of(key)
        if "batch" in key:
            d = d[1:]                                             # the warm-up call
        else:
            d = d[F:]                                             # the warm-up round
        med[key] = statistics.median(d)
        b = bytes_of.get(key)
        tb = b / med[key] / 1e3 if b else None
        out.append([name, len(d), f"{med[key]:.0f}", min(d), max(d), b or "", f"{tb:.3f}" if tb else "", f"{tb / ROOF_TBPS:.3f}" if tb else ""])
        if "batch" not in key:
            rounds = [sum(d[i:i + F]) for i in range(0, len(d) - F + 1, F)]
            med[key + "_round"] = statistics.median(rounds)
            out.append([f"sum of {F} launches of {key}, per round", len(rounds), f"{med[key + '_round']:.0f}", min(rounds), max(rounds),
                        F * b if b else "", "", ""])
    per_w = med["k_morph_weights_round"] + med["k_morph_weights_reduce_round"]
    bat_w = med["k_morph_weights_batch"] + med["k_morph_weights_batch_reduce"]
    out.append([f"weights: {F} per-frame launch pairs / batched pair", "", f"{per_w:.0f} / {bat_w:.0f}", "", "", "", f"ratio {per_w / bat_w:.2f}", "bar 5"])
    out.append([f"displacement: {F} per-frame launches / batched launch", "", f"{med['k_morph_displace_round']:.0f} / {med['k_morph_displace_batch']:.0f}",
                "", "", "", f"ratio {med['k_morph_displace_round'] / med['k_morph_displace_batch']:.2f}", "bar 5"])
    with open(args.out, "w", newline="") as fh:
        csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC).writerows(out)
    for r in out:
        print(",".join(str(x) for x in r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--shapes", type=int, default=50)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarise", help="a rocprofv3 kernel trace (csv) of a run of this tool")
    ap.add_argument("--out", default="profiles/morph_batch_1M_50_32_kernel_stats.csv")
    args = ap.parse_args()
    summarise(args) if args.summarise else run(args)


if __name__ == "__main__":
    main()
