"""bench.py --dump-outputs DIR: after the timed steps the benchmark writes what its timed path computed for the last
step -- the deformed positions and the fall-off of that frame -- as DIR/<name>.npy (float32 / float64, 64 MB at most, a
fixed seeded row sample beyond that), so that two builds run with the same arguments can be compared output for output.

CPU: the writer itself (budget, sampling, dtypes, determinism) and the flag's presence.
GPU: the benchmark's own dump held to the oracle for the frame of its last timed step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT, l2_parity_ulp


def test_dump_writes_every_array_whole_under_the_budget(tmp_path):
    P = np.arange(30, dtype=np.float32).reshape(10, 3)
    fall = np.linspace(0, 1, 10).astype(np.float32)
    shapes = bench.dump_outputs(str(tmp_path), {"deformed_P": P, "falloff": fall, "w": np.arange(10, dtype=np.int32)})
    assert shapes == {"deformed_P": [10, 3], "falloff": [10], "w": [10]}
    assert sorted(os.listdir(tmp_path)) == ["deformed_P.npy", "falloff.npy", "w.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "deformed_P.npy"), P)
    assert np.load(tmp_path / "deformed_P.npy").dtype == np.float32
    assert np.load(tmp_path / "w.npy").dtype == np.float64            # other dtypes widen to float64


def test_dump_samples_the_same_rows_of_every_array_over_the_budget(tmp_path):
    n = 5000
    P = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    fall = np.arange(n, dtype=np.float32)
    budget = 4096
    bench.dump_outputs(str(tmp_path / "a"), {"deformed_P": P, "falloff": fall}, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), {"deformed_P": P, "falloff": fall}, budget=budget)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    rows = np.load(tmp_path / "a" / "row_index.npy")
    assert 0 < rows.size < n and total <= budget + 3 * 128               # (+ one .npy header per file)
    assert np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "deformed_P.npy"), P[r])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "falloff.npy"), fall[r])
    for f in os.listdir(tmp_path / "a"):                                  # fixed seed: the same sample every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_refuses_arrays_of_different_lengths(tmp_path):
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(3, np.float32), "b": np.zeros(4, np.float32)})


def test_bench_offers_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_the_dump_is_the_last_timed_step_and_matches_the_oracle(tmp_path, oracle):
    """C2, 70 timed steps in groups of 32: the last step is frame 5 of the third group (lane 2 of 3), delta phase 69 % 64 = 5.
    Its dumped positions agree with the oracle's deformation of that phase on a sample of vertices, and every vertex was
    written with fall-off 1 (no dist2 input)."""
    from facedeform_amd import synth
    from oracle import fd_oracle as fo
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "70", "--warmup", "0",
                        "--no-cpu-baseline", "--no-shared-factor-alternative", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    assert '"metric"' in r.stdout and '"steps": 70' in r.stdout
    n_verts, n_ctrl, mesh, _ = bench.CONFIGS["c2"]
    out = np.load(out_dir / "deformed_P.npy")
    fall = np.load(out_dir / "falloff.npy")
    assert out.shape == (n_verts, 3) and out.dtype == np.float32
    assert fall.shape == (n_verts,) and np.all(fall == 1.0)
    assert np.isfinite(out).all()
    P = synth.head_mesh(n_verts)
    rest = synth.control_points(n_ctrl, mesh)
    delta = synth.smooth_deltas(rest, 69 % bench.N_FRAMES)
    idx = np.unique(np.concatenate([np.arange(512), n_verts - 512 + np.arange(512),
                                    np.random.default_rng(3).choice(n_verts, 4000, replace=False)]))
    Ps = np.ascontiguousarray(P[idx])
    table = np.concatenate([rest, delta], axis=1).astype(np.float64)       # bench.py uploads these fp32 deltas as they are
    rc, tt, W, radii = oracle.build(table, fo.KERNEL_THIN_PLATE, [], fo.TERM_LINEAR)
    assert tt == 1
    ref, _ = oracle.deform(table, fo.KERNEL_THIN_PLATE, radii, W, Ps)
    assert l2_parity_ulp(out[idx], ref, Ps) <= 1.0
