"""CPU: the plan of the shared-rig fp32 launch (facedeform_amd/csrc/fd_shared_plan.h) against the arithmetic it replaced.
tests/tools/shared_plan_check.cpp includes that header alone and prints every field of shared_plan for Mpad in 16, 32, .., 640,
1024, 2048, 4096, 1 to 32 frames, thin-plate and QNN; tests/golden/shared_plan_table.txt holds the same columns as the commit
before the header computed them in launch_deform_shared, shared_wtile_bytes, shared_frame_bytes, shared_kernel_name and
shared_packing (recorded once by a program that carried those expressions verbatim; its first line names the commit).  The
GPU tests of the launch (test_gpu_shared.py) read the variant boundaries from the same table."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facedeform_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "shared_plan_table.txt")
COLUMNS = ("Mpad nF kind variant ntiles nslot nkb kchunk poly_at copy_at norm_at wtile_bytes frame_bytes lds_fixed lds_per_kb "
           "threads group_vertices kernel").split()
THIN_PLATE = 2


def parse(text):
    """{(Mpad, nF, kind): {column: value}} of the table's lines; every column but the kernel's name is an integer"""
    rows = {}
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        w = line.split()
        assert len(w) == len(COLUMNS), line
        r = {c: (v if c == "kernel" else int(v)) for c, v in zip(COLUMNS, w)}
        key = (r["Mpad"], r["nF"], r["kind"])
        assert key not in rows, line
        rows[key] = r
    return rows


def golden():
    with open(TABLE) as f:
        text = f.read()
    assert text.splitlines()[1].split()[1:] == COLUMNS
    return parse(text)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("shared_plan") / "shared_plan_check")
    # (sanitizers linked statically, as in test_fit_host.py: the shared ASan runtime refuses to start beside a preloaded library)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "shared_plan_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return parse(r.stdout)


def test_the_table_covers_the_cases():
    want = {(M, F, k) for M in list(range(16, 641, 16)) + [1024, 2048, 4096] for F in range(1, 33) for k in (THIN_PLATE, 1)}
    assert set(golden()) == want


def test_every_field_is_the_parents(plan):
    ref = golden()
    assert set(plan) == set(ref)
    for key, want in ref.items():
        got = plan[key]
        for c in COLUMNS:
            if c != "wtile_bytes":
                assert got[c] == want[c], (key, c, got[c], want[c])
        # the scratch is the variant's own extent: never more than it was, and all of what the pack kernel writes
        assert (got["norm_at"] + 1) * 16 <= got["wtile_bytes"] <= want["wtile_bytes"], (key, got["wtile_bytes"], want["wtile_bytes"])
        if got["variant"] in (0, 1):
            assert got["wtile_bytes"] == want["wtile_bytes"], key


def boundary(rows, nF):
    """(Mpad, Mpad + 16): the last shape of nF frames that runs k_deform32_shared_w1 and the first that is staged in chunks"""
    w1 = [M for (M, F, k), r in rows.items() if F == nF and k == THIN_PLATE and r["kernel"] == "k_deform32_shared_w1"]
    return max(w1), max(w1) + 16


@pytest.mark.parametrize("nF", [32, 20])
def test_residency_boundary(plan, nF):
    """One Mpad whose kernel is the one-tile kernel and the next whose kernel is the two-tile one, in the table and in the plan;
    below the boundary every shape is resident, above it none (the table decides where it lies: 352 | 368 at 32 frames,
    512 | 528 at 20 as recorded)."""
    ref = golden()
    lo, hi = boundary(ref, nF)
    print("nF=%d: %d resident, %d staged" % (nF, lo, hi))
    for rows in (ref, plan):
        for kind in (THIN_PLATE, 1):
            a, b = rows[(lo, nF, kind)], rows[(hi, nF, kind)]
            assert (a["kernel"], a["variant"]) == ("k_deform32_shared_w1", 3)
            assert (b["kernel"], b["variant"]) == ("k_deform32_tps_shared_wide", 2)
            assert a["kchunk"] == a["nkb"] and b["kchunk"] < b["nkb"]
            for (M, F, k), r in rows.items():
                if F == nF and k == kind:
                    assert (r["variant"] == 3) == (M <= lo), (M, F, k)
