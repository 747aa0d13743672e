"""CPU: the ABI of fd_batch_deform_adjoint_points_shared_dev, and the contraction its launch rests on, restated in numpy.

The identity: with r_f = f Pi g_f per vertex,
    sum_f J_f^T r_f = sum_j grad phi_j s_j + sum_f L_f^T r_f,      s_j = sum_{f,b} w_{f,j,b} r_{f,b},
checked in fp64 on random small inputs for every kind, with s and sum_f L_f^T r_f formed the way the launch forms them: from
operand arrays filled by the dealing of facedeform_amd/csrc/fd_adjoint_points_shot.h -- the inline functions the pack kernel
calls, compiled for the host into tests/tools/adjoint_points_shot_dealing.cpp's table -- and contracted as
v_mfma_f64_16x16x4_f64 contracts them (lane l of the A operand: row l & 15, depth slot l >> 4)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_points_cases as cases
from facedeform_amd import _build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fd_batch_deform_adjoint_points_shared_dev", "fd_shared_adjoint_points_kernel_name")


def test_header_library_and_bindings_agree(hip_lib):
    header = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    assert re.search(r"\bint fd_batch_deform_adjoint_points_shared_dev\(fd_batch \*batch, void \*hip_stream, int64_t N, const float \*d_P_in,\s*"
                     r"const float \*d_G, const float \*d_dist2,\s*const float \*d_tu, const float \*d_tv, const float \*d_nrm,\s*"
                     r"float radius2, float falloffrate, double \*d_grad_P\);", header)
    assert re.search(r"\bconst char \*fd_shared_adjoint_points_kernel_name\(int M, int frames, int kind\);", header)
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
        assert getattr(capi.load(), name).argtypes is not None
    assert lib.fd_abi_version() == 9 and re.search(r"#define FD_ABI_VERSION 9\b", header)
    assert hasattr(capi.Batch, "deform_adjoint_points_shared_dev")


def test_kernel_name_needs_no_device(hip_lib):
    name = capi.fd_shared_adjoint_points_kernel_name
    assert name(64, 32, capi.KERNEL_THIN_PLATE) == "k_adjoint_points64_shot"
    assert name(64, 1, capi.KERNEL_THIN_PLATE) == "" and name(64, 4, capi.KERNEL_GAUSSIAN_ML) == ""
    assert name(0, 4, capi.KERNEL_THIN_PLATE) == "" and name(64, 33, capi.KERNEL_THIN_PLATE) == ""


def test_the_new_source_owns_nothing_by_hand():
    """tests/test_shared_qnn_build_abi.py's rule: device memory, events and streams are released by fd_owned.h's owners."""
    for f in ("fd_adjoint_points_shot.hip", "fd_adjoint_points_shot.h"):
        src = open(os.path.join(_build.CSRC, f)).read()
        for word in ("hipFree", "hipEventDestroy", "hipStreamDestroy"):
            assert word not in src, (f, word)
    assert "fd_adjoint_points_shot.hip" in _build.SOURCES


@pytest.fixture(scope="module")
def dealing(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.path.dirname(_build.hipcc_path()), "..", "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path_factory.mktemp("aps") / "dealing")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", _build.CSRC, os.path.join(ROOT, "tests", "tools", "adjoint_points_shot_dealing.cpp"), "-o", exe])

    def table(nq, Mpad):
        out = subprocess.check_output([exe, str(nq), str(Mpad)]).decode().split("\n")
        rows = {k: [] for k in "WASL"}
        for line in out:
            if line:
                rows[line[0]].append([int(x) for x in line.split()[1:]])
        return {k: np.array(v) for k, v in rows.items()}
    return table


def test_lds_arithmetic(dealing):
    """The figures tests/test_gpu_adjoint_points_shot.py takes its M from: at 32 frames 11 tiles of 16 centres stay in LDS."""
    L = dealing(1, 16)["L"]
    assert L[:, 0].tolist() == list(range(1, 9))
    nq, fixed, per_tile, tiles = L[7]
    assert (fixed, per_tile) == (8 * (16 + 24 * 64), 8 * (64 + 24 * 64)) and tiles == (158 * 1024 - fixed) // per_tile == 11
    assert 16 * tiles == 176                     # M_RESIDENT; 177 pads to 192 centres, 12 tiles: staged
    assert all(t * p + f <= 158 * 1024 < (t + 1) * p + f for _, f, p, t in L)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("F,M", [(1, 16), (5, 33), (13, 20)])
def test_the_contraction_restated(dealing, kind, F, M):
    rng = np.random.default_rng(100 * F + M)
    nq, Mpad, V = (F + 3) // 4, (M + 15) // 16 * 16, 16
    S = 3 * nq
    tab = dealing(nq, Mpad)
    centres = rng.uniform(-1, 1, (M, 3)); radii = rng.uniform(0.5, 1.2, M)
    X = rng.uniform(-1.2, 1.2, (V, 3))
    W = rng.standard_normal((F, M + 4, 3)) * 0.3                  # fd_get_weights' layout per frame
    r = rng.standard_normal((F, V, 3))
    # the direct form: sum_f J_f^T r_f, J_f[c][k] = sum_j w_f[j][c] grad phi_j[k] + L_f[c][k]
    _, gphi = cases.phi_grad(kind, X.astype(cases.LD), centres.astype(cases.LD), radii)
    gphi = np.asarray(gphi, np.float64)                           # (V, M, 3)
    direct = np.zeros((V, 3))
    for f in range(F):
        w, L = W[f, :M], W[f, M + 1:].T                           # L[c][k] = W[M + 1 + k][c]
        J = np.einsum("jc,vjk->vck", w, gphi) + L[None]
        direct += np.einsum("vck,vc->vk", J, r[f])
    # the operands as the pack kernel and the launch's prologue deal them
    wq = tab["W"]
    assert wq.shape == (Mpad // 16 * S * 64, 4) and (wq[:, 0] == np.arange(len(wq))).all()
    A = np.zeros(len(wq))
    for q, centre, f, b in wq:
        if f < F and centre < M:
            A[q] = W[f, centre, b]
    aq = tab["A"]
    assert aq.shape == (S * 64, 4)
    Aff = np.zeros(len(aq))
    for q, dr, f, b in aq:
        if f < F and dr < 3:
            Aff[q] = W[f, M + 1 + dr, b]
    B = np.zeros((S, 4, V))
    seen = set()
    for f, b, step, k in tab["S"]:
        assert (step, k) not in seen and 0 <= step < S and 0 <= k < 4
        seen.add((step, k))
        if f < F:
            B[step, k] = r[f, :, b]
    assert len(seen) == 4 * S                                    # every depth slot of every step is dealt exactly once
    # one matrix instruction: D[row][v] += sum_k A[lane = row + 16 k] B[k][v]
    def product(tile):                                           # tile: (S, 64)
        D = np.zeros((16, V))
        for s in range(S):
            D += np.einsum("kr,kv->rv", tile[s].reshape(4, 16), B[s])
        return D
    A = A.reshape(Mpad // 16, S, 64)
    s = np.concatenate([product(A[t]) for t in range(Mpad // 16)])[:M]        # (M, V)
    want_s = np.einsum("fjb,fvb->jv", W[:, :M], r)
    assert np.abs(s - want_s).max() <= 1e-13 * np.abs(want_s).max()
    lt = product(Aff.reshape(S, 64))
    assert (lt[3:] == 0).all()
    via = np.einsum("vjk,jv->vk", gphi, s) + lt[:3].T
    scale = np.abs(np.einsum("vjk,jv->vk", np.abs(gphi), np.abs(s))).max()
    assert np.abs(via - direct).max() <= 1e-13 * scale
