"""CPU: the C ABI of fd_deform_adjoint_shot* and fd_fit_deltas_shot -- the exported symbols, the contract in the header, the
Engine methods, and the argument checks that answer before any device work (NULL context, NULL G / grad_W / T / delta_out,
N < 0, F = 0, mu < 0 or NaN, a report too small anywhere in the array)."""
import ctypes as C
import os

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

SHOT_FNS = ["fd_deform_adjoint_shot", "fd_deform_adjoint_shot_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_shot_symbols_exported(hip_lib):
    for name in SHOT_FNS + ["fd_fit_deltas_shot"]:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_adjoint_shot.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_adjoint_shot.hip"))


def test_contract_is_in_the_header():
    text = _header()
    assert "the adjoint and the fit for the frames of a shot" in text
    assert "grad_W[f] = Psi^T R_f,   r_{f,v} = f_v Pi_v g_{f,v}" in text
    assert "sum_{j,a} grad_W[f][j][a] W'[j][a] = sum_v g_{f,v} . D_v(W')" in text
    assert "G is F x N x 3 fp32, frame-major" in text
    assert "grad_W is F x (C+4) x 3" in text
    assert "is a function of N and C alone, not of F" in text
    assert "differ in the order of additions and are not bit-equal to each other" in text
    assert "reaches frame f's block only" in text
    assert "On FD_E_SINGULAR nothing is written to delta_out" in text
    for decl in ("int fd_deform_adjoint_shot_dev(fd_ctx *ctx, int64_t N, int F, const float *d_P_in, const float *d_G, const float *d_dist2,",
                 "int fd_deform_adjoint_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *G, const float *dist2,",
                 "int fd_fit_deltas_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *T, const float *omega,"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_adjoint_shot", "deform_adjoint_shot_dev", "fit_deltas_shot"):
        assert callable(getattr(capi.Engine, name))


def _adj(lib, fn, ctx, N, F, P, G, out):
    return getattr(lib, fn)(ctx, N, F, P, G, None, None, None, None, 1.0, 1.0, out)


def _fit(lib, ctx, N, F, P, T, out, mu=0.0, reports=None):
    return lib.fd_fit_deltas_shot(ctx, N, F, P, T, None, None, None, None, None, 1.0, 1.0, mu, None, None, out, reports)


def test_null_context_is_invalid(hip_lib):
    arr = (C.c_float * 9)()
    out = (C.c_double * 64)()
    for fn in SHOT_FNS:
        assert _adj(hip_lib, fn, None, 0, 1, None, None, None) == capi.FD_E_INVALID
        assert _adj(hip_lib, fn, None, 1, 2, arr, arr, out) == capi.FD_E_INVALID
    assert _fit(hip_lib, None, 0, 1, None, None, None) == capi.FD_E_INVALID
    assert _fit(hip_lib, None, 1, 2, arr, arr, out) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # a stand-in handle (as tests/test_gram_abi.py): the checks read only the arguments and set_err writes into the context's
    # message buffer -- give it one the size of fd_ctx's.  Zeroed, it is a context with no points and no model.
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    arr = (C.c_float * 9)()
    out = (C.c_double * 64)()
    for fn in SHOT_FNS:
        assert _adj(hip_lib, fn, ctx, 1, 2, arr, None, out) == capi.FD_E_INVALID         # NULL G
        assert _adj(hip_lib, fn, ctx, 1, 2, arr, arr, None) == capi.FD_E_INVALID         # NULL grad_W
        assert _adj(hip_lib, fn, ctx, 0, 2, None, None, None) == capi.FD_E_INVALID       # both, even with N = 0
        assert _adj(hip_lib, fn, ctx, -1, 2, arr, arr, out) == capi.FD_E_INVALID         # N < 0
        assert _adj(hip_lib, fn, ctx, 1, 0, arr, arr, out) == capi.FD_E_INVALID          # F = 0
        assert _adj(hip_lib, fn, ctx, 1, -3, arr, arr, out) == capi.FD_E_INVALID
        # everything in order as far as the arguments go: the next check is the model's
        assert _adj(hip_lib, fn, ctx, 1, 2, arr, arr, out) == capi.FD_E_NOT_BUILT
    assert _fit(hip_lib, ctx, 1, 2, arr, None, out) == capi.FD_E_INVALID                 # NULL T
    assert _fit(hip_lib, ctx, 1, 2, arr, arr, None) == capi.FD_E_INVALID                 # NULL delta_out
    assert _fit(hip_lib, ctx, -1, 2, arr, arr, out) == capi.FD_E_INVALID                 # N < 0
    assert _fit(hip_lib, ctx, 1, 2, None, arr, out) == capi.FD_E_INVALID                 # NULL P with N > 0
    assert _fit(hip_lib, ctx, 1, 0, arr, arr, out) == capi.FD_E_INVALID                  # F = 0
    assert _fit(hip_lib, ctx, 1, 2, arr, arr, out, mu=-1e-9) == capi.FD_E_INVALID        # mu < 0
    assert _fit(hip_lib, ctx, 1, 2, arr, arr, out, mu=float("nan")) == capi.FD_E_INVALID
    size = C.sizeof(capi.FdFitReport)
    for bad in (0, 1, 2):                                                                # a short struct_size anywhere, the last entry included
        reps = (capi.FdFitReport * 3)()
        for k, r in enumerate(reps):
            r.struct_size = size - 1 if k == bad else size
        assert _fit(hip_lib, ctx, 1, 3, arr, arr, out, reports=reps) == capi.FD_E_INVALID
    reps = (capi.FdFitReport * 3)()
    for r in reps:
        r.struct_size = size
    assert _fit(hip_lib, ctx, 1, 3, arr, arr, out, reports=reps) == capi.FD_E_NOT_BUILT
