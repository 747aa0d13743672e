"""CPU: the C ABI of fd_deform_adjoint* and fd_solve_operator -- the exported symbols, the contract in the header, and the
argument checks that answer before any device work (NULL context, NULL G, NULL grad_W, N < 0)."""
import ctypes as C
import os

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

FNS = ["fd_deform_adjoint", "fd_deform_adjoint_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_adjoint_symbols_exported(hip_lib):
    for name in FNS + ["fd_solve_operator"]:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_adjoint.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_adjoint.hip"))


def test_contract_is_in_the_header():
    text = _header()
    assert "sum_{j,a} grad_W[j][a] W'[j][a] = sum_v g_v . D_v(W')" in text
    assert "grad_W[j][a]     = sum_v phi_j(x_v) r_v[a],   r_v = f_v Pi_v g_v" in text
    assert "a select, not a product" in text
    assert "grad_delta = S^T . grad_W" in text
    for decl in ("int fd_deform_adjoint_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2,",
                 "int fd_deform_adjoint(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2,",
                 "int fd_solve_operator(fd_ctx *ctx, double *S);"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_adjoint", "deform_adjoint_dev", "solve_operator"):
        assert callable(getattr(capi.Engine, name))


@pytest.mark.parametrize("fn", FNS)
def test_null_context_is_invalid(hip_lib, fn):
    arr = (C.c_float * 3)()
    out = (C.c_double * 15)()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 1, arr, arr, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID
    assert hip_lib.fd_solve_operator(None, None) == capi.FD_E_INVALID
    assert hip_lib.fd_solve_operator(None, C.cast(out, C.POINTER(C.c_double))) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", FNS)
def test_null_arrays_are_invalid_before_device_work(hip_lib, fn):
    # fd_create needs a device, so a stand-in handle (as tests/test_invert_abi.py): the checks read only the arguments, never
    # the context's state, and set_err writes into the context's message buffer -- give it one the size of fd_ctx's
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    out = (C.c_double * 15)()
    assert call(ctx, 1, arr, None, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID       # NULL G
    assert call(ctx, 1, arr, arr, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID      # NULL grad_W
    assert call(ctx, -1, arr, arr, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID      # N < 0
    assert call(ctx, 0, None, None, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID     # NULL G, even with N = 0
    assert hip_lib.fd_solve_operator(ctx, None) == capi.FD_E_INVALID
