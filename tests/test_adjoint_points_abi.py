"""CPU: the C ABI of fd_deform_adjoint_points* -- the exported symbols, fd_adjoint_points_opts' layout, the contract in the
header, and the argument checks that answer before any device work (NULL context, NULL G, NULL grad_P, N < 0, struct_size)."""
import ctypes as C
import os
import re

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

FNS = ["fd_deform_adjoint_points", "fd_deform_adjoint_points_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def _opts(struct_size=None, grad_f=None):
    o = capi.FdAdjointPointsOpts()
    o.struct_size = C.sizeof(capi.FdAdjointPointsOpts) if struct_size is None else struct_size
    o.grad_f = grad_f
    return o


def test_symbols_exported(hip_lib):
    for name in FNS:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_adjoint_points.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_adjoint_points.hip"))


def test_opts_layout():
    # int struct_size, int reserved, then one pointer
    assert C.sizeof(capi.FdAdjointPointsOpts) == 16
    names = [f[0] for f in capi.FdAdjointPointsOpts._fields_]
    assert names == ["struct_size", "reserved", "grad_f"]
    assert [getattr(capi.FdAdjointPointsOpts, n).offset for n in names] == [0, 4, 8]
    body = re.search(r"typedef struct fd_adjoint_points_opts \{(.*?)\} fd_adjoint_points_opts;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|double|float)\s*(\*?)\s*(\w+)\s*;", body)
    assert [(f[0], f[1], f[2]) for f in fields] == [("int", "", "struct_size"), ("int", "", "reserved"), ("double", "*", "grad_f")]


def test_contract_is_in_the_header():
    text = _header()
    assert "sum_v grad_P[v] . t_v = sum_v g_v . (A_v t_v)" in text
    assert "grad_P[v] = A_v^T g_v = g_v + J(x_v)^T r_v" in text
    assert "grad_f[v] = g_v . Pi_v d(x_v)" in text
    for decl in ("typedef struct fd_adjoint_points_opts {",
                 "int fd_deform_adjoint_points_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2,",
                 "int fd_deform_adjoint_points(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2,"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_adjoint_points", "deform_adjoint_points_dev"):
        assert callable(getattr(capi.Engine, name))


@pytest.mark.parametrize("fn", FNS)
def test_null_context_is_invalid(hip_lib, fn):
    arr = (C.c_float * 3)()
    out = (C.c_double * 3)()
    o = _opts()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, 1.0, 1.0, None, None) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 1, arr, arr, None, None, None, None, 1.0, 1.0, out, C.byref(o)) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_invalid_before_device_work(hip_lib, fn):
    # fd_create needs a device, so a stand-in handle (as tests/test_adjoint_abi.py): the checks read only the arguments, never
    # the context's state, and set_err writes into the context's message buffer -- give it one the size of fd_ctx's
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    out = (C.c_double * 3)()
    assert call(ctx, 1, arr, None, None, None, None, None, 1.0, 1.0, out, None) == capi.FD_E_INVALID       # NULL G
    assert call(ctx, 1, arr, arr, None, None, None, None, 1.0, 1.0, None, None) == capi.FD_E_INVALID      # NULL grad_P
    assert call(ctx, -1, arr, arr, None, None, None, None, 1.0, 1.0, out, None) == capi.FD_E_INVALID      # N < 0
    assert call(ctx, 0, None, None, None, None, None, None, 1.0, 1.0, out, None) == capi.FD_E_INVALID     # NULL G, even with N = 0
    o = _opts(struct_size=8)
    assert call(ctx, 1, arr, arr, None, None, None, None, 1.0, 1.0, out, C.byref(o)) == capi.FD_E_INVALID  # opts too small
