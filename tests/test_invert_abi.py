"""CPU: the C ABI of fd_invert* -- fd_invert_opts' layout, the exported symbols, and the argument checks that answer
before any device work (NULL context, struct_size, NULL opts)."""
import ctypes as C
import os
import re

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

FNS = ["fd_invert", "fd_invert_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_fd_invert_opts_layout():
    # int struct_size, int max_iter, double tol, then two pointers
    assert C.sizeof(capi.FdInvertOpts) == 8 + 8 + 2 * 8
    names = [f[0] for f in capi.FdInvertOpts._fields_]
    assert names == ["struct_size", "max_iter", "tol", "residual_out", "iters_out"]
    offs = [getattr(capi.FdInvertOpts, n).offset for n in names]
    assert offs == [0, 4, 8, 16, 24]
    body = re.search(r"typedef struct fd_invert_opts \{(.*?)\} fd_invert_opts;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|double|float)\s*(\*?)\s*(\w+)\s*;", body)
    assert [f[2] for f in fields] == names
    assert [(f[0], f[1]) for f in fields] == [("int", ""), ("int", ""), ("double", ""), ("float", "*"), ("int", "*")]


def test_invert_symbols_exported(hip_lib):
    for name in FNS:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_invert.hip" in _build.SOURCES


def test_contract_is_in_the_header():
    text = _header()
    assert "x + f . Pi . d(x) = y" in text
    assert "-2 broke down" in text


def _opts(**kw):
    o = capi.FdInvertOpts()
    o.struct_size = kw.pop("struct_size", C.sizeof(capi.FdInvertOpts))
    for k, val in kw.items():
        setattr(o, k, val)
    return o


@pytest.mark.parametrize("fn", FNS)
def test_null_context_is_invalid(hip_lib, fn):
    o = _opts()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, 1.0, 1.0, C.byref(o)) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", FNS)
def test_bad_opts_are_invalid_before_device_work(hip_lib, fn):
    # fd_create needs a device, so a stand-in handle (as tests/test_vectors_abi.py): the checks read only the struct, never
    # the context's state, and set_err writes into the context's message buffer -- give it one the size of fd_ctx's
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    for o in (_opts(struct_size=0), _opts(struct_size=C.sizeof(capi.FdInvertOpts) - 8)):
        assert call(ctx, 1, arr, arr, None, None, None, None, 1.0, 1.0, C.byref(o)) == capi.FD_E_INVALID
    assert call(ctx, 1, arr, arr, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID
