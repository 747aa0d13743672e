"""CPU: the C ABI of fd_deform_vectors* -- fd_vectors' layout, the exported symbols, and the argument checks that
answer before any device work (NULL context, struct_size, a vector without its output)."""
import ctypes as C
import os
import re

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import capi


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_fd_vectors_layout():
    # int struct_size, then seven pointers (N, N_out, tu, tu_out, tv, tv_out, jacobian) from offset 8
    assert C.sizeof(capi.FdVectors) == 8 + 7 * 8
    names = [f[0] for f in capi.FdVectors._fields_]
    assert names == ["struct_size", "N", "N_out", "tu", "tu_out", "tv", "tv_out", "jacobian"]
    assert capi.FdVectors.N.offset == 8 and capi.FdVectors.jacobian.offset == 56
    body = re.search(r"typedef struct fd_vectors \{(.*?)\} fd_vectors;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*[;,]|int\s+(\w+)\s*;", body)
    assert [a or b for a, b in fields] == names


def test_vectors_symbols_exported(hip_lib):
    for name in ("fd_deform_vectors", "fd_deform_vectors_dev"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_definition_is_in_the_header():
    text = _header()
    assert "A = I + f . Pi . J(x)" in text
    assert "cof(A)(u x v) = (A u) x (A v)" in text


def _vec(**kw):
    v = capi.FdVectors()
    v.struct_size = kw.pop("struct_size", C.sizeof(capi.FdVectors))
    for k, val in kw.items():
        setattr(v, k, val)
    return v


@pytest.mark.parametrize("fn", ["fd_deform_vectors", "fd_deform_vectors_dev"])
def test_null_context_is_invalid(hip_lib, fn):
    v = _vec()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, None, 1.0, 1.0, C.byref(v)) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", ["fd_deform_vectors", "fd_deform_vectors_dev"])
def test_bad_struct_is_invalid_before_device_work(hip_lib, fn):
    # fd_create needs a device, so a stand-in handle: the checks read only the struct, never the context's state,
    # and set_err on an invalid struct writes into the context's message buffer -- give it one the size of fd_ctx's
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    for v in (_vec(struct_size=0), _vec(struct_size=C.sizeof(capi.FdVectors) - 8),
              _vec(N=C.addressof(arr)), _vec(tu_out=C.addressof(arr)), _vec(tv=C.addressof(arr))):
        assert call(ctx, 1, arr, arr, None, None, None, None, None, 1.0, 1.0, C.byref(v)) == capi.FD_E_INVALID
