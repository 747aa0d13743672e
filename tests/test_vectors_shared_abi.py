"""CPU: the C ABI of fd_batch_deform_vectors_shared_dev -- fd_batch_vectors' layout, the exported symbols, the header's
rules, and the argument checks that answer before any device work (NULL batch, struct_size, half-given pairs, an output
that is a shared input)."""
import ctypes as C
import os
import re

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import capi


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_fd_batch_vectors_layout():
    # int struct_size, then seven pointers (N, N_out, tu, tu_out, tv, tv_out, jacobian) from offset 8
    assert C.sizeof(capi.FdBatchVectors) == 8 + 7 * 8
    names = [f[0] for f in capi.FdBatchVectors._fields_]
    assert names == ["struct_size", "N", "N_out", "tu", "tu_out", "tv", "tv_out", "jacobian"]
    assert capi.FdBatchVectors.N.offset == 8 and capi.FdBatchVectors.N_out.offset == 16
    assert capi.FdBatchVectors.jacobian.offset == 56
    body = re.search(r"typedef struct fd_batch_vectors \{(.*?)\} fd_batch_vectors;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*[;,]|int\s+(\w+)\s*;", body)
    assert [a or b for a, b in fields] == names


def test_symbols_exported(hip_lib):
    for name in ("fd_batch_deform_vectors_shared_dev", "fd_shared_vectors_kernel_name"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_kernel_name_query(hip_lib):
    # where fd_shared_kernel_name names a launch, the vector launch has one too; elsewhere both are ""
    for kind, name in ((capi.KERNEL_THIN_PLATE, "k_vectors32_shared_thin_plate"), (capi.KERNEL_GAUSSIAN, "k_vectors32_shared_gaussian"),
                       (capi.KERNEL_GAUSSIAN_QNN, "k_vectors32_shared_gaussian")):
        for M, F in ((32, 1), (96, 13), (256, 32)):
            assert capi.fd_shared_vectors_kernel_name(M, F, kind) == name
    assert capi.fd_shared_vectors_kernel_name(16, 4, capi.KERNEL_THIN_PLATE) == ""
    assert capi.fd_shared_vectors_kernel_name(256, 4, capi.KERNEL_BIHARMONIC) == ""
    assert capi.fd_shared_vectors_kernel_name(256, 4, capi.KERNEL_CUBIC) == ""


def test_header_states_the_rules():
    text = _header()
    decl = text[text.index("typedef struct fd_batch_vectors"):text.index("const char *fd_shared_vectors_kernel_name")]
    assert "t' = A_f t (not renormalised)" in decl
    assert "cof(A_f) n rescaled to |n|" in decl
    assert "bit for bit" in decl and "A = I exactly" in decl
    assert "must differ from every shared input" in decl and "FD_E_INVALID, before" in decl
    assert "bit-identical to fd_batch_deform_shared_dev" in decl
    assert "fd_batch_wait_consumed covers the vector launch" in decl


def _vec(**kw):
    v = capi.FdBatchVectors()
    v.struct_size = kw.pop("struct_size", C.sizeof(capi.FdBatchVectors))
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def test_null_batch_is_invalid(hip_lib):
    v = _vec()
    f = hip_lib.fd_batch_deform_vectors_shared_dev
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0, C.byref(v)) == capi.FD_E_INVALID
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a batch handle without a device: the checks run before any HIP call")
def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # fd_batch_create needs a device, so a stand-in handle: the checks read only the batch's size (its first int) and
    # write its message buffer -- give it one larger than fd_batch
    buf = (C.c_char * (1 << 16))()
    C.cast(buf, C.POINTER(C.c_int))[0] = 2
    b = C.cast(buf, C.c_void_p)
    f = hip_lib.fd_batch_deform_vectors_shared_dev
    mesh, vin = (C.c_float * 6)(), (C.c_float * 6)()
    o1, o2, o3, o4 = ((C.c_float * 6)() for _ in range(4))
    vp = C.c_void_p
    P_out = (vp * 2)(C.addressof(o1), C.addressof(o2))
    tab = lambda *a: (vp * 2)(*[C.addressof(x) if x is not None else None for x in a])

    def call(v, pout=P_out, fall=None):
        return f(b, None, 2, mesh, pout, None, fall, None, None, None, 1.0, 1.0, C.byref(v))

    for v in (_vec(struct_size=0), _vec(struct_size=C.sizeof(capi.FdBatchVectors) - 8, N=C.addressof(vin), N_out=tab(o3, o4)),
              _vec(N=C.addressof(vin)), _vec(N_out=tab(o3, o4)), _vec(tu=C.addressof(vin)), _vec(tv_out=tab(o3, o4)),
              _vec(N=C.addressof(vin), N_out=tab(o3, None)),                       # a table with a NULL entry
              _vec(N=C.addressof(vin), N_out=tab(o3, vin)),                        # output = the vector input
              _vec(N=C.addressof(vin), N_out=tab(mesh, o4)),                       # output = P_in
              _vec(tu=C.addressof(vin), tu_out=tab(o3, o4), jacobian=tab(o1, o4))):  # Jacobian over a P_out is fine, over P_in not:
        if v.jacobian:
            v.jacobian = tab(mesh, o4)
        assert call(v) == capi.FD_E_INVALID
    # P_out / falloff_out over a shared input, once vectors are asked for
    v = _vec(N=C.addressof(vin), N_out=tab(o3, o4))
    assert call(v, pout=tab(o1, mesh)) == capi.FD_E_INVALID
    assert call(v, fall=tab(vin, o2)) == capi.FD_E_INVALID
