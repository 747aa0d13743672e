"""CPU: the C ABI of fd_batch_deform_shared_fp64_dev -- the exported symbols, the kernel-name query, the header's rules,
and the argument checks that answer before any device work (NULL batch, NULL table entries, an output that is a shared
input)."""
import ctypes as C
import os

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import capi

KINDS = (capi.KERNEL_THIN_PLATE, capi.KERNEL_GAUSSIAN, capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_BIHARMONIC, capi.KERNEL_CUBIC)


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_symbols_exported(hip_lib):
    for name in ("fd_batch_deform_shared_fp64_dev", "fd_shared_fp64_kernel_name"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hasattr(capi.Batch, "deform_shared_fp64_dev")
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_kernel_name_query(hip_lib):
    for kind in KINDS:
        for M, F in ((32, 4), (96, 13), (256, 32), (2048, 32)):
            assert capi.fd_shared_fp64_kernel_name(M, F, kind) == "k_deform64_shared"
        assert capi.fd_shared_fp64_kernel_name(256, 1, kind) != ""       # no lower threshold on the frame count
    assert capi.fd_shared_fp64_kernel_name(256, 32, capi.KERNEL_GAUSSIAN_ML) == ""
    assert capi.fd_shared_fp64_kernel_name(256, 33, capi.KERNEL_THIN_PLATE) == ""
    assert capi.fd_shared_fp64_kernel_name(256, 0, capi.KERNEL_THIN_PLATE) == ""


def test_header_states_the_rules():
    text = _header()
    decl = text[text.index("The frames of a shot evaluated in fp64 by ONE matrix-pipe launch"):text.index("const char *fd_shared_fp64_kernel_name")]
    assert "in fp64 whatever fd_set_eval_precision says" in decl and "settings are not changed" in decl
    assert "ONE rounding of the three sums to fp32" in decl
    assert "within one fp32 ulp" in decl and "bit-identical" in decl
    assert "is passed through" in decl and "terminationtype != 1" in decl and "fd_falloff entry is not written" in decl
    assert "Entries past N are not touched" in decl
    assert "no output (P_out, falloff_out) may be a shared input" in decl and "FD_E_INVALID, before any device work" in decl
    assert "P_out[0] == d_P_in is allowed" in decl
    assert "fd_batch_wait_consumed covers this launch" in decl
    assert "fd_batch_cook_group, fdsop_cook and fd_batch_deform_vectors_shared_dev do not take this launch" in decl
    assert "int fd_batch_deform_shared_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in," in decl
    assert "#define FD_ABI_VERSION 9" in text


def test_null_batch_is_invalid(hip_lib):
    f = hip_lib.fd_batch_deform_shared_fp64_dev
    out = (C.c_float * 6)()
    tab = (C.c_void_p * 1)(C.addressof(out))
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID
    assert f(None, None, 2, out, tab, None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a batch handle without a device: the checks run before any HIP call")
def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # fd_batch_create needs a device, so a stand-in handle: the checks read only the batch's size (its first int) and
    # write its message buffer -- give it one larger than fd_batch
    def handle(n):
        buf = (C.c_char * (1 << 16))()
        C.cast(buf, C.POINTER(C.c_int))[0] = n
        return buf, C.cast(buf, C.c_void_p)

    f = hip_lib.fd_batch_deform_shared_fp64_dev
    mesh, d2, tu, tv, nr = ((C.c_float * 6)() for _ in range(5))
    o1, o2, f1, f2 = ((C.c_float * 6)() for _ in range(4))
    vp = C.c_void_p
    tab = lambda *a: (vp * len(a))(*[C.addressof(x) if x is not None else None for x in a])
    keep, b = handle(2)

    def call(pout, fall=None, h=b, frames=True, N=2):
        return f(h, None, N, mesh, pout, d2, fall, tu if frames else None, tv if frames else None, nr if frames else None, 1.0, 1.0)

    assert call(None) == capi.FD_E_INVALID                             # no output table
    assert call(tab(o1, None)) == capi.FD_E_INVALID                    # a table with a NULL entry
    assert f(b, None, 2, None, tab(o1, o2), None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID     # N > 0 without a mesh
    assert f(b, None, -1, mesh, tab(o1, o2), None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID
    assert f(b, None, 2, mesh, tab(o1, o2), None, None, tu, None, None, 1.0, 1.0) == capi.FD_E_INVALID       # half-given frames
    for shared in (mesh, d2, tu, tv, nr):
        assert call(tab(o1, shared)) == capi.FD_E_INVALID              # P_out over a shared input
        assert call(tab(shared, o2)) == capi.FD_E_INVALID
        assert call(tab(o1, o2), fall=tab(f1, shared)) == capi.FD_E_INVALID     # fd_falloff over a shared input
    assert b"shared input" in hip_lib.fd_batch_last_error(b)
    # (N = 0 with clean arguments is answered FD_OK, still before any device work)
    assert call(tab(o1, o2), fall=tab(f1, f2), N=0) == capi.FD_OK
    # one frame: P_out[0] == P_in is the one alias allowed (answered here with N = 0: nothing to launch) ...
    keep1, b1 = handle(1)
    assert call(tab(mesh), h=b1, N=0) == capi.FD_OK
    # ... every other one is not
    for shared in (d2, tu, tv, nr):
        assert call(tab(shared), h=b1, N=0) == capi.FD_E_INVALID
    assert call(tab(o1), fall=tab(mesh), h=b1, N=0) == capi.FD_E_INVALID
    assert call(tab(o1), fall=tab(d2), h=b1, N=0) == capi.FD_E_INVALID
