"""CPU: the C ABI of fd_batch_deform_shared_ml_fp64_dev -- the exported symbols, the kernel-name query, the header's
contract, and the argument checks that answer before any device work (NULL batch, NULL table entries, half-given tangent
frames, an output that is a shared input)."""
import ctypes as C
import os

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import capi

NAME = "k_deform64_shared_ml"


def threshold():
    """The smallest frame count the launch takes (the name query is its statement)."""
    return next(F for F in range(1, 33) if capi.fd_shared_ml_fp64_kernel_name(64, 4, F) != "")


def test_symbols_exported(hip_lib):
    for name in ("fd_batch_deform_shared_ml_fp64_dev", "fd_shared_ml_fp64_kernel_name"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hasattr(capi.Batch, "deform_shared_ml_fp64_dev")
    assert callable(capi.fd_shared_ml_fp64_kernel_name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_kernel_name_query(hip_lib):
    for M, L, F in ((33, 8, 5), (256, 4, 32), (700, 3, 20)):
        assert capi.fd_shared_ml_fp64_kernel_name(M, L, F) == NAME
    assert capi.fd_shared_ml_fp64_kernel_name(256, 0, 32) == ""
    assert capi.fd_shared_ml_fp64_kernel_name(256, 9, 32) == ""
    assert capi.fd_shared_ml_fp64_kernel_name(256, 4, 0) == ""
    assert capi.fd_shared_ml_fp64_kernel_name(256, 4, 33) == ""
    assert capi.fd_shared_ml_fp64_kernel_name(0, 4, 32) == ""
    assert capi.fd_shared_ml_fp64_kernel_name(-5, 4, 32) == ""
    # monotone in F around the threshold, the same threshold in both layer columns
    t = threshold()
    assert 1 <= t <= 32
    for F in range(1, 33):
        assert capi.fd_shared_ml_fp64_kernel_name(256, 4, F) == (NAME if F >= t else "")
        assert capi.fd_shared_ml_fp64_kernel_name(256, 8, F) == (NAME if F >= t else "")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    decl = text[text.index("The frames of a shot of MULTILAYER models evaluated in FP64"):text.index("const char *fd_shared_ml_fp64_kernel_name")]
    assert "int fd_batch_deform_shared_ml_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in," in decl
    assert "bit for bit" in decl and "fd_batch_wait_consumed covers this launch" in decl
    assert "Entries past N are not touched" in decl and "FD_E_INVALID" in decl and "Not covered" in decl
    assert "(96 + M L) 2^-53 S_f" in decl and "AT l = 4 THE CHAIN RESTARTS" in decl
    assert "const char *fd_shared_ml_fp64_kernel_name(int M, int layers, int frames);" in text
    assert "#define FD_ABI_VERSION 9" in text


def test_null_batch_is_invalid(hip_lib):
    f = hip_lib.fd_batch_deform_shared_ml_fp64_dev
    out = (C.c_float * 6)()
    tab = (C.c_void_p * 1)(C.addressof(out))
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID
    assert f(None, None, 2, out, tab, None, None, None, None, None, 1.0, 1.0) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a batch handle without a device: the checks run before any HIP call")
def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # fd_batch_create needs a device, so a stand-in handle (tests/test_shared_fp64_abi.py): the checks read only the batch's
    # size (its first int) and write its message buffer -- give it one larger than fd_batch
    def handle(n):
        buf = (C.c_char * (1 << 16))()
        C.cast(buf, C.POINTER(C.c_int))[0] = n
        return buf, C.cast(buf, C.c_void_p)

    f = hip_lib.fd_batch_deform_shared_ml_fp64_dev
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
    assert f(b, None, 2, mesh, tab(o1, o2), None, None, tu, tv, None, 1.0, 1.0) == capi.FD_E_INVALID
    for shared in (mesh, d2, tu, tv, nr):
        assert call(tab(o1, shared)) == capi.FD_E_INVALID              # P_out over a shared input
        assert call(tab(shared, o2)) == capi.FD_E_INVALID
        assert call(tab(o1, o2), fall=tab(f1, shared)) == capi.FD_E_INVALID     # fd_falloff over a shared input
        assert call(tab(o1, o2), fall=tab(shared, f2)) == capi.FD_E_INVALID
    assert b"shared input" in hip_lib.fd_batch_last_error(b)
    # N = 0 with clean arguments is answered FD_OK, still before any device work
    assert call(tab(o1, o2), fall=tab(f1, f2), N=0) == capi.FD_OK
    # one frame: P_out[0] == P_in is the one alias allowed (answered here with N = 0: nothing to launch) ...
    keep1, b1 = handle(1)
    assert call(tab(mesh), h=b1, N=0) == capi.FD_OK
    # ... every other one is not
    for shared in (d2, tu, tv, nr):
        assert call(tab(shared), h=b1, N=0) == capi.FD_E_INVALID
    assert call(tab(o1), fall=tab(mesh), h=b1, N=0) == capi.FD_E_INVALID
    assert call(tab(o1), fall=tab(d2), h=b1, N=0) == capi.FD_E_INVALID
