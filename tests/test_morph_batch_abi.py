"""CPU: the C ABI of the batched morph-space passes (fd_morph_compute_weights_batch_dev, fd_morph_displace_batch_dev,
fd_morph_get_weights_batch) -- the exported symbols, the header's rules, and the argument checks that answer before any
device work (NULL object, F outside 1..FD_MAX_BATCH, a NULL table or entry, two frames writing one array)."""
import ctypes as C
import os

from conftest import ROOT
from facedeform_amd import capi

NAMES = ("fd_morph_compute_weights_batch_dev", "fd_morph_displace_batch_dev", "fd_morph_get_weights_batch")
FD_MAX_BATCH = 32


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    for name in ("compute_weights_batch_dev", "displace_batch_dev", "weights_batch"):
        assert callable(getattr(capi.Morph, name))


def test_header_states_the_rules():
    text = _header()
    assert "#define FD_MAX_BATCH %d" % FD_MAX_BATCH in text
    decl = text[text.index("The F = 1..FD_MAX_BATCH frames of one shot"):text.index("int fd_morph_get_weights_batch(")]
    for ref in ("dbse.cpp:39-60", "SOP_FaceDeform.cpp:458-473", "dbse.cpp:62-77"):
        assert ref in decl
    assert "once per call instead of once per frame" in decl
    assert "not bit for bit" in decl and "no floating-point atomics" in decl
    assert "bit-identical to the one-frame call" in decl
    assert "neither read nor" in decl and "fd_morph_init* clears them" in decl
    assert "FD_E_NOT_BUILT" in decl and "FD_E_INVALID before any device work" in decl
    assert "Two equal entries" in decl and "Entries of the table may repeat" in decl
    assert "entries past N are not touched" in decl


def test_null_object_is_invalid(hip_lib):
    a = (C.c_float * 6)()
    tab = (C.c_void_p * 1)(C.addressof(a))
    w = (C.c_double * 4)()
    assert hip_lib.fd_morph_compute_weights_batch_dev(None, 1, tab, None) == capi.FD_E_INVALID
    assert b"fd_morph_compute_weights_batch_dev" in hip_lib.fd_morph_last_error(None)
    assert hip_lib.fd_morph_displace_batch_dev(None, 1, tab, None, 0, 0.0, None) == capi.FD_E_INVALID
    assert b"fd_morph_displace_batch_dev" in hip_lib.fd_morph_last_error(None)
    assert hip_lib.fd_morph_get_weights_batch(None, 1, w) == capi.FD_E_INVALID
    assert b"fd_morph_get_weights_batch" in hip_lib.fd_morph_last_error(None)


def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # fd_morph_create needs a device, so a stand-in object: the argument checks read nothing of it and write only its
    # message buffer -- give it one larger than fd_morph.  Every call below must answer before it looks further.
    buf = (C.c_char * (1 << 16))()
    m = C.cast(buf, C.c_void_p)
    arrays = [(C.c_float * 6)() for _ in range(FD_MAX_BATCH + 1)]
    vp = C.c_void_p

    def tab(*idx):
        return (vp * max(1, len(idx)))(*[None if i is None else C.addressof(arrays[i]) for i in idx])

    compute = lambda F, t: hip_lib.fd_morph_compute_weights_batch_dev(m, F, t, None)
    displace = lambda F, t: hip_lib.fd_morph_displace_batch_dev(m, F, t, None, 0, 0.0, None)
    msg = lambda: hip_lib.fd_morph_last_error(m).decode()
    full = tab(*range(FD_MAX_BATCH + 1))
    for call in (compute, displace):
        for F in (0, -1, FD_MAX_BATCH + 1):
            assert call(F, full) == capi.FD_E_INVALID and "need 1..32 frames" in msg()
        assert call(2, None) == capi.FD_E_INVALID and "table" in msg()
        assert call(3, tab(0, None, 2)) == capi.FD_E_INVALID and "frame 1 is NULL" in msg()
        assert call(1, tab(None)) == capi.FD_E_INVALID
    # two frames writing one array; (the read-only weights call takes such a table: GPU tests)
    assert displace(3, tab(0, 1, 0)) == capi.FD_E_INVALID and "frames 0 and 2 are the same array" in msg()
    assert displace(FD_MAX_BATCH, tab(*(list(range(FD_MAX_BATCH - 1)) + [5]))) == capi.FD_E_INVALID
    w = (C.c_double * 4)()
    for F in (0, FD_MAX_BATCH + 1):
        assert hip_lib.fd_morph_get_weights_batch(m, F, w) == capi.FD_E_INVALID
    assert hip_lib.fd_morph_get_weights_batch(m, 1, None) == capi.FD_E_INVALID
