"""CPU: the C ABI of the multilayer case of fd_batch_set_shared_factor -- one factorisation per layer for a shot of
multilayer models (facedeform_amd/csrc/fd_build_ml_shared.hip): the exported symbols, the kernel-name
query and what the header promises."""
import os

from conftest import ROOT
from facedeform_amd import capi

NAME = "k_ml_solve_shared"


def threshold():
    """The smallest frame count the shared build takes (the name query is its statement)."""
    return next(F for F in range(1, 33) if capi.fd_shared_ml_build_kernel_name(256, 4, F) != "")


def test_symbols_exported(hip_lib):
    for name in ("fd_shared_ml_build_kernel_name", "fd_batch_set_shared_factor", "fd_batch_last_build_shared_factor"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hasattr(capi, "fd_shared_ml_build_kernel_name")
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_kernel_name_query(hip_lib):
    for M, L, F in ((33, 8, 5), (256, 4, 32), (1024, 2, 2)):
        assert capi.fd_shared_ml_build_kernel_name(M, L, F) == NAME
    for L in (0, 9, -1):
        assert capi.fd_shared_ml_build_kernel_name(256, L, 32) == ""
    for F in (-3, 0, 1, 33):
        assert capi.fd_shared_ml_build_kernel_name(256, 4, F) == ""
    for M in (0, -5, 1025, 5000):
        assert capi.fd_shared_ml_build_kernel_name(M, 4, 32) == ""
    t = threshold()
    assert 2 <= t <= 32
    for F in range(1, 33):
        for M, L in ((256, 4), (256, 8), (700, 3), (1024, 1)):
            assert capi.fd_shared_ml_build_kernel_name(M, L, F) == (NAME if F >= t else "")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    decl = text[text.index("One factorisation per batched build where the contexts share the rest rig"):
                text.index("int fd_batch_set_shared_factor(fd_batch *batch, int on);")]
    # what "the factor" is for the multilayer model
    assert "FD_KERNEL_GAUSSIAN_ML" in decl and "L factors, one per layer" in decl
    # the conditions
    assert "same (R, layers, lambda)" in decl and "SAME rest array" in decl and "at least two contexts" in decl and "M <= 1024" in decl
    # the delegation, and how close the results are
    assert "Delegation" in decl and "exactly as without the switch, bit for bit" in decl
    assert "to rounding, not bit for bit" in decl
    assert "FD_E_NOT_BUILT" in decl and "k_ml_solve_shared" in decl
    assert "const char *fd_shared_ml_build_kernel_name(int M, int layers, int frames);" in text
    assert "#define FD_ABI_VERSION 9" in text


def test_source_is_built(hip_lib):
    from facedeform_amd import _build
    assert "fd_build_ml_shared.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_build_ml_shared.hip"))
