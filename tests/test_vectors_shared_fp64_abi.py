"""CPU: the C ABI of fd_batch_deform_vectors_shared_fp64_dev -- the exported symbols, the header's contract, the Python
binding and the kernel-name query."""
import os

from conftest import ROOT
from facedeform_amd import capi

KINDS = (capi.KERNEL_THIN_PLATE, capi.KERNEL_GAUSSIAN, capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_BIHARMONIC, capi.KERNEL_CUBIC)
NAMES = ("fd_batch_deform_vectors_shared_fp64_dev", "fd_shared_vectors_fp64_kernel_name")


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_header_declares_them_and_states_the_contract():
    text = _header()
    assert "#define FD_ABI_VERSION 9" in text
    assert "int fd_batch_deform_vectors_shared_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in," in text
    assert "const char *fd_shared_vectors_fp64_kernel_name(int M, int frames, int kind);" in text
    decl = text[text.index("fd_batch_deform_shared_fp64_dev plus, for every frame f"):text.index("const char *fd_shared_vectors_fp64_kernel_name")]
    assert "bit-identical to fd_batch_deform_shared_fp64_dev called with the same arguments" in decl
    assert "is exactly fd_batch_deform_shared_fp64_dev" in decl
    assert "A_f = I + f Pi J_f" in decl and "not renormalised" in decl and "rescaled to |n|" in decl and "A is stored as fp32" in decl
    assert "A = I exactly" in decl and "Entries past N are not touched" in decl
    assert "FD_E_INVALID, before any device work" in decl and "a batch of one as well" in decl
    assert "both or neither" in decl and "n non-NULL entries" in decl
    assert "The multilayer model and an eval_variant override do not take it" in decl
    assert "fewer than 2 frames (thin-plate, biharmonic) or 3 (the Gaussian kinds, cubic)" in decl
    assert "fd_batch_wait_consumed covers it" in decl
    assert "no floating-point atomics" in decl
    assert "fd_batch_deform_vectors_shared_dev is unchanged" in decl


def test_python_binding():
    assert hasattr(capi.Batch, "deform_vectors_shared_fp64_dev")
    assert callable(capi.fd_shared_vectors_fp64_kernel_name)


# the fewest frames at which the one launch is taken (include/facedeform_hip.h, DESIGN.md 4.7c: below it the per-context
# launches measured faster)
MIN_FRAMES = {capi.KERNEL_THIN_PLATE: 2, capi.KERNEL_GAUSSIAN: 3, capi.KERNEL_GAUSSIAN_QNN: 3, capi.KERNEL_BIHARMONIC: 2, capi.KERNEL_CUBIC: 3}


def test_kernel_name_query(hip_lib):
    for kind in KINDS:
        for M in (1, 32, 96, 256, 2048):
            for F in range(1, 33):
                want = "k_vectors64_shared" if F >= MIN_FRAMES[kind] else ""
                assert capi.fd_shared_vectors_fp64_kernel_name(M, F, kind) == want, (kind, M, F)
        for M, F in ((0, 4), (-3, 4), (256, 0), (256, -1), (256, 33)):
            assert capi.fd_shared_vectors_fp64_kernel_name(M, F, kind) == ""
    for M, F in ((32, 1), (256, 32)):
        assert capi.fd_shared_vectors_fp64_kernel_name(M, F, capi.KERNEL_GAUSSIAN_ML) == ""


def test_null_batch_is_invalid(hip_lib):
    f = hip_lib.fd_batch_deform_vectors_shared_fp64_dev
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID
