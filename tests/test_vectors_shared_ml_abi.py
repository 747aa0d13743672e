"""CPU: the C ABI of fd_batch_deform_vectors_shared_ml_dev -- the exported symbols, the header's contract, the Python
binding and the kernel-name query."""
import os

from conftest import ROOT
from facedeform_amd import capi

NAME = "k_vectors32_shared_ml"
NAMES = ("fd_batch_deform_vectors_shared_ml_dev", "fd_shared_vectors_ml_kernel_name")
# the fewest frames at which the one launch is taken, per layer count (include/facedeform_hip.h): copied from
# profiles/vectors_shared_ml_1M_256_events.csv and ..._small_frames.csv, not read from the library.  At two frames the launch
# is ahead of the per-context launches with 2 to 8 layers (1.05x to 1.13x) and ties with one (0.2950 / 0.2951 ms; 1.33x at three)
MIN_FRAMES = {L: 3 if L == 1 else 2 for L in range(1, 9)}
FD_MAX_BATCH = 32


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
    assert "int fd_batch_deform_vectors_shared_ml_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in," in text
    assert "const char *fd_shared_vectors_ml_kernel_name(int M, int layers, int frames);" in text
    decl = text[text.index("fd_batch_deform_shared_ml_dev plus, for every frame f"):text.index("const char *fd_shared_vectors_ml_kernel_name")]
    # positions bit-identical
    assert "bit-identical to fd_batch_deform_shared_ml_dev called with the same arguments" in decl
    assert "is exactly fd_batch_deform_shared_ml_dev" in decl
    assert "A_f = I + f Pi J_f" in decl and "not renormalised" in decl and "rescaled to |n|" in decl and "A is stored as fp32" in decl
    assert "never E_{l+1} = E_l^4" in decl and "2^-22 ||A_ref||_F + 2^-21 f S'_f(x)" in decl
    # pass-through
    assert "A = I exactly" in decl and "Entries past N are not touched" in decl
    # aliasing and tables
    assert "FD_E_INVALID, before any device work" in decl and "a batch of one as well" in decl
    assert "both or neither" in decl and "n non-NULL entries" in decl
    # delegation
    assert "IS fd_batch_deform_vectors_shared_dev with the same arguments, bit for bit" in decl
    assert "what\n *     fd_deform_vectors_dev writes for an FD_EVAL_FP32 context" in decl
    # the radius limit
    assert "FINEST-layer radius R' / 2^(L - 1) of at least 0.00245 rig radii" in decl and "A is not finite" in decl
    assert "fd_batch_wait_consumed covers it" in decl
    # the threshold of the header is the one the name query answers by
    assert "measured threshold: 3 frames with one layer, 2 frames with\n *     2 to 8 layers" in decl
    assert "no floating-point atomics" in decl and "fd_batch_set_eval_cus" in decl
    assert "The seven other shared calls, fd_batch_cook_group and fdsop_cook are unchanged" in decl
    # the position call points at this one
    pos = text[text.index("The frames of a shot of MULTILAYER models (FD_KERNEL_GAUSSIAN_ML)"):text.index("const char *fd_shared_ml_kernel_name")]
    assert "fd_batch_deform_vectors_shared_ml_dev (below)" in pos and "stay\n *     with the per-context launches" not in pos


def test_python_binding():
    assert hasattr(capi.Batch, "deform_vectors_shared_ml_dev")
    assert callable(capi.fd_shared_vectors_ml_kernel_name)


def test_kernel_name_query(hip_lib):
    for M in (1, 33, 256, 2048):
        for L in range(1, 9):
            for F in range(1, FD_MAX_BATCH + 1):
                want = NAME if F >= MIN_FRAMES[L] else ""
                assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == want, (M, L, F)
    for M, L, F in ((0, 4, 32), (-3, 4, 32), (256, 0, 32), (256, 9, 32), (256, 4, 0), (256, 4, FD_MAX_BATCH + 1)):
        assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == ""
    # never where the position launch itself does not apply
    for L in range(1, 9):
        for F in range(1, FD_MAX_BATCH + 1):
            if capi.fd_shared_ml_kernel_name(256, L, F) == "":
                assert capi.fd_shared_vectors_ml_kernel_name(256, L, F) == ""


def test_null_batch_is_invalid(hip_lib):
    f = hip_lib.fd_batch_deform_vectors_shared_ml_dev
    assert f(None, None, 0, None, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID
