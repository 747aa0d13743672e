"""CPU: the C ABI of fd_batch_set_shared_lu -- one LU of the rest rig's kernel block for a shot of QNN models
(facedeform_amd/csrc/fd_build_qnn_shared.hip): the exported symbols, the kernel-name query and what the
header promises."""
import os

from conftest import ROOT
from facedeform_amd import capi

NAME = "k_qnn_solve_shared"
LIMIT = 1020            # the largest M whose padded order (M + 4 rounded up to 32) the LU without pivot search takes


def threshold():
    """The smallest frame count the shared build takes (the name query is its statement)."""
    return next(F for F in range(1, 33) if capi.fd_shared_qnn_build_kernel_name(256, F) != "")


def test_symbols_exported(hip_lib):
    for name in ("fd_batch_set_shared_lu", "fd_shared_qnn_build_kernel_name", "fd_batch_last_build_shared_factor"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hasattr(capi, "fd_shared_qnn_build_kernel_name")
    assert hasattr(capi.Batch, "set_shared_lu")
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_kernel_name_query(hip_lib):
    t = threshold()
    assert 2 <= t <= 32
    for M, F in ((20, 32), (33, 32), (256, 32), (1000, 32), (LIMIT, 32), (256, t), (1, t)):
        assert capi.fd_shared_qnn_build_kernel_name(M, F) == NAME
    for M in (0, -5):
        assert capi.fd_shared_qnn_build_kernel_name(M, 32) == ""
    for M in (LIMIT + 1, 1025, 2048, 5000):         # above the no-pivot limit
        assert capi.fd_shared_qnn_build_kernel_name(M, 32) == ""
    for F in (-3, 0, 1, 33, 64):
        assert capi.fd_shared_qnn_build_kernel_name(256, F) == ""
    for F in range(1, 40):
        for M in (20, 256, 700, 1000):
            assert capi.fd_shared_qnn_build_kernel_name(M, F) == (NAME if t <= F <= 32 else "")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    # below the multilayer query, and the other switch's comment left alone
    assert text.index("const char *fd_shared_ml_build_kernel_name(int M, int layers, int frames);") < text.index("One LU factorisation per batched build")
    decl = text[text.index("One LU factorisation per batched build"):text.index("int fd_batch_set_shared_lu(fd_batch *batch, int on);")]
    # what is shared
    assert "radii" in decl and "reflectors" in decl and "LU without pivot search ONCE" in decl and "ONE" in decl and "k_qnn_solve_shared" in decl
    # the conditions
    assert "FD_KERNEL_GAUSSIAN_QNN" in decl and "FD_SOLVER_AUTO" in decl and "at most 1024" in decl and "pivoted LU" in decl
    assert "polynomial columns" in decl and "SAME rest array" in decl and "minimum frame count" in decl and "scratch could be allocated" in decl
    # the delegation, and how close the results are
    assert "Delegation" in decl and "exactly as without the switch, bit for bit" in decl
    assert "to rounding, not bit for bit" in decl and "same bits on every" in decl and "radii are bit-identical" in decl
    assert "FD_SOLVER_LU_NOPIVOT" in decl and "-5 in every frame" in decl
    # the fallback, and that nothing is kept
    assert "Fallback" in decl and "every frame reports" in decl and "-4" in decl
    assert "FD_E_NOT_BUILT" in decl
    assert "const char *fd_shared_qnn_build_kernel_name(int M, int frames);" in text
    assert "#define FD_ABI_VERSION 9" in text


def test_source_is_built(hip_lib):
    from facedeform_amd import _build
    assert "fd_build_qnn_shared.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_build_qnn_shared.hip"))
    assert os.path.join(_build.CSRC, "fd_shared_solve.h") in _build.HEADERS
    # every header of csrc/ is a dependency of the build, and no translation unit reaches another one's text: what two of them
    # share is in a header (the one-frame helpers of the shot evaluations: fd_eval_point.h)
    names = sorted(os.listdir(_build.CSRC))
    for name in names:
        if name.endswith(".h"):
            assert os.path.join(_build.CSRC, name) in _build.HEADERS, name
        text = open(os.path.join(_build.CSRC, name)).read()
        assert "one_frame" not in text, name
        # what the host layer holds on the device is released by its owners (fd_owned.h), not from lists in the destroy functions
        if name in ("fd_capi.hip", "fd_morph.hip"):
            for call in ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipGraphExecDestroy("):
                assert call not in text, (name, call)
        for line in text.splitlines():
            if line.lstrip().startswith("#") and "include" in line:
                assert ".hip" not in line, (name, line)
