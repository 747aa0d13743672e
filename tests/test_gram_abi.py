"""CPU: the C ABI of fd_deform_gram* and fd_fit_deltas -- the exported symbols, the contract in the header, and the argument
checks that answer before any device work (NULL context, NULL H / T / delta_out, N < 0, mu < 0, a report too small)."""
import ctypes as C
import os

import pytest

from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

GRAM_FNS = ["fd_deform_gram", "fd_deform_gram_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def test_gram_symbols_exported(hip_lib):
    for name in GRAM_FNS + ["fd_fit_deltas"]:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_gram.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_gram.hip"))


def test_contract_is_in_the_header():
    text = _header()
    assert "the Gram operator and the fit" in text
    assert "H[q][j][k] = sum_v omega_v f_v^2 (Pi_v^2)[b][c] Psi_vj Psi_vk        q <-> (b,c)" in text
    assert "sum_{b,c} sum_{j,k} W'[j][b] H[q(b,c)][j][k] W''[k][c] = sum_v omega_v D_v(W') . D_v(W'')" in text
    assert "D_v(W) = f_v Pi_v (Psi_v W)" in text
    assert "ordered xx, xy, xz, yy, yz, zz" in text
    assert "the lower is the mirror of" in text
    assert "E(delta) = sum_v omega_v |D_v(S delta) - (T_v - P_v)|^2 + mu sum_i |delta_i - delta0_i|^2" in text
    assert "at most 256 MiB" in text
    for decl in ("int fd_deform_gram_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_omega, const float *d_dist2,",
                 "int fd_deform_gram(fd_ctx *ctx, int64_t N, const float *P_in, const float *omega, const float *dist2,",
                 "int fd_fit_deltas(fd_ctx *ctx, int64_t N, const float *P_in, const float *T, const float *omega, const float *dist2,",
                 "#define FD_FIT_MAX_ROWS 1028", "#define FD_FIT_MAX_ORDER 3072", "} fd_fit_report;"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_gram", "deform_gram_dev", "fit_deltas"):
        assert callable(getattr(capi.Engine, name))
    # the Python mirror of fd_fit_report: two ints and eight doubles, struct_size first
    assert capi.FdFitReport._fields_[0][0] == "struct_size" and C.sizeof(capi.FdFitReport) == 8 + 8 * 8


def _fit(lib, ctx, N, P, T, out, mu=0.0, report=None):
    return lib.fd_fit_deltas(ctx, N, P, T, None, None, None, None, None, 1.0, 1.0, mu, None, None, out, report)


def test_null_context_is_invalid(hip_lib):
    arr = (C.c_float * 3)()
    out = (C.c_double * 64)()
    for fn in GRAM_FNS:
        assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID
        assert getattr(hip_lib, fn)(None, 1, arr, None, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID
    assert _fit(hip_lib, None, 0, None, None, None) == capi.FD_E_INVALID
    assert _fit(hip_lib, None, 1, arr, arr, out) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
def test_bad_arguments_are_invalid_before_device_work(hip_lib):
    # a stand-in handle (as tests/test_adjoint_abi.py): the checks read only the arguments and set_err writes into the context's
    # message buffer -- give it one the size of fd_ctx's.  Zeroed, it is a context with no points and no model.
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    arr = (C.c_float * 3)()
    out = (C.c_double * 64)()
    for fn in GRAM_FNS:
        call = getattr(hip_lib, fn)
        assert call(ctx, 1, arr, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID      # NULL H
        assert call(ctx, 0, None, None, None, None, None, None, 1.0, 1.0, None) == capi.FD_E_INVALID     # NULL H, even with N = 0
        assert call(ctx, -1, arr, None, None, None, None, None, 1.0, 1.0, out) == capi.FD_E_INVALID      # N < 0
    assert _fit(hip_lib, ctx, 1, arr, None, out) == capi.FD_E_INVALID                                    # NULL T
    assert _fit(hip_lib, ctx, 1, arr, arr, None) == capi.FD_E_INVALID                                    # NULL delta_out
    assert _fit(hip_lib, ctx, -1, arr, arr, out) == capi.FD_E_INVALID                                    # N < 0
    assert _fit(hip_lib, ctx, 1, None, arr, out) == capi.FD_E_INVALID                                    # NULL P with N > 0
    assert _fit(hip_lib, ctx, 1, arr, arr, out, mu=-1e-9) == capi.FD_E_INVALID                           # mu < 0
    assert _fit(hip_lib, ctx, 1, arr, arr, out, mu=float("nan")) == capi.FD_E_INVALID
    small = capi.FdFitReport()
    small.struct_size = C.sizeof(capi.FdFitReport) - 1
    assert _fit(hip_lib, ctx, 1, arr, arr, out, report=C.byref(small)) == capi.FD_E_INVALID              # struct_size too small
    good = capi.FdFitReport()
    good.struct_size = C.sizeof(capi.FdFitReport)
    # everything in order as far as the arguments go: the next check is the model's
    assert _fit(hip_lib, ctx, 1, arr, arr, out, report=C.byref(good)) == capi.FD_E_NOT_BUILT
