"""CPU: the C ABI of fd_deform_bake* -- the exported symbols, fd_bake_opts' layout, the contract in the header, the argument
checks that answer before any device work (NULL context, NULL S in the device form, N < 0, M that is not the context's, both
outputs NULL, struct_size, a bad frame triple), the plan header's constants, and -- with the oracle's weights -- that the rig
tests/test_gpu_bake.py takes for its affine-reproduction check has the property the check asks for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bake_cases as bc
from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi

FNS = ["fd_deform_bake", "fd_deform_bake_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def _opts(struct_size=None, B32=None):
    o = capi.FdBakeOpts()
    o.struct_size = C.sizeof(capi.FdBakeOpts) if struct_size is None else struct_size
    o.B32 = B32
    return o


def test_symbols_exported(hip_lib):
    for name in FNS:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "fd_bake.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "fd_bake.hip"))
    assert os.path.join(_build.CSRC, "fd_bake_plan.h") in _build.HEADERS


def test_opts_layout():
    # int struct_size, int reserved, then one pointer
    assert C.sizeof(capi.FdBakeOpts) == 16
    names = [f[0] for f in capi.FdBakeOpts._fields_]
    assert names == ["struct_size", "reserved", "B32"]
    assert [getattr(capi.FdBakeOpts, n).offset for n in names] == [0, 4, 8]
    body = re.search(r"typedef struct fd_bake_opts \{(.*?)\} fd_bake_opts;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|double|float)\s*(\*?)\s*(\w+)\s*;", body)
    assert [(f[0], f[1], f[2]) for f in fields] == [("int", "", "struct_size"), ("int", "", "reserved"), ("float", "*", "B32")]


def test_contract_is_in_the_header():
    text = _header()
    assert "B[v][i] = f_v sum_j Psi_vj S_ji" in text
    assert "Pi_v sum_i B[v][i] delta'_i = D_v(S delta')" in text
    assert "Pi is a 3 x 3 and is not folded in" in text
    assert "bit for bit (float)B" in text
    assert "A caller short of memory bakes vertex ranges and gets the same bits." in text
    for decl in ("typedef struct fd_bake_opts {",
                 "int fd_deform_bake_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2,",
                 "int fd_deform_bake(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2,",
                 "float radius2, float falloffrate, const double *d_S, int M,",
                 "float radius2, float falloffrate, const double *S, int M,"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_bake", "deform_bake_dev"):
        assert callable(getattr(capi.Engine, name))


@pytest.mark.parametrize("fn", FNS)
def test_null_context_is_invalid(hip_lib, fn):
    arr = (C.c_float * 3)()
    S = (C.c_double * 5)()
    out = (C.c_double * 3)()
    o = _opts()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, 1.0, 1.0, None, 0, None, None) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 1, arr, None, None, None, None, 1.0, 1.0, S, 1, out, C.byref(o)) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_invalid_before_device_work(hip_lib, fn):
    # fd_create needs a device, so a stand-in handle (as tests/test_adjoint_abi.py): zeroed memory the size of fd_ctx and more,
    # which reads as a context with M = 0 control points and no model; set_err writes into its message buffer
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    S = (C.c_double * 5)()
    out = (C.c_double * 3)()
    out32 = (C.c_float * 3)()
    ok32 = _opts(B32=C.cast(out32, C.c_void_p))
    if fn.endswith("_dev"):
        assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, None, 0, out, None) == capi.FD_E_INVALID   # NULL S
    assert call(ctx, -1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_INVALID        # N < 0
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 1, out, None) == capi.FD_E_INVALID         # M is not the context's
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, None) == capi.FD_E_INVALID        # no output at all
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, C.byref(_opts())) == capi.FD_E_INVALID   # B and B32 NULL
    small = _opts(struct_size=8, B32=C.cast(out32, C.c_void_p))
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, C.byref(small)) == capi.FD_E_INVALID      # opts too small
    assert call(ctx, 1, arr, None, arr, arr, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_INVALID           # a bad frame triple
    assert call(ctx, 1, arr, None, None, None, arr, 1.0, 1.0, S, 0, None, C.byref(ok32)) == capi.FD_E_INVALID
    # with every argument in order the same handle gets past these checks: it has no model
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_NOT_BUILT
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, C.byref(ok32)) == capi.FD_E_NOT_BUILT


def test_plan_header_holds_the_layout():
    """The pack kernel and the launch take every layout constant from fd_bake_plan.h; the constants tests/bake_cases.py
    restates for the shapes are the header's."""
    text = open(os.path.join(_build.CSRC, "fd_bake_plan.h")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert val("kTile") == bc.TILE and val("kTile") * val("kWaves") == bc.GROUP and val("kPanelTiles") * val("kTile") == bc.PANEL
    assert "static_assert" in text
    src = open(os.path.join(_build.CSRC, "fd_bake.hip")).read()
    assert '#include "fd_bake_plan.h"' in src and "bake::plan(" in src


@pytest.mark.parametrize("M", [bc.M_RIG, bc.PANEL + 1])
def test_oracle_reproduces_affine_maps_on_the_rig(oracle, M):
    """Thin-plate with the linear term interpolates affine data exactly: deltas that are all (1, 1, 1) deform every point by
    (1, 1, 1), and deltas delta_i = c_i deform x by x.  In terms of S these are sum_i (Psi S)[v][i] = 1 and
    sum_i (Psi S)[v][i] c_i = x_v, what tests/test_gpu_bake.py asks of B.  Checked here with the oracle's weights for that
    test's rigs, to 1e-5 of the rig's extent, its bar."""
    from oracle import fd_oracle as fo
    rest = bc.rig(M).astype(np.float64)
    extent = float(np.abs(rest).max())
    x = bc.inputs()[0].astype(np.float64)
    for delta, want in ((np.ones_like(rest), np.ones_like(x)), (rest, x)):
        table = np.concatenate([rest, delta], axis=1)
        rc, tt, W, radii = oracle.build(table, fo.KERNEL_THIN_PLATE, (), fo.TERM_LINEAR)
        assert rc == 0 and tt == 1
        got = oracle.eval(table, fo.KERNEL_THIN_PLATE, radii, W, x)
        err = float(np.abs(got - want).max())
        print(f"oracle, affine data: worst |eval - exact| = {err:.3e}, bar {1e-5 * extent:.3e}")
        assert err <= 1e-5 * extent
