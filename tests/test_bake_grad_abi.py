"""CPU: the C ABI of fd_deform_bake_grad* -- the exported symbols, fd_bake_grad_opts' layout, the contract in the header, the
argument checks that answer before any device work (tests/test_bake_abi.py's list under the new names), the plan header's
gradient constants, and the ground tests/test_gpu_bake_grad.py stands on: that tests/bake_grad_cases.py's dPsi is the
derivative of tests/bake_cases.py's Psi, and that the oracle's thin-plate weights reproduce affine maps on the rigs of the GPU
affine test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bake_cases as bc
import bake_grad_cases as bg
from conftest import HAVE_GPU, ROOT
from facedeform_amd import _build, capi
from test_bake_abi import test_oracle_reproduces_affine_maps_on_the_rig as _affine_on_the_rig

FNS = ["fd_deform_bake_grad", "fd_deform_bake_grad_dev"]
LD = bc.LD


def _header():
    return open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()


def _opts(struct_size=None, G32=None):
    o = capi.FdBakeGradOpts()
    o.struct_size = C.sizeof(capi.FdBakeGradOpts) if struct_size is None else struct_size
    o.G32 = G32
    return o


def test_symbols_exported(hip_lib):
    for name in FNS:
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move


def test_opts_layout():
    # int struct_size, int reserved, then one pointer
    assert C.sizeof(capi.FdBakeGradOpts) == 16
    names = [f[0] for f in capi.FdBakeGradOpts._fields_]
    assert names == ["struct_size", "reserved", "G32"]
    assert [getattr(capi.FdBakeGradOpts, n).offset for n in names] == [0, 4, 8]
    body = re.search(r"typedef struct fd_bake_grad_opts \{(.*?)\} fd_bake_grad_opts;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|double|float)\s*(\*?)\s*(\w+)\s*;", body)
    assert [(f[0], f[1], f[2]) for f in fields] == [("int", "", "struct_size"), ("int", "", "reserved"), ("float", "*", "G32")]
    # fd_bake_opts is not touched
    assert "typedef struct fd_bake_opts {" in _header() and C.sizeof(capi.FdBakeOpts) == 16


def test_contract_is_in_the_header():
    text = _header()
    assert "G[v][a][i] = f_v sum_j dPsi_vj/dx_a S_ji" in text
    assert "(A_v - I)[b][a] = sum_c Pi_v[b][c] sum_i delta_i[c] G[v][a][i]" in text
    assert "I + Pi_v sum_i delta'_i (x) G[v][.][i] = the A of fd_deform_vectors for the model built on delta'" in text
    assert "Pi stays out, as in the bake" in text
    assert "bit for bit (float)G" in text
    assert "A vertex's 3 x M block depends on its own inputs, the model and S only" in text
    assert "G is N x 3 x M fp64 row-major: vertex, component a of x, control point" in text
    for decl in ("typedef struct fd_bake_grad_opts {",
                 "int fd_deform_bake_grad_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2,",
                 "int fd_deform_bake_grad(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2,",
                 "double *d_G, const fd_bake_grad_opts *opts);",
                 "double *G, const fd_bake_grad_opts *opts);"):
        assert decl in text
    assert "#define FD_ABI_VERSION 9" in text


def test_engine_methods_exist():
    for name in ("deform_bake_grad", "deform_bake_grad_dev"):
        assert callable(getattr(capi.Engine, name))


@pytest.mark.parametrize("fn", FNS)
def test_null_context_is_invalid(hip_lib, fn):
    arr = (C.c_float * 3)()
    S = (C.c_double * 5)()
    out = (C.c_double * 9)()
    o = _opts()
    assert getattr(hip_lib, fn)(None, 0, None, None, None, None, None, 1.0, 1.0, None, 0, None, None) == capi.FD_E_INVALID
    assert getattr(hip_lib, fn)(None, 1, arr, None, None, None, None, 1.0, 1.0, S, 1, out, C.byref(o)) == capi.FD_E_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="needs a context handle without a device: the checks run before any HIP call")
@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_invalid_before_device_work(hip_lib, fn):
    # the stand-in handle of tests/test_bake_abi.py: zeroed memory the size of fd_ctx and more, which reads as a context with
    # M = 0 control points and no model; set_err writes into its message buffer
    buf = (C.c_char * (1 << 16))()
    ctx = C.cast(buf, C.c_void_p)
    call = getattr(hip_lib, fn)
    arr = (C.c_float * 3)()
    S = (C.c_double * 5)()
    out = (C.c_double * 9)()
    out32 = (C.c_float * 9)()
    ok32 = _opts(G32=C.cast(out32, C.c_void_p))
    if fn.endswith("_dev"):
        assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, None, 0, out, None) == capi.FD_E_INVALID   # NULL S
    assert call(ctx, -1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_INVALID        # N < 0
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 1, out, None) == capi.FD_E_INVALID         # M is not the context's
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, None) == capi.FD_E_INVALID        # no output at all
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, C.byref(_opts())) == capi.FD_E_INVALID   # G and G32 NULL
    small = _opts(struct_size=8, G32=C.cast(out32, C.c_void_p))
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, C.byref(small)) == capi.FD_E_INVALID      # opts too small
    assert call(ctx, 1, arr, None, arr, arr, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_INVALID           # a bad frame triple
    assert call(ctx, 1, arr, None, None, None, arr, 1.0, 1.0, S, 0, None, C.byref(ok32)) == capi.FD_E_INVALID
    # with every argument in order the same handle gets past these checks: it has no model
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, out, None) == capi.FD_E_NOT_BUILT
    assert call(ctx, 1, arr, None, None, None, None, 1.0, 1.0, S, 0, None, C.byref(ok32)) == capi.FD_E_NOT_BUILT


def test_plan_header_holds_the_gradient_constants():
    """The gradient launch's panel cap and its accumulator budget stand in fd_bake_plan.h beside the bake's; the plan and the
    one pack kernel take the cap as an argument."""
    text = open(os.path.join(_build.CSRC, "fd_bake_plan.h")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert val("kGradPanelTiles") in (4, 5) and val("kGradPanelTiles") * bc.TILE == bg.PG
    assert val("kPanelTiles") * bc.TILE == bc.PANEL                       # the bake keeps its layout
    asserts = re.findall(r"static_assert\((.*?)\);", text, re.S)
    assert sum("kGradPanelTiles" in a for a in asserts) >= 2
    assert re.search(r"Plan plan\(int C, int M, int cap = kPanelTiles\)", text)
    src = open(os.path.join(_build.CSRC, "fd_bake.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bk_bake_pack\w*\(", src)) == 1          # one pack kernel, not two
    assert "bake::plan(C, M, cap)" in src and "bake::kGradPanelTiles" in src


# ---- the restatement is a derivative ---------------------------------------------------------------------------------

DERIVATIVE_CASES = [(k, bc.M_RIG) for k in sorted(bc.KINDS)] + [("thin_plate", bc.PANEL + 1), ("qnn", bc.PANEL + 1)]


def _radii(oracle, kind_name, rest):
    """(centres, radii) in W's layout for the rig, from the oracle's build: the radii rule is the reference's."""
    from oracle import fd_oracle as fo
    kind, params = bc.KINDS[kind_name]
    table = np.concatenate([rest.astype(np.float64), rest.astype(np.float64)], axis=1)
    if kind == capi.KERNEL_GAUSSIAN_ML:
        tt, tab, _, radii = oracle.build_multilayer(table, params[0], int(params[1]), params[2], fo.TERM_LINEAR)
        assert tt == 1
        return tab[:, :3], radii
    rc, tt, _, radii = oracle.build(table, kind, params, fo.TERM_LINEAR)
    assert rc == 0 and tt == 1
    return rest.astype(np.float64), radii


@pytest.mark.parametrize("kind_name,M", DERIVATIVE_CASES)
def test_the_restatement_is_a_derivative(oracle, kind_name, M):
    """The central difference of tests/bake_cases.py's Psi in longdouble, h = 2^-20, against dPsi, over the 769 vertices that
    are not the 8 points on centres (thin-plate and biharmonic are not differentiable there; the table says 0), to 1e-6 of the
    case's largest |dPsi|.  The truncation term is h^2 / 6 times the third derivative: the closest vertex-centre distance on
    these rigs is 4.3e-3 (at 300 points), which puts it near 1e-8 for the steepest kind, biharmonic."""
    P = bc.inputs()[0]
    keep = np.r_[0:700, 708:bc.N_FULL]
    X = P[keep].astype(LD)
    assert X.shape[0] == 769
    kind = bc.KINDS[kind_name][0]
    centres, radii = _radii(oracle, kind_name, bc.rig(M))
    h = LD(2) ** -20
    got = bg.dpsi(kind, X, centres, radii, 4)
    scale = float(np.abs(got).max())
    worst = 0.0
    for a in range(3):
        e = np.zeros(3, LD); e[a] = h
        fd = (bc.psi(kind, X + e, centres, radii, 4) - bc.psi(kind, X - e, centres, radii, 4)) / (2 * h)
        worst = max(worst, float(np.abs(fd - got[:, a, :]).max()))
    print(f"derivative {kind_name} M={M}: worst |central difference - dPsi| = {worst:.3e}, largest |dPsi| = {scale:.3e}, "
          f"ratio {worst / scale:.3e}")
    assert worst <= 1e-6 * scale
    # the magnitude as computed bounds the value, and the columns a term lacks are zero in both
    assert (bg.dpsi_abs(kind, X, centres, radii, 4) >= np.abs(got)).all()
    assert not bg.dpsi(kind, X, centres, radii, 1)[:, :, centres.shape[0] + 1:].any()


@pytest.mark.parametrize("M", [bc.M_RIG, bc.PANEL + 1])
def test_oracle_reproduces_affine_maps_on_the_rig(oracle, M):
    """tests/test_bake_abi.py's check, on the rigs of tests/test_gpu_bake_grad.py's affine test: a model that reproduces x
    exactly has the Jacobian I, which is what that test asks of G."""
    _affine_on_the_rig(oracle, M)
