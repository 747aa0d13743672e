"""GPU: fd_deform_bake* -- B[v][i] = f_v sum_j Psi_vj S_ji, every control point's influence on every vertex
(include/facedeform_hip.h states the contract).

The yardstick is tests/bake_cases.py's restatement in np.longdouble: Psi built from the weights' layout, the rest rig and the
radii the engine reports, S the very array passed to the call, f the fall-off fd_deform reports; never the call's own output.
Inputs are tests/test_gpu_gram.py's recipe cut down to 777 vertices: head-mesh vertices, 8 points on centres, 69 points off the
surface, a gate that removes about a third, every 97th vertex exactly on the radius (f = 0), frames on and off.

The bars:
  restatement  per entry |B - ref| <= KAPPA 2^-53 |f| (|Psi| @ |S|); where that is 0 both sides are exact zeros.  KAPPA is four
               times the worst ratio measured on the MI355X over the cases of this file (the cases, every N of the shape test
               and the chunked host call), rounded up to a power of two, per family of kinds:
                 thin-plate, biharmonic, cubic   measured 4.23 (biharmonic, 64 points, vertex 707 column 7; thin-plate at most
                                                 3.33, at 257 points; 3.03 over the 349 569-vertex call; cubic 1.43),
                                                 asserted 32;
                 the Gaussian kinds              measured 56.73 (the plain Gaussian's one-point rig, vertex 767, an
                                                 off-surface point far from the centre; QNN 7.93 at 257 points, 7.92 at 300,
                                                 7.44 at 64 without a term; Gaussian 4.37 and the multilayer model 2.12 at 64),
                                                 asserted 256.
               The one-point figure is exp's conditioning alone: the entry is exp(-d2 / R^2) S with d2 / R^2 = 36.6, and exp(x)
               carries |x| ulps of the rounding of its argument.
               The margin covers the conditioning of phi in its fp64 argument, which differs from case to case; the sum itself
               is one accumulator on the matrix pipe and stays near the depth's ulps.  The thin-plate entries of S are far
               larger than Psi S, which is why the bar scales with |Psi| @ |S| and not with |B|.
  dual         the project's parity metric (conftest.l2_parity) between Pi_v sum_i B[v][i] delta'_i, Pi restated in longdouble,
               and fd_deform's own fp64 displacement for the model built on delta', stored in fp32: 1e-5.  Measured: at most 9.4e-08 without frames and
               2.1e-06 with them (multilayer, 4 layers), over the 17 cases.
  affine       thin-plate with the linear term: sum_i B[v][i] = f_v and sum_i B[v][i] c_i = f_v x_v to 1e-5 of the rig's
               extent (tests/test_bake_abi.py holds the oracle's weights to the same on this rig).  Measured: 3.6e-14 and
               3.2e-14 at 64 points, 5.3e-13 and 2.7e-13 at 257."""
import functools

import numpy as np
import pytest
import torch

import bake_cases as bc
from conftest import l2_parity
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = bc.LD
KAPPA = {"polyharmonic": 32.0, "gaussian": 256.0}
RADIUS2, RATE = bc.RADIUS2, bc.RATE


def _engine(kind_name, term, rest, delta, check=True):
    kind, params = bc.KINDS[kind_name]
    e = capi.Engine(device=0)
    e.set_points(rest, delta)
    e.set_kernel(kind, params)
    e.set_term(bc.TERMS[term])
    e.build(check=check)
    return e


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _kw(frames, N=None):
    P, tu, tv, nrm, dist2 = (a[:N] for a in bc.inputs())
    return P, dict(dist2=dist2, tangents=(tu, tv, nrm) if frames else None, radius2=RADIUS2, falloffrate=RATE)


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, M, frames):
    """One engine, the call under test on all vertices and everything the restatement needs, computed once."""
    P, kw = _kw(frames)
    rest = bc.rig(M)
    e = _engine(kind_name, term, rest, synth.rig_deltas(rest, 0))
    W, radii = e.get_weights()
    centres = np.tile(rest.astype(np.float64), ((W.shape[0] - 4) // M, 1))
    S = e.solve_operator()
    _, fall = e.deform(P, **kw)
    e.set_eval_precision(capi.EVAL_FP32)            # the bake is fp64 whatever the context says
    B, B32 = e.deform_bake(P, S=S, want_fp32=True, **kw)
    e.close()
    Psi = bc.psi(bc.KINDS[kind_name][0], P, centres, radii, bc.TERM_ROWS[term])
    ref, bar1, out = bc.restatement(Psi, S, fall, kw["dist2"])
    for a in (S, B, B32, fall):
        a.setflags(write=False)
    return dict(kind_name=kind_name, term=term, M=M, rest=rest, S=S, B=B, B32=B32, fall=fall, ref=ref, bar1=bar1, out=out)


def _hold(c, got, N=None, what=""):
    n = got.shape[0] if N is None else N
    r, at = bc.ratio(got, c["ref"][:n], c["bar1"][:n])
    print(f"restatement {c['kind_name']}/{c['term']} M={c['M']} {what}: worst |B - ref| / (2^-53 |f| |Psi| |S|) = {r:.2f} at {at}")
    assert r <= KAPPA[bc.FAMILY[c["kind_name"]]]
    return r


# ---- 1: against the restatement; B32 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,M,frames", bc.CASES)
def test_against_the_restatement(hip_lib, kind_name, term, M, frames):
    c = _case(kind_name, term, M, frames)
    assert c["B"].shape == (bc.N_FULL, M) and c["B"].dtype == np.float64 and np.isfinite(c["B"]).all()
    _hold(c, c["B"], what=f"frames={frames}")
    assert _same(c["B32"], c["B"].astype(np.float32))                    # rounded once, bit for bit
    assert c["out"].sum() > bc.N_FULL // 4 and (~c["out"]).sum() > bc.N_FULL // 4
    assert not c["B"][c["out"]].any() and c["B"][~c["out"]].any(axis=1).all()


def test_frames_are_accepted_and_unused(hip_lib):
    a, b = _case("thin_plate", "linear", bc.M_RIG, False), _case("thin_plate", "linear", bc.M_RIG, True)
    assert _same(a["B"], b["B"])


# ---- 2: launch shapes, determinism, the two forms ----------------------------------------------------------------------

SHAPE_RIGS = [("thin_plate", bc.M_RIG), ("thin_plate", 80), ("qnn", bc.PANEL + 1)]


@pytest.mark.parametrize("kind_name,M", SHAPE_RIGS)
def test_launch_shapes_and_determinism(hip_lib, kind_name, M):
    """N around a wave's tile and a workgroup's vertex group, each against the restatement and bit for bit the same rows of the
    full call; two calls agree; the host call and the device-pointer call agree, with B alone, B32 alone and both; entries
    beyond N M of an oversized output stay untouched; a sub-range of the vertices gives the same rows."""
    dev = torch.device("cuda", 0)
    c = _case(kind_name, "linear", M, False)
    P, kw = _kw(False)
    e = _engine(kind_name, "linear", c["rest"], synth.rig_deltas(c["rest"], 0))
    for N in bc.N_SHAPES:
        Pn, kwn = _kw(False, N)
        got, got32 = e.deform_bake(Pn, S=c["S"], want_fp32=True, **kwn)
        assert got.shape == (N, M) and got32.shape == (N, M)
        assert _same(got, c["B"][:N]) and _same(got32, c["B32"][:N]), N
        if N:
            _hold(c, got, N, what=f"N={N}")
    assert _same(e.deform_bake(P, S=c["S"], **kw), c["B"])
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_P, d_d2, d_S = T(P), T(kw["dist2"]), T(c["S"])
    size = c["B"].size
    for want64, want32 in ((True, True), (True, False), (False, True), (True, True)):
        d_B = torch.full((size + 11,), -7.25, dtype=torch.float64, device=dev)
        d_B32 = torch.full((size + 11,), -7.25, dtype=torch.float32, device=dev)
        e.deform_bake_dev(bc.N_FULL, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr() if want64 else 0,
                          d_B32.data_ptr() if want32 else 0, d_d2.data_ptr(), radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
        if want64:
            assert _same(d_B[:size].cpu().numpy().reshape(c["B"].shape), c["B"]) and (d_B[size:] == -7.25).all()
        else:
            assert (d_B == -7.25).all()
        if want32:
            assert _same(d_B32[:size].cpu().numpy().reshape(c["B"].shape), c["B32"]) and (d_B32[size:] == -7.25).all()
        else:
            assert (d_B32 == -7.25).all()
    # vertex ranges: any start, any length
    for a, b in ((1, 2), (5, 5 + bc.TILE), (bc.GROUP - 3, 2 * bc.GROUP + 7), (300, bc.N_FULL)):
        d_B = torch.full(((b - a) * M + 5,), -7.25, dtype=torch.float64, device=dev)
        e.deform_bake_dev(b - a, d_P.data_ptr() + 12 * a, d_S.data_ptr(), d_B.data_ptr(), 0, d_d2.data_ptr() + 4 * a,
                          radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
        assert _same(d_B[:(b - a) * M].cpu().numpy().reshape(b - a, M), c["B"][a:b]) and (d_B[(b - a) * M:] == -7.25).all()
    # no vertices: nothing is written
    d_B = torch.full((7,), -7.25, dtype=torch.float64, device=dev)
    e.deform_bake_dev(0, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr())
    e.synchronize()
    assert (d_B == -7.25).all()
    e.close()


def test_the_operator_computed_inside_the_call(hip_lib):
    """S = None has the call run fd_solve_operator itself; fd_set_output has no effect."""
    c = _case("qnn", "linear", 33, False)
    P, kw = _kw(False)
    e = _engine("qnn", "linear", c["rest"], synth.rig_deltas(c["rest"], 0))
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    got = e.deform_bake(P, **kw)
    e.close()
    assert _same(got, c["B"])


def test_host_chunks_are_one_launch(hip_lib):
    """B and B32 of 349 569 vertices by 64 points are 256 MiB and 129 rows more: the host call brings them back in two chunks,
    the second a workgroup's vertex group and one vertex.  Bit for bit the device-pointer call's one launch; the first rows
    and the rows around the chunk edge against the restatement."""
    dev = torch.device("cuda", 0)
    M = bc.M_RIG
    per = (256 << 20) // (12 * M) // bc.GROUP * bc.GROUP
    N = per + bc.GROUP + 1
    assert N == 349_569
    P = synth.head_mesh(N)
    dist2 = (np.random.default_rng(3).random(N) * 1.5 * RADIUS2).astype(np.float32)
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    rest = bc.rig(M)
    e = _engine("thin_plate", "linear", rest, synth.rig_deltas(rest, 0))
    S = e.solve_operator()
    B, B32 = e.deform_bake(P, S=S, want_fp32=True, **kw)
    d_P, d_d2, d_S = (torch.from_numpy(a).to(dev) for a in (P, dist2, S))
    d_B = torch.empty((N, M), dtype=torch.float64, device=dev)
    d_B32 = torch.empty((N, M), dtype=torch.float32, device=dev)
    e.deform_bake_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr(), d_B32.data_ptr(), d_d2.data_ptr(), radius2=RADIUS2,
                      falloffrate=RATE)
    e.synchronize()
    assert _same(d_B.cpu().numpy(), B) and _same(d_B32.cpu().numpy(), B32)
    del d_B, d_B32
    rows = np.r_[0:300, per - 300:N]
    _, fall = e.deform(P[rows], dist2=dist2[rows], radius2=RADIUS2, falloffrate=RATE)
    W, radii = e.get_weights()
    e.close()
    Psi = bc.psi(capi.KERNEL_THIN_PLATE, P[rows], rest.astype(np.float64), radii, 4)
    ref, bar1, _ = bc.restatement(Psi, S, fall, dist2[rows])
    r, at = bc.ratio(B[rows], ref, bar1)
    print(f"restatement thin_plate/linear M={M} N={N} (rows around the chunk edge): worst ratio {r:.2f} at {at}")
    assert r <= KAPPA["polyharmonic"]


# ---- 3: rows that are exactly zero ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,M", [("thin_plate", "linear", bc.M_RIG), ("qnn", "const", bc.M_RIG), ("qnn", "linear", bc.PANEL + 1)])
def test_rows_of_vertices_that_are_out_are_zero(hip_lib, kind_name, term, M):
    c = _case(kind_name, term, M, False)
    P, kw = _kw(False)
    gated = kw["dist2"] > np.float32(RADIUS2)
    f0 = (c["fall"] == 0) & ~gated
    assert gated.any() and f0.any()
    P_nan = P.copy(); P_nan[gated | f0] = np.nan                         # P is not read where the vertex is out
    e = _engine(kind_name, term, c["rest"], synth.rig_deltas(c["rest"], 0))
    got, got32 = e.deform_bake(P_nan, S=c["S"], want_fp32=True, **kw)
    e.close()
    assert np.isfinite(got).all() and _same(got, c["B"]) and _same(got32, c["B32"])
    zero = got[gated | f0]
    assert np.array_equal(_bits(zero), np.zeros(zero.shape, np.uint64))      # +0.0, every bit


def test_failed_build_gives_zeros(hip_lib):
    """Coincident control points: the build ends with -5 and is not repaired.  Enqueued right behind the build, whose status
    cannot be known yet, the launch sees a model whose forward map is the identity: zeros and FD_OK, with NaN in P.  Once the
    status is in, every call returns what fd_deform_dev returns."""
    dev = torch.device("cuda", 0)
    P, _ = _kw(False)
    M = bc.M_RIG
    rest = bc.rig(M)
    dup = rest.copy(); dup[17] = dup[40]
    e = capi.Engine(device=0)
    e.set_points(dup, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    N = P.shape[0]
    P_nan = P.copy(); P_nan[::5] = np.nan
    d_P = torch.from_numpy(P_nan).to(dev)
    d_S = torch.from_numpy(np.random.default_rng(1).standard_normal((M + 4, M))).to(dev)
    d_B = torch.full((N, M), -7.25, dtype=torch.float64, device=dev)
    d_def = torch.empty_like(d_P)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.deform_bake_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert np.array_equal(_bits(d_B.cpu().numpy()), np.zeros((N, M), np.uint64))
    rc_bake = rc_of(lambda: e.deform_bake_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_B.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_P.data_ptr(), d_def.data_ptr()))
    assert rc_bake == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    S = np.zeros((M + 4, M))
    assert rc_of(lambda: e.deform_bake(P, S=S)) == rc_of(lambda: e.deform(P)) == rc_def
    e.close()


def test_not_built_and_bad_arguments(hip_lib):
    P, tu, tv, _, _ = bc.inputs()
    M = bc.M_RIG
    e = capi.Engine(device=0)
    rest = bc.rig(M)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    S = np.zeros((M + 4, M))
    with pytest.raises(capi.FdError) as ei:
        e.deform_bake(P, S=S)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    e.build()
    out = np.empty((P.shape[0], M), np.float64)
    ptr = capi._np_ptr
    call = lambda *a: e.L.fd_deform_bake(e.ctx, *a)
    assert call(P.shape[0], ptr(P), None, ptr(tu), ptr(tv), None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_E_INVALID   # frames
    assert call(P.shape[0], ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M - 1, ptr(out), None) == capi.FD_E_INVALID     # M
    assert call(P.shape[0], ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, None, None) == capi.FD_E_INVALID             # no output
    assert call(-1, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_E_INVALID
    assert e.L.fd_deform_bake_dev(e.ctx, 1, ptr(P), None, None, None, None, 1.0, 1.0, None, M, ptr(out), None) == capi.FD_E_INVALID
    assert call(0, None, None, None, None, None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_OK
    e.close()


# ---- 4: dual to the library's own forward map ------------------------------------------------------------------------

DUAL_CASES = [(k, "linear", bc.M_RIG, fr) for k in sorted(bc.KINDS) for fr in (False, True)] + \
             [("thin_plate", "const", bc.M_RIG, False), ("qnn", "zero", bc.M_RIG, False), ("qnn", "linear", bc.PANEL + 1, False)]


@pytest.mark.parametrize("kind_name,term,M,frames", DUAL_CASES)
def test_dual_to_the_forward_map(hip_lib, kind_name, term, M, frames):
    """For random delta': fd_set_deltas(delta') and build (fd_set_points with delta' for the multilayer model), the fp64
    fd_deform with FD_OUTPUT_DISPLACEMENT, against Pi_v sum_i B[v][i] delta'_i."""
    c = _case(kind_name, term, M, frames)
    P, kw = _kw(frames)
    delta = (0.05 * np.random.default_rng(41).standard_normal(c["rest"].shape)).astype(np.float32)
    if kind_name.startswith("multilayer"):           # the multilayer build keeps no factorisation for fd_set_deltas: a fresh rig
        e = _engine(kind_name, term, c["rest"], delta)
    else:
        e = _engine(kind_name, term, c["rest"], synth.rig_deltas(c["rest"], 0))
        e.set_deltas(delta)
        e.build()
    e.set_eval_precision(capi.EVAL_FP64)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    D = e.deform(P, **kw)[0].astype(np.float64)
    e.close()
    recon = c["B"].astype(LD) @ delta.astype(LD)
    if frames:
        recon = np.einsum("vbc,vc->vb", bc.projection(*kw["tangents"]), recon)
    zero = np.zeros_like(D)
    parity = l2_parity(recon.astype(np.float64), D, zero)
    print(f"dual {kind_name}/{term} M={M} frames={frames}: parity of Pi B delta' against fd_deform's displacement = {parity:.3e}")
    assert np.abs(D).max() > 1e-3 and parity <= 1e-5


# ---- 5: thin-plate with the linear term reproduces affine maps --------------------------------------------------------

@pytest.mark.parametrize("M", [bc.M_RIG, bc.PANEL + 1])
def test_affine_reproduction(hip_lib, M):
    c = _case("thin_plate", "linear", M, False)
    P, _ = _kw(False)
    B, f = c["B"].astype(LD), np.where(c["out"], 0, c["fall"]).astype(LD)
    cen, X = c["rest"].astype(LD), P.astype(LD)
    extent = float(np.abs(c["rest"]).max())
    e1 = float(np.abs(B.sum(axis=1) - f).max())
    e2 = float(np.abs(B @ cen - f[:, None] * X).max())
    print(f"affine M={M}: worst |sum_i B - f| = {e1:.3e}, worst |sum_i B c_i - f x| = {e2:.3e}, bar {1e-5 * extent:.3e}")
    assert e1 <= 1e-5 * extent and e2 <= 1e-5 * extent
