"""GPU: fd_deform_bake_grad* -- G[v][a][i] = f_v sum_j dPsi_vj/dx_a S_ji, the baked deformer differentiated once in x
(include/facedeform_hip.h states the contract).

The yardstick is tests/bake_grad_cases.py's restatement in np.longdouble: dPsi from the header's table, built from the
weights' layout, the rest rig and the radii the engine reports (tests/test_bake_grad_abi.py holds it to the central difference
of Psi), S the very array passed to the call, f the fall-off fd_deform reports; never the call's own output.  Inputs are
tests/bake_cases.py's 777 vertices: head-mesh vertices, 8 points on centres, 69 points off the surface, a gate that removes
about a third, every 97th vertex exactly on the radius (f = 0), frames on and off.

The bars:
  restatement  per entry |G - ref| <= KAPPA 2^-53 |f| (dPsi_abs @ |S|); where that is 0 both sides are exact zeros.  dPsi_abs is
               |dPsi|, for thin-plate |x_a - c_a| (|ln d2| + 1).  KAPPA is four times the worst ratio measured on the MI355X
               over the cases of this file (the cases, every N of the shape test and the rows of the chunked host call),
               rounded up to a power of two, per family of kinds:
                 thin-plate, biharmonic, cubic   measured 5.33 (biharmonic, 64 points, vertex 69, component 1, column 6;
                                                 thin-plate at most 2.53, at 257 points; 1.65 over the rows of the
                                                 120 000-vertex call; cubic 1.66), asserted 32;
                 the Gaussian kinds              measured 56.97 (the plain Gaussian's one-point rig, vertex 767, component 0,
                                                 an off-surface point far from the centre; 23.51 on the three-point rig; QNN
                                                 15.00 at 257 points, 14.22 at 64 with the constant term, 13.31 at 129;
                                                 Gaussian 10.91 and the multilayer model 6.17 at 64), asserted 256.
               The margin covers the conditioning of the kind's transcendental in its fp64 argument, which differs from case
               to case (exp(x) carries |x| ulps of its argument's rounding; the one-point Gaussian rig has d2 / R^2 = 36.6 at
               its worst vertex); the sum itself is one accumulator on the matrix pipe.
  dual         conftest.l2_parity_ulp over the nine entries of A per vertex, between I + Pi sum_i delta'_i (x) G[v][.][i] (Pi
               restated in longdouble) and the jacobian fd_deform_vectors writes in fp32 for the model built on delta' and
               evaluated in fp64:  |err|_2 <= 1e-5 max(|A_ref - I|_2, 1e-5 max_v) + |ulp32(A_ref)|_2.  Measured: between 0.38 and
               0.46 of the bar over the 16 cases (QNN with frames the largest), the rounding of A to fp32; |A - I| reaches 0.17.
  affine       thin-plate with the linear term: sum_i G[v][a][i] = 0 and sum_i G[v][a][i] c_i[b] = f_v delta_ab to 1e-5 of the
               rig's extent (tests/test_bake_grad_abi.py holds the oracle's weights to the same on these rigs).  Measured:
               8.3e-14 and 5.2e-14 at 64 points, 1.0e-12 and 5.0e-13 at 257."""
import functools

import numpy as np
import pytest
import torch

import bake_cases as bc
import bake_grad_cases as bg
from conftest import l2_parity_ulp
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = bc.LD
KAPPA = {"polyharmonic": 32.0, "gaussian": 256.0}
RADIUS2, RATE = bc.RADIUS2, bc.RATE
SENTINEL = -7.25


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


def _reference(kind_name, term, rest, W, radii, S, P, fall, dist2):
    centres = np.tile(rest.astype(np.float64), ((W.shape[0] - 4) // rest.shape[0], 1))
    kind, rows = bc.KINDS[kind_name][0], bc.TERM_ROWS[term]
    return bg.restatement(bg.dpsi(kind, P, centres, radii, rows), bg.dpsi_abs(kind, P, centres, radii, rows), S, fall, dist2)


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, M, frames):
    """One engine, the call under test on all vertices and everything the restatement needs, computed once."""
    P, kw = _kw(frames)
    rest = bc.rig(M)
    e = _engine(kind_name, term, rest, synth.rig_deltas(rest, 0))
    W, radii = e.get_weights()
    S = e.solve_operator()
    _, fall = e.deform(P, **kw)
    e.set_eval_precision(capi.EVAL_FP32)            # the call is fp64 whatever the context says
    G, G32 = e.deform_bake_grad(P, S=S, want_fp32=True, **kw)
    e.close()
    ref, bar1, out = _reference(kind_name, term, rest, W, radii, S, P, fall, kw["dist2"])
    for a in (S, G, G32, fall):
        a.setflags(write=False)
    return dict(kind_name=kind_name, term=term, M=M, rest=rest, S=S, G=G, G32=G32, fall=fall, ref=ref, bar1=bar1, out=out)


def _host_g32_alone(e, P, dist2, S):
    """The host form with G = NULL and opts->G32 set (Engine.deform_bake_grad always asks for G)."""
    ptr = capi._np_ptr
    P, dist2, S = (np.ascontiguousarray(a) for a in (P, dist2, S))
    out32 = np.full((P.shape[0], 3, e.M), SENTINEL, np.float32)
    opts = capi.FdBakeGradOpts(capi.C.sizeof(capi.FdBakeGradOpts), 0, ptr(out32))
    rc = e.L.fd_deform_bake_grad(e.ctx, P.shape[0], ptr(P), ptr(dist2), None, None, None, RADIUS2, RATE, ptr(S), e.M, None,
                                 capi.C.byref(opts))
    assert rc == capi.FD_OK
    return out32


def _hold(c, got, N=None, what=""):
    n = got.shape[0] if N is None else N
    r, at = bc.ratio(got, c["ref"][:n], c["bar1"][:n])
    print(f"restatement {c['kind_name']}/{c['term']} M={c['M']} {what}: worst |G - ref| / (2^-53 |f| |dPsi| |S|) = {r:.2f} at {at}")
    assert r <= KAPPA[bc.FAMILY[c["kind_name"]]]
    return r


# ---- 1: against the restatement; G32 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,M,frames", bg.CASES)
def test_against_the_restatement(hip_lib, kind_name, term, M, frames):
    c = _case(kind_name, term, M, frames)
    assert c["G"].shape == (bc.N_FULL, 3, M) and c["G"].dtype == np.float64 and np.isfinite(c["G"]).all()
    _hold(c, c["G"], what=f"frames={frames}")
    assert _same(c["G32"], c["G"].astype(np.float32))                    # rounded once, bit for bit
    assert c["out"].sum() > bc.N_FULL // 4 and (~c["out"]).sum() > bc.N_FULL // 4
    assert not c["G"][c["out"]].any() and c["G"][~c["out"]].any(axis=(1, 2)).all()


# ---- 2: the frames ---------------------------------------------------------------------------------------------------

def test_frames_are_accepted_and_unused(hip_lib):
    a, b = _case("thin_plate", "linear", bc.M_RIG, False), _case("thin_plate", "linear", bc.M_RIG, True)
    assert _same(a["G"], b["G"]) and _same(a["G32"], b["G32"])


# ---- 3: launch shapes, determinism, the two forms ----------------------------------------------------------------------

SHAPE_RIGS = [("thin_plate", bc.M_RIG), ("thin_plate", bg.PG + 1), ("qnn", bc.PANEL + 1)]


@pytest.mark.parametrize("kind_name,M", SHAPE_RIGS)
def test_launch_shapes_and_determinism(hip_lib, kind_name, M):
    """N around a wave's tile and a workgroup's vertex group, each against the restatement and bit for bit the same rows of the
    full call; two calls agree; the host call and the device-pointer call agree, with G alone, G32 alone and both; entries
    beyond 3 N M of an oversized output stay untouched, and so does an output that was not asked for; a sub-range of the
    vertices gives the same rows; no vertices, nothing written."""
    dev = torch.device("cuda", 0)
    c = _case(kind_name, "linear", M, False)
    P, kw = _kw(False)
    e = _engine(kind_name, "linear", c["rest"], synth.rig_deltas(c["rest"], 0))
    for N in bc.N_SHAPES:
        Pn, kwn = _kw(False, N)
        got, got32 = e.deform_bake_grad(Pn, S=c["S"], want_fp32=True, **kwn)
        assert got.shape == (N, 3, M) and got32.shape == (N, 3, M)
        assert _same(got, c["G"][:N]) and _same(got32, c["G32"][:N]), N
        if N:
            _hold(c, got, N, what=f"N={N}")
    assert _same(e.deform_bake_grad(P, S=c["S"], **kw), c["G"])          # G alone, host form; a second call
    assert _same(_host_g32_alone(e, P, kw["dist2"], c["S"]), c["G32"])   # G32 alone, host form
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_P, d_d2, d_S = T(P), T(kw["dist2"]), T(c["S"])
    size = c["G"].size
    for want64, want32 in ((True, True), (True, False), (False, True), (True, True)):
        d_G = torch.full((size + 11,), SENTINEL, dtype=torch.float64, device=dev)
        d_G32 = torch.full((size + 11,), SENTINEL, dtype=torch.float32, device=dev)
        e.deform_bake_grad_dev(bc.N_FULL, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr() if want64 else 0,
                               d_G32.data_ptr() if want32 else 0, d_d2.data_ptr(), radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
        if want64:
            assert _same(d_G[:size].cpu().numpy().reshape(c["G"].shape), c["G"]) and (d_G[size:] == SENTINEL).all()
        else:
            assert (d_G == SENTINEL).all()
        if want32:
            assert _same(d_G32[:size].cpu().numpy().reshape(c["G"].shape), c["G32"]) and (d_G32[size:] == SENTINEL).all()
        else:
            assert (d_G32 == SENTINEL).all()
    # vertex ranges: any start, any length
    for a, b in ((1, 2), (5, 5 + bc.TILE), (bc.GROUP - 3, 2 * bc.GROUP + 7), (300, bc.N_FULL)):
        n = (b - a) * 3 * M
        d_G = torch.full((n + 5,), SENTINEL, dtype=torch.float64, device=dev)
        e.deform_bake_grad_dev(b - a, d_P.data_ptr() + 12 * a, d_S.data_ptr(), d_G.data_ptr(), 0, d_d2.data_ptr() + 4 * a,
                               radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
        assert _same(d_G[:n].cpu().numpy().reshape(b - a, 3, M), c["G"][a:b]) and (d_G[n:] == SENTINEL).all()
    # no vertices: nothing is written
    d_G = torch.full((7,), SENTINEL, dtype=torch.float64, device=dev)
    e.deform_bake_grad_dev(0, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr())
    e.synchronize()
    assert (d_G == SENTINEL).all()
    # the bake behind the gradient on the same context packs its own layout again: its bits are its own
    B1 = e.deform_bake(P, S=c["S"], **kw)
    e.deform_bake_grad(P[:bc.GROUP], S=c["S"], dist2=kw["dist2"][:bc.GROUP], radius2=RADIUS2, falloffrate=RATE)
    assert _same(e.deform_bake(P, S=c["S"], **kw), B1)
    e.close()


def test_the_operator_computed_inside_the_call(hip_lib):
    """S = None has the call run fd_solve_operator itself; fd_set_output has no effect."""
    c = _case("qnn", "linear", 33, False)
    P, kw = _kw(False)
    e = _engine("qnn", "linear", c["rest"], synth.rig_deltas(c["rest"], 0))
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    got = e.deform_bake_grad(P, **kw)
    e.close()
    assert _same(got, c["G"])


# ---- 4: the host call's chunks ------------------------------------------------------------------------------------------

def test_host_chunks_are_one_launch(hip_lib):
    """120 000 vertices by 64 points: 3 M doubles and floats per vertex are 2 304 bytes, so the host call brings G and G32
    back in chunks of 116 480 vertices (256 MiB / 2 304, in whole vertex groups) -- two chunks, the second 3 520 vertices.
    Bit for bit the device-pointer call's one launch; the first rows, the last and the rows around the chunk edge -- and around
    77 568, where chunks of 18 bytes an entry would end -- against the restatement."""
    dev = torch.device("cuda", 0)
    M, N = bc.M_RIG, 120_000
    per = (256 << 20) // (3 * M * 12) // bc.GROUP * bc.GROUP
    assert per == 116_480 and per < N < 2 * per
    P = synth.head_mesh(N)
    dist2 = (np.random.default_rng(3).random(N) * 1.5 * RADIUS2).astype(np.float32)
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    rest = bc.rig(M)
    e = _engine("thin_plate", "linear", rest, synth.rig_deltas(rest, 0))
    S = e.solve_operator()
    G, G32 = e.deform_bake_grad(P, S=S, want_fp32=True, **kw)
    d_P, d_d2, d_S = (torch.from_numpy(a).to(dev) for a in (P, dist2, S))
    d_G = torch.empty((N, 3, M), dtype=torch.float64, device=dev)
    d_G32 = torch.empty((N, 3, M), dtype=torch.float32, device=dev)
    e.deform_bake_grad_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr(), d_G32.data_ptr(), d_d2.data_ptr(), radius2=RADIUS2,
                           falloffrate=RATE)
    e.synchronize()
    assert _same(d_G.cpu().numpy(), G) and _same(d_G32.cpu().numpy(), G32)
    del d_G, d_G32
    rows = np.r_[0:200, 77_568 - 200:77_568 + 200, per - 200:per + 200, N - 200:N]
    _, fall = e.deform(P[rows], dist2=dist2[rows], radius2=RADIUS2, falloffrate=RATE)
    W, radii = e.get_weights()
    e.close()
    ref, bar1, _ = _reference("thin_plate", "linear", rest, W, radii, S, P[rows], fall, dist2[rows])
    r, at = bc.ratio(G[rows], ref, bar1)
    print(f"restatement thin_plate/linear M={M} N={N} (rows around the chunk edges): worst ratio {r:.2f} at {at}")
    assert r <= KAPPA["polyharmonic"]


@pytest.mark.parametrize("which,entry_bytes,N", [("G", 8, 174_849), ("G32", 4, 349_569)])
def test_host_chunks_with_one_output(hip_lib, which, entry_bytes, N):
    """With one output the chunk is longer -- at 64 points 174 720 vertices for G alone (1 536 bytes a vertex) and 349 440 for
    G32 alone (768) -- so the host call is split only from there: N a chunk, a vertex group and one vertex.  Bit for bit the
    device-pointer call's one launch.  The rows around the chunk edge, computed once more in fp64 by a launch of their own, are
    held to the restatement, and the host call's rows are those bits (G32 alone: those rounded once to fp32)."""
    dev = torch.device("cuda", 0)
    M = bc.M_RIG
    per = (256 << 20) // (3 * M * entry_bytes) // bc.GROUP * bc.GROUP
    assert N == per + bc.GROUP + 1
    P = synth.head_mesh(N)
    dist2 = (np.random.default_rng(3).random(N) * 1.5 * RADIUS2).astype(np.float32)
    rest = bc.rig(M)
    e = _engine("thin_plate", "linear", rest, synth.rig_deltas(rest, 0))
    S = e.solve_operator()
    if which == "G":
        host = e.deform_bake_grad(P, S=S, dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    else:
        host = _host_g32_alone(e, P, dist2, S)
    d_P, d_d2, d_S = (torch.from_numpy(a).to(dev) for a in (P, dist2, S))
    d_out = torch.empty((N, 3, M), dtype=torch.float64 if which == "G" else torch.float32, device=dev)
    e.deform_bake_grad_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_out.data_ptr() if which == "G" else 0,
                           d_out.data_ptr() if which == "G32" else 0, d_d2.data_ptr(), radius2=RADIUS2, falloffrate=RATE)
    e.synchronize()
    assert _same(d_out.cpu().numpy(), host)
    del d_out
    rows = np.r_[0:200, per - 200:N]
    # the edge rows in fp64 from a launch of their own: a vertex's block depends on nothing else
    d_rows = torch.empty((rows.size, 3, M), dtype=torch.float64, device=dev)
    d_Pr, d_dr = torch.from_numpy(P[rows]).to(dev), torch.from_numpy(dist2[rows]).to(dev)
    e.deform_bake_grad_dev(rows.size, d_Pr.data_ptr(), d_S.data_ptr(), d_rows.data_ptr(), 0, d_dr.data_ptr(), radius2=RADIUS2,
                           falloffrate=RATE)
    e.synchronize()
    G_rows = d_rows.cpu().numpy()
    _, fall = e.deform(P[rows], dist2=dist2[rows], radius2=RADIUS2, falloffrate=RATE)
    W, radii = e.get_weights()
    e.close()
    ref, bar1, _ = _reference("thin_plate", "linear", rest, W, radii, S, P[rows], fall, dist2[rows])
    r, at = bc.ratio(G_rows, ref, bar1)
    print(f"restatement thin_plate/linear M={M} N={N} {which} alone (rows around the chunk edge): worst ratio {r:.2f} at {at}")
    assert r <= KAPPA["polyharmonic"]
    assert _same(host[rows], G_rows if which == "G" else G_rows.astype(np.float32))


# ---- 5: blocks that are exactly zero ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,M", [("thin_plate", "linear", bc.M_RIG), ("qnn", "const", bc.M_RIG), ("qnn", "linear", bc.PANEL + 1)])
def test_blocks_of_vertices_that_are_out_are_zero(hip_lib, kind_name, term, M):
    c = _case(kind_name, term, M, False)
    P, kw = _kw(False)
    gated = kw["dist2"] > np.float32(RADIUS2)
    f0 = (c["fall"] == 0) & ~gated
    assert gated.any() and f0.any()
    P_nan = P.copy(); P_nan[gated | f0] = np.nan                         # P is not read where the vertex is out
    e = _engine(kind_name, term, c["rest"], synth.rig_deltas(c["rest"], 0))
    got, got32 = e.deform_bake_grad(P_nan, S=c["S"], want_fp32=True, **kw)
    e.close()
    assert np.isfinite(got).all() and _same(got, c["G"]) and _same(got32, c["G32"])
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
    d_G = torch.full((N, 3, M), SENTINEL, dtype=torch.float64, device=dev)
    d_def = torch.empty_like(d_P)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.deform_bake_grad_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert np.array_equal(_bits(d_G.cpu().numpy()), np.zeros((N, 3, M), np.uint64))
    rc_grad = rc_of(lambda: e.deform_bake_grad_dev(N, d_P.data_ptr(), d_S.data_ptr(), d_G.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_P.data_ptr(), d_def.data_ptr()))
    assert rc_grad == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    S = np.zeros((M + 4, M))
    assert rc_of(lambda: e.deform_bake_grad(P, S=S)) == rc_of(lambda: e.deform(P)) == rc_def
    e.close()


def test_not_built_and_bad_arguments(hip_lib):
    P, tu, tv, _, _ = bc.inputs()
    M = bc.M_RIG
    e = capi.Engine(device=0)
    rest = bc.rig(M)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    S = np.zeros((M + 4, M))
    with pytest.raises(capi.FdError) as ei:
        e.deform_bake_grad(P, S=S)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    e.build()
    out = np.empty((P.shape[0], 3, M), np.float64)
    out32 = np.empty((P.shape[0], 3, M), np.float32)
    ptr = capi._np_ptr
    call = lambda *a: e.L.fd_deform_bake_grad(e.ctx, *a)
    n = P.shape[0]
    assert call(n, ptr(P), None, ptr(tu), ptr(tv), None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_E_INVALID   # frames
    assert call(n, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M - 1, ptr(out), None) == capi.FD_E_INVALID     # M
    assert call(n, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, None, None) == capi.FD_E_INVALID             # no output
    empty = capi.FdBakeGradOpts(16, 0, None)
    assert call(n, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, None, capi.C.byref(empty)) == capi.FD_E_INVALID
    small = capi.FdBakeGradOpts(8, 0, ptr(out32))
    assert call(n, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, ptr(out), capi.C.byref(small)) == capi.FD_E_INVALID
    assert call(-1, ptr(P), None, None, None, None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_E_INVALID
    assert e.L.fd_deform_bake_grad_dev(e.ctx, 1, ptr(P), None, None, None, None, 1.0, 1.0, None, M, ptr(out), None) == capi.FD_E_INVALID
    assert call(0, None, None, None, None, None, 1.0, 1.0, ptr(S), M, ptr(out), None) == capi.FD_OK
    e.close()


# ---- 6: dual to fd_deform_vectors' Jacobian ---------------------------------------------------------------------------

DUAL_CASES = [(k, "linear", bc.M_RIG, fr) for k in sorted(bc.KINDS) for fr in (False, True)] + \
             [("thin_plate", "linear", bc.PANEL + 1, False), ("qnn", "linear", bc.PANEL + 1, False)]


@pytest.mark.parametrize("kind_name,term,M,frames", DUAL_CASES)
def test_dual_to_the_jacobian(hip_lib, kind_name, term, M, frames):
    """For the deltas delta' of another frame of the rig: the model built on delta', evaluated in fp64, writes its Jacobian A
    (fp32); against I + Pi_v sum_i delta'_i (x) G[v][.][i].  Vertices that are out have A = I exactly on both sides."""
    c = _case(kind_name, term, M, frames)
    P, kw = _kw(frames)
    delta = synth.rig_deltas(c["rest"], 3)
    e = _engine(kind_name, term, c["rest"], delta)
    e.set_eval_precision(capi.EVAL_FP64)
    A = e.deform_vectors(P, want_jacobian=True, **kw)[5].astype(np.float64)
    e.close()
    # (A - I)[v][b][a] = sum_c Pi[v][b][c] sum_i delta'_i[c] G[v][a][i]
    J = np.einsum("vai,ic->vca", c["G"].astype(LD), delta.astype(LD))
    if frames:
        J = np.einsum("vbc,vca->vba", bc.projection(*kw["tangents"]), J)
    eye = np.eye(3)
    recon = (eye[None].astype(LD) + J).astype(np.float64)
    assert np.array_equal(A[c["out"]], np.broadcast_to(eye, A[c["out"]].shape)) and np.array_equal(recon[c["out"]], A[c["out"]])
    flat = lambda a: np.ascontiguousarray(a).reshape(a.shape[0], 9)
    worst = l2_parity_ulp(flat(recon), flat(A), flat(np.broadcast_to(eye, A.shape)))
    print(f"dual {kind_name}/{term} M={M} frames={frames}: |I + Pi delta' (x) G - A|_2 over its bar, worst vertex = {worst:.3e}; "
          f"largest |A - I| = {np.abs(A - eye).max():.3e}")
    assert np.abs(A - eye).max() > 1e-3 and worst <= 1.0


# ---- 7: thin-plate with the linear term reproduces affine maps ----------------------------------------------------------

@pytest.mark.parametrize("M", [bc.M_RIG, bc.PANEL + 1])
def test_affine_reproduction(hip_lib, M):
    """Deltas that are all equal move every point alike: the Jacobian's RBF part vanishes, sum_i G[v][a][i] = 0.  Deltas
    delta_i = c_i deform x by x: sum_i G[v][a][i] c_i[b] = f_v delta_ab."""
    c = _case("thin_plate", "linear", M, False)
    G, f = c["G"].astype(LD), np.where(c["out"], 0, c["fall"]).astype(LD)
    cen = c["rest"].astype(LD)
    extent = float(np.abs(c["rest"]).max())
    e1 = float(np.abs(G.sum(axis=2)).max())
    e2 = float(np.abs(np.einsum("vai,ib->vab", G, cen) - f[:, None, None] * np.eye(3, dtype=LD)[None]).max())
    print(f"affine M={M}: worst |sum_i G| = {e1:.3e}, worst |sum_i G c_i - f I| = {e2:.3e}, bar {1e-5 * extent:.3e}")
    assert e1 <= 1e-5 * extent and e2 <= 1e-5 * extent
