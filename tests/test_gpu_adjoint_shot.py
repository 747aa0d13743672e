"""GPU: fd_deform_adjoint_shot* -- grad_W[f] = Psi^T R_f, r_{f,v} = f_v Pi_v g_{f,v}, for the F cotangents of a shot in one
matrix-pipe launch per 32 frames (include/facedeform_hip.h states the contract).

Inputs, restatement (np.longdouble) and bars are tests/test_gpu_adjoint.py's: 3208 vertices, a gate that removes about a third,
every 97th vertex exactly on the radius; frame 0 of G is that file's G, the other frames are random normal fp32.

The bars:
  restatement  per frame and entry |grad_W[f] - ref_f| <= KAPPA 2^-53 S_{f,j}, KAPPA = 32 as in that file: phi is the same
               function on the same inputs, only the order of the fp64 additions differs, and any order of N additions stays
               inside (N - 1) 2^-53 S_j.  Measured on the MI355X over the cases of tests 1 and 4 (worst of F = 3 frames), with
               fd_deform_adjoint's ratio on the same frames in brackets: the worst is 4.72 (4.72) (multilayer 64 x 4,
               projection on; 2.83 (2.86) off; 4.25 (6.30) at 100 x 4); of the other kinds at 64 points Gaussian 1.46 (1.69),
               QNN 1.16 (1.71), thin-plate, biharmonic and cubic at most 0.42 (0.50); thin-plate over 12 ... 300 points at
               most 0.63 (0.80); QNN at 300 points 3.44 (3.51); N = 1 ... 513 at most 3.09 (N = 31, where a few vertices are
               the whole sum); F = 1 ... 33 at most 0.58; N = 262 653 with 16 points 0.13.  The shot launch is level with the
               single one or below it everywhere: the figure is phi's own rounding, not the order of the additions.
  independence frame f's block has the same bits from F = 1, from F = 5 (at another position) and from F = 33, in the host and
               device-pointer forms, and on every call.
  dual         |sum grad_W[f] W - sum_v g_{f,v} . D_v| <= 2e-7 sum_v |g_{f,v}|_2 |D_v|_2, that file's bar."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_adjoint as ta
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
KAPPA = ta.KAPPA
RADIUS2, RATE = ta.RADIUS2, ta.RATE
F_MAX = 33


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _G():
    """(33, N, 3) fp32: frame 0 is tests/test_gpu_adjoint.py's G.  Fewer frames are the first ones of these."""
    base = ta._inputs()[5]
    G = np.random.default_rng(211).standard_normal((F_MAX,) + base.shape).astype(np.float32)
    G[0] = base
    G.setflags(write=False)
    return G


def _refs(c, G, N=None):
    """Per frame (ref, S) of the restatement on the first N vertices: Psi and Pi are formed once, in longdouble."""
    P, tu, tv, nrm, dist2, _ = ta._inputs()
    n = P.shape[0] if N is None else N
    X = P[:n].astype(LD)
    Phi = np.concatenate([ta._phi(c["kind"], X, c["centres"].astype(LD), c["radii"]), np.ones((n, 1), LD), X], axis=1)
    Phi[:, c["centres"].shape[0] + c["rows"]:] = 0
    proj = c["kw"]["tangents"] is not None
    Pi = ta._projection(tu[:n], tv[:n], nrm[:n]) if proj else None
    f = c["fall"][:n].astype(LD)
    out = c["out"][:n]
    res = []
    for g in G:
        r = g[:n].astype(LD)
        if proj:
            r = np.einsum("bij,bj->bi", Pi, r)
        r = r * f[:, None]
        r[out] = 0
        res.append((Phi.T @ r, np.abs(Phi).T @ np.abs(r).max(axis=1)))
    return res


def _worst(got, refs):
    return max(ta._ratio(got[k], ref, S) for k, (ref, S) in enumerate(refs))


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, proj, M=ta.M_RIG, params=None, F=3):
    """tests/test_gpu_adjoint.py's case (model, fall-off, fp64 displacement) plus the shot call on F frames and fd_deform_adjoint
    on each of them."""
    c = dict(ta._case(kind_name, term, proj, M, params))
    kind, _ = ta.KINDS[kind_name]
    P = ta._inputs()[0]
    G = _G()[:F]
    e = ta._engine(kind, c["params"], ta.TERMS[term], c["rest"], synth.rig_deltas(c["rest"], 0))
    c["shot"] = e.deform_adjoint_shot(P, G, **c["kw"])
    c["single"] = np.stack([e.deform_adjoint(P, g, **c["kw"]) for g in G])
    e.close()
    c["G"] = G
    c["refs"] = _refs(c, G)
    return c


def _report(tag, c):
    shot, single = _worst(c["shot"], c["refs"]), _worst(c["single"], c["refs"])
    print(f"{tag}: worst |grad_W[f] - ref_f| / (2^-53 S) = {shot:.2f}  (fd_deform_adjoint on the same frames: {single:.2f})")
    return shot


# ---- 1: against the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", ta.CASES)
def test_against_the_restatement(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj)
    n = c["W"].shape[0]
    assert c["shot"].shape == (3, n, 3) and np.isfinite(c["shot"]).all()
    assert _report(f"restatement {kind_name}/{term} proj={proj}", c) <= KAPPA
    # rows of the polynomial term the model lacks: 0.0 exactly, in every frame
    lacking = c["shot"][:, n - 4 + c["rows"]:]
    assert np.array_equal(_bits(lacking), _bits(np.zeros_like(lacking)))


# ---- 2: frame independence, bit for bit --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,proj", [("thin_plate", True), ("qnn", False)])
def test_frame_independence(hip_lib, kind_name, proj):
    dev = torch.device("cuda", 0)
    c = _case(kind_name, "linear", proj)
    kind, _ = ta.KINDS[kind_name]
    P, tu, tv, nrm, dist2, _ = ta._inputs()
    G = _G()
    n = c["W"].shape[0]
    e = ta._engine(kind, c["params"], capi.TERM_LINEAR, c["rest"], synth.rig_deltas(c["rest"], 0))
    all33 = e.deform_adjoint_shot(P, G, **c["kw"])                       # two groups, the second with one frame
    assert all33.shape == (F_MAX, n, 3)
    assert np.array_equal(_bits(all33[:3]), _bits(c["shot"]))            # F = 3, another engine, another call
    order5 = [3, 32, 0, 7, 31]                                           # among other frames and at other positions
    five = e.deform_adjoint_shot(P, G[order5], **c["kw"])
    for k, f in enumerate(order5):
        assert np.array_equal(_bits(five[k]), _bits(all33[f])), f
    for f in (0, 3, 31, 32):
        alone = e.deform_adjoint_shot(P, G[f:f + 1], **c["kw"])
        assert np.array_equal(_bits(alone[0]), _bits(all33[f])), f
    # the device-pointer form, twice; rows beyond F (C + 4) stay untouched
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d_P, d_G, d_d2 = T(P), T(G), T(dist2)
    d_frames = [T(a) for a in (tu, tv, nrm)] if proj else []
    d_fr = [a.data_ptr() for a in d_frames] if proj else [0, 0, 0]
    d_out = torch.full((F_MAX * n + 5, 3), -7.25, dtype=torch.float64, device=dev)
    for _ in range(2):
        e.deform_adjoint_shot_dev(P.shape[0], F_MAX, d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr(), d_d2.data_ptr(), *d_fr,
                                  RADIUS2, RATE)
        e.synchronize()
        assert np.array_equal(_bits(d_out[:F_MAX * n].cpu().numpy().reshape(F_MAX, n, 3)), _bits(all33))
        assert (d_out[F_MAX * n:] == -7.25).all()
    # the context's weights are as they were
    assert np.array_equal(_bits(e.get_weights()[0]), _bits(c["W"]))
    e.close()


# ---- 3: out vertices and NaN containment ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", [("thin_plate", "linear", True), ("qnn", "const", False), ("biharmonic", "linear", False)])
def test_out_vertices_and_nan_containment(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj)
    P, _, _, _, dist2, _ = ta._inputs()
    out = c["out"]
    gated = dist2 > np.float32(RADIUS2)
    assert gated.any() and (out & ~gated).any()                       # gated vertices, and f = 0 vertices that are not gated
    kind, _ = ta.KINDS[kind_name]
    e = ta._engine(kind, c["params"], ta.TERMS[term], c["rest"], synth.rig_deltas(c["rest"], 0))
    G = np.array(_G()[:5])
    clean = e.deform_adjoint_shot(P, G, **c["kw"])
    assert np.array_equal(_bits(clean[:3]), _bits(c["shot"]))
    for fill in (np.nan, np.inf, 0.0):
        Gf = G.copy(); Gf[:, out] = fill
        got = e.deform_adjoint_shot(P, Gf, **c["kw"])
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(clean)), fill
    live = int(np.flatnonzero(~out)[17])
    Gn = G.copy(); Gn[2, live, 1] = np.nan
    got = e.deform_adjoint_shot(P, Gn, **c["kw"])
    e.close()
    assert not np.isfinite(got[2]).all()
    for f in (0, 1, 3, 4):
        assert np.array_equal(_bits(got[f]), _bits(clean[f])), f


# ---- 4: shapes ---------------------------------------------------------------------------------------------------------

def test_vertex_counts(hip_lib):
    """N around the 32-vertex chunk and the 128-vertex super-tile, and across several ranges; F = 2."""
    c = _case("thin_plate", "linear", True)
    P, tu, tv, nrm, dist2, _ = ta._inputs()
    kind, params = ta.KINDS["thin_plate"]
    G = _G()[:2]
    e = ta._engine(kind, params, capi.TERM_LINEAR, c["rest"], synth.rig_deltas(c["rest"], 0))
    for N in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513):
        got = e.deform_adjoint_shot(P[:N], G[:, :N], dist2=dist2[:N], tangents=(tu[:N], tv[:N], nrm[:N]), radius2=RADIUS2, falloffrate=RATE)
        ratio = _worst(got, _refs(c, G, N))
        print(f"N = {N}: worst ratio {ratio:.2f}")
        assert ratio <= KAPPA, N
    e.close()


def test_frame_counts(hip_lib):
    """3, 6, 15, 18, 33 and 96 columns -- below one column tile, across one, the full six -- and a second group of one frame;
    every frame against the restatement."""
    c = _case("thin_plate", "linear", True)
    P = ta._inputs()[0]
    kind, params = ta.KINDS["thin_plate"]
    G = _G()
    refs = _refs(c, G)
    e = ta._engine(kind, params, capi.TERM_LINEAR, c["rest"], synth.rig_deltas(c["rest"], 0))
    for F in (1, 2, 5, 6, 11, 32, 33):
        got = e.deform_adjoint_shot(P, G[:F], **c["kw"])
        assert got.shape[0] == F
        ratio = _worst(got, refs[:F])
        print(f"F = {F}: worst ratio {ratio:.2f}")
        assert ratio <= KAPPA, F
    e.close()


# C + 4 = 16, 17, 128, 129, 304: exactly one row tile, one row over, exactly one panel, one row over, three panels; QNN and the
# multilayer records' centre-major order
RECORD_CASES = [("thin_plate", M) for M in (12, 13, 124, 125, 300)] + [("qnn", 33), ("qnn", 300), ("multilayer", 64), ("multilayer", 100)]


@pytest.mark.parametrize("kind_name,M", RECORD_CASES)
def test_record_counts(hip_lib, kind_name, M):
    c = _case(kind_name, "linear", True, M)
    C = c["shot"].shape[1] - 4
    assert C == (M * 4 if kind_name == "multilayer" else M)
    assert _report(f"{kind_name} M = {M} ({C} records)", c) <= KAPPA


def test_several_super_tiles_per_range(hip_lib):
    """N = 262 653: 2052 super-tiles of 128 vertices, nine per range.  Thin-plate, 16 control points, gate and fall-off,
    no frames, F = 2; against the restatement (in chunks of vertices), and two calls give the same bits."""
    N = ta.N_LARGE
    kind, params = ta.KINDS["thin_plate"]
    rest = synth.control_points(16)
    P = synth.head_mesh(N)
    rng = np.random.default_rng(3)
    dist2 = (rng.random(N) * 1.5 * RADIUS2).astype(np.float32)
    G = rng.standard_normal((2,) + P.shape).astype(np.float32)
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    e = ta._engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    _, centres, radii = ta._model(e, rest)
    _, fall = e.deform(P, **kw)
    got = e.deform_adjoint_shot(P, G, **kw)
    again = e.deform_adjoint_shot(P, G, **kw)
    e.close()
    assert np.array_equal(_bits(got), _bits(again))
    for f in range(2):
        r, _ = ta._cotangent(G[f], fall, dist2, None)
        ref = np.zeros((20, 3), LD); S = np.zeros(20, LD)
        for a in range(0, N, 1 << 15):
            ref_a, S_a = ta._restatement(kind, P[a:a + (1 << 15)], r[a:a + (1 << 15)], centres, radii, 4)
            ref += ref_a; S += S_a
        ratio = ta._ratio(got[f], ref, S)
        print(f"N = {N}, frame {f}: worst ratio {ratio:.2f}")
        assert ratio <= KAPPA


# ---- 5: dual to the library's own forward map ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_dual_to_the_forward_map(hip_lib, kind_name):
    c = _case(kind_name, "linear", True)
    D = c["D"].astype(np.float64)
    for f in range(3):
        G = c["G"][f].astype(np.float64)
        lhs = float((c["shot"][f].astype(LD) * c["W"].astype(LD)).sum())
        rhs = float((G.astype(LD) * D.astype(LD)).sum())
        bar = 2e-7 * float((np.linalg.norm(G, axis=1) * np.linalg.norm(D, axis=1)).sum())
        print(f"dual {kind_name} frame {f}: <grad_W, W> = {lhs:.12e}, sum g.D = {rhs:.12e}, |diff| / bar = {abs(lhs - rhs) / bar:.3e}")
        assert bar > 0 and abs(lhs - rhs) <= bar


# ---- 6: model and argument edges -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name", ["thin_plate", "multilayer"])
def test_no_vertices_gives_zeros(hip_lib, kind_name):
    dev = torch.device("cuda", 0)
    kind, params = ta.KINDS[kind_name]
    rest = synth.control_points(ta.M_RIG)
    e = ta._engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    n = e.get_weights()[0].shape[0]
    got = e.deform_adjoint_shot(np.zeros((0, 3), np.float32), np.zeros((3, 0, 3), np.float32))
    assert got.shape == (3, n, 3) and np.array_equal(_bits(got), _bits(np.zeros_like(got)))
    d_out = torch.full((3 * n + 2, 3), -7.25, dtype=torch.float64, device=dev)
    d_any = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    e.deform_adjoint_shot_dev(0, 3, d_any.data_ptr(), d_any.data_ptr(), d_out.data_ptr())
    e.synchronize()
    assert (d_out[:3 * n] == 0).all() and (d_out[3 * n:] == -7.25).all()
    e.close()


def test_failed_build_gives_zeros(hip_lib):
    """Coincident control points: the build ends with -5 and is not repaired.  Enqueued right behind the build, whose status
    cannot be known yet, the launches see a model whose forward map is the identity: zeros and FD_OK.  Once the status is in,
    the call returns what fd_deform_dev returns."""
    dev = torch.device("cuda", 0)
    P = ta._inputs()[0]
    G = _G()[:3]
    rest = synth.control_points(ta.M_RIG)
    dup = rest.copy(); dup[17] = dup[40]
    e = capi.Engine(device=0)
    e.set_points(dup, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    N = P.shape[0]
    d_P = torch.from_numpy(P.copy()).to(dev); d_G = torch.from_numpy(G.copy()).to(dev)
    d_out = torch.full((3 * (ta.M_RIG + 4), 3), -7.25, dtype=torch.float64, device=dev)
    d_def = torch.empty_like(d_P)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.deform_adjoint_shot_dev(N, 3, d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert (d_out == 0).all()
    rc_adj = rc_of(lambda: e.deform_adjoint_shot_dev(N, 3, d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_P.data_ptr(), d_def.data_ptr()))
    assert rc_adj == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    assert rc_of(lambda: e.deform_adjoint_shot(P, G)) == rc_def
    e.close()


def test_not_built_and_bad_frames(hip_lib):
    P, tu, tv, _, _, _ = ta._inputs()
    G = np.array(_G()[:2])
    e = capi.Engine(device=0)
    rest = synth.control_points(ta.M_RIG)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    with pytest.raises(capi.FdError) as ei:
        e.deform_adjoint_shot(P, G)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    e.build()
    out = np.empty((2, ta.M_RIG + 4, 3), np.float64)
    ptr = capi._np_ptr
    rc = e.L.fd_deform_adjoint_shot(e.ctx, P.shape[0], 2, ptr(P), ptr(G), None, ptr(tu), ptr(tv), None, 1.0, 1.0, ptr(out))
    assert rc == capi.FD_E_INVALID                                    # the all-or-none rule for the frames
    # fd_set_output has no effect
    a = e.deform_adjoint_shot(P, G)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    b = e.deform_adjoint_shot(P, G)
    assert np.array_equal(_bits(a), _bits(b))
    e.close()
