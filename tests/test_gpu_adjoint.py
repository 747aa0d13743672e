"""GPU: fd_deform_adjoint* -- grad_W = sum_v phi_j(x_v) r_v, r_v = f_v Pi_v g_v, the exact transpose of the deformation in
the weights -- and fd_solve_operator, the map deltas -> weights (include/facedeform_hip.h states both contracts).

The yardstick is this file's own restatement in np.longdouble, built from the weights' layout (Engine.get_weights), the rest
rig, the radii the engine reports and the fall-off fd_deform reports.  Inputs are tests/test_gpu_invert.py's: 3000 head
vertices, 8 points on centres, 200 points off the surface, a gate that removes about a third, every 97th vertex exactly on the
radius (f = 0), frames on and off; G is random normal, fp32.

The bars:
  restatement  per entry |grad_W - ref| <= KAPPA 2^-53 S_j,  S_j = sum_v |phi_j(x_v)| |r_v|_inf  (the polynomial rows with
               1, x, y, z in phi's place).  KAPPA is four times the worst ratio measured on the MI355X over the cases of tests
               1, 4 and 5, rounded up to a power of two: measured 4.72 (multilayer, 64 x 4 records, projection on;
               at most 1.71 for the other kinds at 64 points, 3.51 for QNN at 300), asserted 32.
               It may not exceed N = 3208: any order of N fp64 additions stays inside (N - 1) 2^-53 S_j.
  dual         |sum grad_W W - sum_v g_v . D_v| <= 2e-7 sum_v |g_v|_2 |D_v|_2, D fd_deform's own fp64 displacement: the
               project's bar for that displacement (tests/test_gpu_invert.py), nothing else in the identity is larger.
  operator     max |S delta' - W'| / max |W'| <= 8 x the same ratio of the oracle's own builds + 3e-15."""
import functools

import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
KINDS = {
    "thin_plate": (capi.KERNEL_THIN_PLATE, []),
    "gaussian": (capi.KERNEL_GAUSSIAN, [0.35]),
    "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
    "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1]),
    "biharmonic": (capi.KERNEL_BIHARMONIC, []),
    "cubic": (capi.KERNEL_CUBIC, []),
}
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
TERM_ROWS = {"linear": 4, "const": 1, "zero": 0}
# linear for all kinds, const and zero for thin-plate and QNN
KIND_TERMS = [(k, "linear") for k in sorted(KINDS)] + [(k, t) for k in ("thin_plate", "qnn") for t in ("const", "zero")]
RADIUS2, RATE = 0.36, 1.7
M_RIG = 64
KAPPA = 32.0
N_FULL = 3208
assert KAPPA <= N_FULL


# ---- inputs --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _inputs():
    """3000 head vertices + the first 8 control points (x on a centre) + 200 mesh points scaled by 1.6 (off the surface);
    frames; a dist2 that gates about a third of the vertices, every 97th exactly on the radius (f = 0, not gated); G."""
    mesh = synth.head_mesh(3000)
    P = np.concatenate([mesh, synth.control_points(M_RIG)[:8], (mesh[:200] * np.float32(1.6))]).astype(np.float32)
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(5)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    G = np.random.default_rng(11).standard_normal(P.shape).astype(np.float32)
    for a in (P, tu, tv, nrm, dist2, G):
        a.setflags(write=False)
    assert P.shape[0] == N_FULL
    return P, tu, tv, nrm, dist2, G


def _engine(kind, params, term, rest, delta, check=True):
    e = capi.Engine(device=0)
    e.set_points(rest, delta)
    e.set_kernel(kind, params)
    e.set_term(term)
    e.build(check=check)
    return e


# ---- the restatement ---------------------------------------------------------------------------------------------

def _normalise(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def _projection(tu, tv, nrm):
    """Pi = a1 a1^T + a2 a2^T as project_to_tangents builds a1, a2, in longdouble."""
    u, v, n = (_normalise(a.astype(LD)) for a in (tu, tv, nrm))
    Gm = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = _normalise(np.einsum("bi,bij->bj", u, Gm)); a2 = _normalise(np.einsum("bi,bij->bj", v, Gm))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def _phi(kind, X, centres, radii):
    """phi_j(x_v) in the convention of fd_get_weights' W (the header's table), longdouble, (N, C)."""
    D = X[:, None, :] - centres[None]
    r2 = (D * D).sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == capi.KERNEL_THIN_PLATE:
            return np.where(r2 > 0, LD(0.5) * r2 * np.log(np.where(r2 > 0, r2, 1)), LD(0))
        if kind == capi.KERNEL_BIHARMONIC:
            return -np.sqrt(r2)
        if kind == capi.KERNEL_CUBIC:
            return r2 * np.sqrt(r2)
        return np.exp(-r2 / (radii.astype(LD)[None] ** 2))


def _cotangent(G, fall, dist2, frames):
    """r_v = f_v Pi_v g_v in longdouble, exactly 0 where the vertex is gated or f = 0; and which vertices those are."""
    r = G.astype(LD)
    if frames is not None:
        r = np.einsum("bij,bj->bi", _projection(*frames), r)
    f = fall.astype(LD)
    out = (dist2 > np.float32(RADIUS2)) | (fall == 0)
    r = r * f[:, None]
    r[out] = 0
    return r, out


def _restatement(kind, P, r, centres, radii, rows):
    """(ref, S): the (C + 4, 3) gradient and, per row, S_j = sum_v |phi_j(x_v)| |r_v|_inf; rows the term lacks are 0."""
    X = P.astype(LD)
    Phi = np.concatenate([_phi(kind, X, centres.astype(LD), radii), np.ones((X.shape[0], 1), LD), X], axis=1)
    C = centres.shape[0]
    Phi[:, C + rows:] = 0
    rinf = np.abs(r).max(axis=1)
    return Phi.T @ r, np.abs(Phi).T @ rinf


def _ratio(got, ref, S):
    """Worst |got - ref| / (2^-53 S_j) over the entries (0 where both sides and S are 0)."""
    err = np.abs(got.astype(LD) - ref)
    bar = (LD(2) ** -53 * S)[:, None] * np.ones((1, 3), LD)
    assert (err[bar == 0] == 0).all()
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0       # (N = 1: vertex 0 has f = 0)


def _model(e, rest):
    """(W, centres, radii) with centres in W's layout: the multilayer model's record l * M + c sits on centre c."""
    W, radii = e.get_weights()
    n = W.shape[0] - 4
    return W, np.tile(rest.astype(np.float64), (n // rest.shape[0], 1)), radii


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, proj, M=M_RIG, params=None):
    """One engine, the call under test on the full mesh and everything the restatement needs, computed once."""
    kind, kparams = KINDS[kind_name]
    kparams = kparams if params is None else list(params)
    P, tu, tv, nrm, dist2, G = _inputs()
    rest = synth.control_points(M)
    e = _engine(kind, kparams, TERMS[term], rest, synth.rig_deltas(rest, 0))
    W, centres, radii = _model(e, rest)
    frames = (tu, tv, nrm) if proj else None
    kw = dict(dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    e.set_eval_precision(capi.EVAL_FP64)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    D, fall = e.deform(P, **kw)
    e.set_output(capi.OUTPUT_POSITION)
    e.set_eval_precision(capi.EVAL_FP32)            # the adjoint is fp64 whatever the context says
    grad = e.deform_adjoint(P, G, **kw)
    e.close()
    r, out = _cotangent(G, fall, dist2, frames)
    ekind = capi.KERNEL_GAUSSIAN if kind in (capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_GAUSSIAN_ML) else kind
    return dict(kind=ekind, params=kparams, term=term, rest=rest, W=W, centres=centres, radii=radii, D=D, fall=fall, grad=grad,
                r=r, out=out, kw=kw, rows=TERM_ROWS[term])


def _case_ratio(c, N=None, got=None):
    P = _inputs()[0]
    n = P.shape[0] if N is None else N
    ref, S = _restatement(c["kind"], P[:n], c["r"][:n], c["centres"], c["radii"], c["rows"])
    return _ratio(c["grad"] if got is None else got, ref, S)


CASES = [(k, t, p) for k, t in KIND_TERMS for p in (False, True)]


# ---- 1: against the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", CASES)
def test_against_the_restatement(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj)
    assert c["grad"].shape == (c["W"].shape[0], 3) and np.isfinite(c["grad"]).all()
    ratio = _case_ratio(c)
    print(f"restatement {kind_name}/{term} proj={proj}: worst |grad_W - ref| / (2^-53 S_j) = {ratio:.2f}")
    assert ratio <= KAPPA


# ---- 2: dual to the library's own forward map --------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", CASES)
def test_dual_to_the_forward_map(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj)
    G = _inputs()[5].astype(np.float64)
    D = c["D"].astype(np.float64)
    lhs = float((c["grad"].astype(LD) * c["W"].astype(LD)).sum())
    rhs = float((G.astype(LD) * D.astype(LD)).sum())
    bar = 2e-7 * float((np.linalg.norm(G, axis=1) * np.linalg.norm(D, axis=1)).sum())
    print(f"dual {kind_name}/{term} proj={proj}: <grad_W, W> = {lhs:.12e}, sum g.D = {rhs:.12e}, |diff| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert bar > 0 and abs(lhs - rhs) <= bar


# ---- 3: exact zeros and selects ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", [("thin_plate", "linear", True), ("qnn", "const", False), ("biharmonic", "linear", False)])
def test_vertices_that_are_out_contribute_nothing(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj)
    P, _, _, _, dist2, G = _inputs()
    out = c["out"]
    gated = dist2 > np.float32(RADIUS2)
    assert gated.any() and (out & ~gated).any()                       # gated vertices, and f = 0 vertices that are not gated
    kind, _ = KINDS[kind_name]
    e = _engine(kind, c["params"], TERMS[term], c["rest"], synth.rig_deltas(c["rest"], 0))
    G_nan = G.copy(); G_nan[out] = np.nan
    G_inf = G.copy(); G_inf[out] = np.inf
    G_zero = G.copy(); G_zero[out] = 0
    got = [e.deform_adjoint(P, g, **c["kw"]) for g in (G_nan, G_inf, G_zero)]
    e.close()
    assert np.isfinite(got[0]).all()
    for g in got:
        assert np.array_equal(g.view(np.uint64), c["grad"].view(np.uint64))
    # rows of the polynomial term the model lacks: 0.0 exactly
    C = c["grad"].shape[0] - 4
    lacking = c["grad"][C + c["rows"]:]
    assert np.array_equal(lacking.view(np.uint64), np.zeros_like(lacking).view(np.uint64))
    assert (c["grad"][C:C + c["rows"]] != 0).all()


@pytest.mark.parametrize("kind_name", ["thin_plate", "biharmonic", "multilayer"])
def test_no_vertices_gives_zeros(hip_lib, kind_name):
    dev = torch.device("cuda", 0)
    kind, params = KINDS[kind_name]
    rest = synth.control_points(M_RIG)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    C = e.get_weights()[0].shape[0] - 4
    got = e.deform_adjoint(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert got.shape == (C + 4, 3) and np.array_equal(got.view(np.uint64), np.zeros_like(got).view(np.uint64))
    d_out = torch.full((C + 6, 3), -7.25, dtype=torch.float64, device=dev)
    d_any = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    e.deform_adjoint_dev(0, d_any.data_ptr(), d_any.data_ptr(), d_out.data_ptr())
    e.synchronize()
    assert (d_out[:C + 4] == 0).all() and (d_out[C + 4:] == -7.25).all()
    e.close()


def test_failed_build_gives_zeros(hip_lib):
    """Coincident control points: the build ends with -5 and is not repaired.  Enqueued right behind the build, whose status
    cannot be known yet, the launches see a model whose forward map is the identity: zeros and FD_OK.  Once the status is in,
    every call returns what fd_deform_dev returns."""
    dev = torch.device("cuda", 0)
    P, _, _, _, _, G = _inputs()
    rest = synth.control_points(M_RIG)
    dup = rest.copy(); dup[17] = dup[40]
    e = capi.Engine(device=0)
    e.set_points(dup, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    N = P.shape[0]
    d_P = torch.from_numpy(P.copy()).to(dev); d_G = torch.from_numpy(G.copy()).to(dev)
    d_out = torch.full((M_RIG + 4, 3), -7.25, dtype=torch.float64, device=dev)
    d_def = torch.empty_like(d_P)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.deform_adjoint_dev(N, d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert (d_out == 0).all()
    rc_adj = rc_of(lambda: e.deform_adjoint_dev(N, d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_P.data_ptr(), d_def.data_ptr()))
    assert rc_adj == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    assert rc_of(lambda: e.deform_adjoint(P, G)) == rc_of(lambda: e.deform(P)) == rc_def
    e.close()


def test_not_built_and_bad_frames(hip_lib):
    P, tu, tv, _, _, G = _inputs()
    e = capi.Engine(device=0)
    rest = synth.control_points(M_RIG)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    with pytest.raises(capi.FdError) as ei:
        e.deform_adjoint(P, G)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    e.build()
    out = np.empty((M_RIG + 4, 3), np.float64)
    ptr = capi._np_ptr
    rc = e.L.fd_deform_adjoint(e.ctx, P.shape[0], ptr(P), ptr(G), None, ptr(tu), ptr(tv), None, 1.0, 1.0, ptr(out))
    assert rc == capi.FD_E_INVALID                                    # the all-or-none rule for the frames
    # fd_set_output has no effect
    a = e.deform_adjoint(P, G)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    b = e.deform_adjoint(P, G)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    e.close()


# ---- 4: launch shapes ------------------------------------------------------------------------------------------------

def test_launch_shapes_and_determinism(hip_lib):
    """N around the 256-vertex tile, each against the restatement at that N; two calls agree; the host call and the
    device-pointer call agree; rows beyond C + 4 of an oversized output stay untouched."""
    dev = torch.device("cuda", 0)
    c = _case("thin_plate", "linear", True)
    P, tu, tv, nrm, dist2, G = _inputs()
    kind, params = KINDS["thin_plate"]
    e = _engine(kind, params, capi.TERM_LINEAR, c["rest"], synth.rig_deltas(c["rest"], 0))
    for N in (1, 255, 256, 257, 511, 513):
        got = e.deform_adjoint(P[:N], G[:N], dist2=dist2[:N], tangents=(tu[:N], tv[:N], nrm[:N]), radius2=RADIUS2, falloffrate=RATE)
        ratio = _case_ratio(c, N, got)
        print(f"N = {N}: worst ratio {ratio:.2f}")
        assert ratio <= KAPPA, N
    again = e.deform_adjoint(P, G, **c["kw"])
    assert np.array_equal(again.view(np.uint64), c["grad"].view(np.uint64))
    C = M_RIG
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_P, d_G, d_d2, d_tu, d_tv, d_nrm = (T(a) for a in (P, G, dist2, tu, tv, nrm))
    d_out = torch.full((C + 4 + 5, 3), -7.25, dtype=torch.float64, device=dev)
    for _ in range(2):
        e.deform_adjoint_dev(P.shape[0], d_P.data_ptr(), d_G.data_ptr(), d_out.data_ptr(), d_d2.data_ptr(), d_tu.data_ptr(),
                             d_tv.data_ptr(), d_nrm.data_ptr(), RADIUS2, RATE)
        e.synchronize()
        assert np.array_equal(d_out[:C + 4].cpu().numpy().view(np.uint64), c["grad"].view(np.uint64))
        assert (d_out[C + 4:] == -7.25).all()
    e.close()


N_LARGE = 1026 * 256 - 3


def test_more_tiles_than_workgroups(hip_lib):
    """N = 262 653: 1026 tiles, so a workgroup walks two tiles and the second launch adds 33 blocks per part -- the sizes at
    which both launches take their other path.  Thin-plate, 16 control points, gate and fall-off, no frames; against the
    restatement (in chunks of vertices) with the bar of test 1, and two calls give the same bits."""
    kind, params = KINDS["thin_plate"]
    rest = synth.control_points(16)
    P = synth.head_mesh(N_LARGE)
    rng = np.random.default_rng(3)
    dist2 = (rng.random(N_LARGE) * 1.5 * RADIUS2).astype(np.float32)
    G = rng.standard_normal(P.shape).astype(np.float32)
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    _, centres, radii = _model(e, rest)
    _, fall = e.deform(P, **kw)
    got = e.deform_adjoint(P, G, **kw)
    again = e.deform_adjoint(P, G, **kw)
    e.close()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    r, _ = _cotangent(G, fall, dist2, None)
    ref = np.zeros((20, 3), LD); S = np.zeros(20, LD)
    for a in range(0, N_LARGE, 1 << 15):
        ref_a, S_a = _restatement(kind, P[a:a + (1 << 15)], r[a:a + (1 << 15)], centres, radii, 4)
        ref += ref_a; S += S_a
    ratio = _ratio(got, ref, S)
    print(f"N = {N_LARGE}: worst ratio {ratio:.2f}")
    assert ratio <= KAPPA


# ---- 5: record counts --------------------------------------------------------------------------------------------------

# Mpad > M (16 | Mpad); a full workgroup of centres; a second centre per lane; a second row of workgroups (M > 512)
RECORD_CASES = [("thin_plate", M, None) for M in (16, 33, 49, 256, 300, 520)] + [("qnn", 33, None), ("qnn", 300, None)] + \
               [("multilayer", 64, None), ("multilayer", 100, None)]


@pytest.mark.parametrize("kind_name,M,params", RECORD_CASES)
def test_record_counts(hip_lib, kind_name, M, params):
    c = _case(kind_name, "linear", True, M, params)
    C = c["grad"].shape[0] - 4
    assert C == (M * 4 if kind_name == "multilayer" else M)
    ratio = _case_ratio(c)
    print(f"{kind_name} M = {M} ({C} records): worst ratio {ratio:.2f}")
    assert ratio <= KAPPA


# ---- 6: fd_solve_operator ----------------------------------------------------------------------------------------------

M_OP = 33
OP_CASES = {"thin_plate": (capi.KERNEL_THIN_PLATE, []), "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
            "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 2, 0.1])}


def _oracle_build(oracle, kind_name, rest, delta):
    from oracle import fd_oracle as fo
    table = oracle.control_table(rest, (rest.astype(np.float64) + delta.astype(np.float64)).astype(np.float32))
    table[:, 3:6] = delta.astype(np.float64)              # the deltas themselves, not a difference of rounded positions
    if kind_name == "multilayer":
        tt, _, W, _ = oracle.build_multilayer(table, 0.7, 2, 0.1, fo.TERM_LINEAR)
    else:
        ko = fo.KERNEL_THIN_PLATE if kind_name == "thin_plate" else fo.KERNEL_GAUSSIAN_QNN
        _, tt, W, _ = oracle.build(table, ko, OP_CASES[kind_name][1], fo.TERM_LINEAR)
    assert tt == 1
    return W


@functools.lru_cache(maxsize=None)
def _oracle_ratio(oracle, kind_name):
    """max |S delta' - W'| / max |W'| from the oracle alone: its builds on unit deltas against its build on delta'."""
    rest = synth.control_points(M_OP)
    delta = _op_delta()
    W = _oracle_build(oracle, kind_name, rest, delta)
    S = np.zeros((W.shape[0], M_OP))
    for k in range((M_OP + 2) // 3):
        unit = np.zeros((M_OP, 3), np.float32)
        for a in range(3):
            if 3 * k + a < M_OP:
                unit[3 * k + a, a] = 1
        Wk = _oracle_build(oracle, kind_name, rest, unit)
        for a in range(3):
            if 3 * k + a < M_OP:
                S[:, 3 * k + a] = Wk[:, a]
    return float(np.abs(S @ delta.astype(np.float64) - W).max() / np.abs(W).max())


def _op_delta():
    return (0.05 * np.random.default_rng(23).standard_normal((M_OP, 3))).astype(np.float32)


@pytest.mark.parametrize("kind_name", sorted(OP_CASES))
def test_solve_operator(hip_lib, oracle, kind_name):
    kind, params = OP_CASES[kind_name]
    P, tu, tv, nrm, dist2, G = _inputs()
    rest = synth.control_points(M_OP)
    delta0 = synth.rig_deltas(rest, 0)
    delta = _op_delta()
    kw = dict(dist2=dist2, tangents=(tu, tv, nrm), radius2=RADIUS2, falloffrate=RATE)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, delta0)
    reuse = kind != capi.KERNEL_GAUSSIAN_ML                 # the multilayer model keeps no factorisation for fd_set_deltas
    W0, _ = e.get_weights()
    S = e.solve_operator()
    assert S.shape == (W0.shape[0], M_OP) and np.isfinite(S).all()
    # (b) the context is as it was: the same weights bit for bit, and fd_set_deltas goes on reusing the factorisation
    W0_after, _ = e.get_weights()
    assert np.array_equal(W0.view(np.uint64), W0_after.view(np.uint64))
    twin = _engine(kind, params, capi.TERM_LINEAR, rest, delta0)          # the same steps without the call in between
    for eng in (e, twin):
        if reuse:
            eng.set_deltas(delta)
        else:
            with pytest.raises(capi.FdError) as ei:
                eng.set_deltas(delta)
            assert ei.value.code == capi.FD_E_NOT_BUILT
            eng.set_points(rest, delta)
        eng.build()
    W1, _ = e.get_weights()
    W1_twin, _ = twin.get_weights()
    twin.close()
    assert np.array_equal(W1.view(np.uint64), W1_twin.view(np.uint64))
    # (a) S delta' against the weights the same context builds for delta'
    dW = np.abs(S @ delta.astype(np.float64) - W1)
    ours = float(dW.max() / np.abs(W1).max())
    theirs = _oracle_ratio(oracle, kind_name)
    print(f"operator {kind_name}: max |S delta' - W'| / max |W'| = {ours:.3e}; the oracle's own: {theirs:.3e}")
    assert ours <= 8 * theirs + 3e-15
    # (c) end to end: <S^T grad_W, delta'> against sum_v g_v . D_v(delta')
    grad = e.deform_adjoint(P, G, **kw)
    e.set_eval_precision(capi.EVAL_FP64)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    D, _ = e.deform(P, **kw)
    e.close()
    lhs = float(((S.T @ grad).astype(LD) * delta.astype(LD)).sum())
    G64 = G.astype(np.float64); D64 = D.astype(np.float64)
    rhs = float((G64.astype(LD) * D64.astype(LD)).sum())
    bar = 2e-7 * float((np.linalg.norm(G64, axis=1) * np.linalg.norm(D64, axis=1)).sum()) + float((np.abs(grad) * dW).sum())
    print(f"operator {kind_name} end to end: {lhs:.12e} against {rhs:.12e}, |diff| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert abs(lhs - rhs) <= bar
