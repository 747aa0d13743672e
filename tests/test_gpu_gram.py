"""GPU: fd_deform_gram* -- H[q][j][k] = sum_v omega_v f_v^2 (Pi_v^2)[b][c] Psi_vj Psi_vk, the Gram matrix of the deformation
in the weights (include/facedeform_hip.h states the contract).

The yardstick is this file's own restatement in np.longdouble, built from the weights' layout (Engine.get_weights), the rest
rig, the radii the engine reports and the fall-off fd_deform reports; never the call's own output.  Inputs are
tests/test_gpu_adjoint.py's recipe: 3000 head vertices, 8 points on centres, 200 points off the surface, a gate that removes
about a third, every 97th vertex exactly on the radius (f = 0), frames on and off, M = 64 (the multilayer model with 2 layers
there, with 4 in the record-count cases); omega, where given, is random in (0, 2) with a tenth exactly 0.

The bars:
  restatement  per entry |H - ref| <= KAPPA 2^-53 sum_v |q_v| |Psi_vj| |Psi_vk|.  KAPPA is four times the worst ratio measured
               on the MI355X over the cases of this file, rounded up to a power of two, per family of kinds -- a stricter
               reading of the rule than one figure for all:
                 thin-plate, biharmonic, cubic   measured 88.24 (thin-plate, 64 points, N = 4 and 5, projection on; 57.91
                                                 without; at most 23.17 from N = 31 on, 12.16 from N = 255 on, 9.53 over the
                                                 record counts at N = 777, 9.31 at N = 262 653), asserted 512;
                 the Gaussian kinds              measured 1051.75 (multilayer, 100 x 4 records, N = 777; 934.55 at 64 x 4;
                                                 278.10 for QNN at 300 points, 35.86 at 64; 29.11 for the plain Gaussian and
                                                 for the multilayer model with 2 layers at N = 3208), asserted 8192.
               What is measured is not the summation (the polyharmonic kinds stay near 10 once a few hundred vertices share
               an entry, at a quarter of a million as at 255) but the conditioning of phi in its fp64
               argument, which the operator squares: exp(x) carries |x| ulps of the rounding of x = -d2 / R^2, and an entry
               between two narrow, distant records is made of terms with |x| in the hundreds only (values around 1e-100, still
               held to a relative 1e-13); log d2 near d2 = 1 loses the same way, which shows where four vertices are the whole sum.
  dual         |sum W'^T H W'' - sum_v omega_v D'_v . D''_v| <= 2e-7 sum_v omega_v |D'_v| |D''_v|, D fd_deform's own fp64
               displacement, stored in fp32: tests/test_gpu_adjoint.py's bar."""
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
    "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 2, 0.1]),
    "biharmonic": (capi.KERNEL_BIHARMONIC, []),
    "cubic": (capi.KERNEL_CUBIC, []),
}
KINDS_ALL = dict(KINDS, multilayer4=(capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1]))      # four layers: the record-count cases
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
TERM_ROWS = {"linear": 4, "const": 1, "zero": 0}
KIND_TERMS = [(k, "linear") for k in sorted(KINDS)] + [(k, t) for k in ("thin_plate", "qnn") for t in ("const", "zero")]
RADIUS2, RATE = 0.36, 1.7
M_RIG = 64
KAPPA = {"thin_plate": 512.0, "biharmonic": 512.0, "cubic": 512.0, "gaussian": 8192.0, "qnn": 8192.0, "multilayer": 8192.0, "multilayer4": 8192.0}
N_FULL = 3208
N_SHAPE = 777                 # the record-count cases: three full super-tiles of 256 vertices and a part, four vertex ranges
QMAP = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
# the launch's constants (fd_gram.hip): MFMA depth 4, staging chunk 32, super-tile = least vertices per range 256
CHUNK, SUPER = 32, 256


# ---- inputs --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _inputs():
    mesh = synth.head_mesh(3000)
    P = np.concatenate([mesh, synth.control_points(M_RIG)[:8], (mesh[:200] * np.float32(1.6))]).astype(np.float32)
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(5)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    orng = np.random.default_rng(17)
    omega = (2 * orng.random(P.shape[0])).astype(np.float32)
    omega[orng.random(P.shape[0]) < 0.1] = 0
    for a in (P, tu, tv, nrm, dist2, omega):
        a.setflags(write=False)
    assert P.shape[0] == N_FULL and (omega == 0).sum() > 200
    return P, tu, tv, nrm, dist2, omega


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


def _psi(kind, P, centres, radii, rows):
    """Psi, (N, C + 4) longdouble: phi in W's convention, then 1, x, y, z; columns the term lacks are 0."""
    X = P.astype(LD)
    Psi = np.concatenate([_phi(kind, X, centres.astype(LD), radii), np.ones((X.shape[0], 1), LD), X], axis=1)
    Psi[:, centres.shape[0] + rows:] = 0
    return Psi


def _weights(fall, dist2, omega, frames):
    """q, (N, nq) longdouble: omega f^2 (Pi^2)[b][c], exactly 0 where the vertex is gated, f = 0 or omega = 0; and which those are."""
    f = fall.astype(LD)
    w = np.ones_like(f) if omega is None else omega.astype(LD)
    out = (dist2 > np.float32(RADIUS2)) | (fall == 0) | (w == 0)
    q = (w * f * f)[:, None]
    if frames is not None:
        Pi = _projection(*frames)
        Pi2 = np.einsum("vbk,vkc->vbc", Pi, Pi)
        q = q * np.stack([Pi2[:, b, c] for b, c in QMAP], axis=1)
    q = np.where(out[:, None], LD(0), q)
    return q, out


def _restatement(Psi, q):
    """(ref, S): (nq, n, n) each -- the Gram matrices and, per entry, sum_v |q_v| |Psi_vj| |Psi_vk|."""
    A = np.abs(Psi)
    ref = np.stack([(Psi * q[:, k:k + 1]).T @ Psi for k in range(q.shape[1])])
    S = np.stack([(A * np.abs(q[:, k:k + 1])).T @ A for k in range(q.shape[1])])
    return ref, S


def _ratio(got, ref, S):
    """Worst |got - ref| / (2^-53 S) over the entries (entries with S = 0 must be exact zeros on both sides)."""
    assert got.shape == ref.shape
    err = np.abs(got.astype(LD) - ref)
    bar = LD(2) ** -53 * S
    assert (err[bar == 0] == 0).all()
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def _model(e, rest):
    """(W, centres, radii) with centres in W's layout: the multilayer model's record l * M + c sits on centre c."""
    W, radii = e.get_weights()
    n = W.shape[0] - 4
    return W, np.tile(rest.astype(np.float64), (n // rest.shape[0], 1)), radii


def _ekind(kind):
    return capi.KERNEL_GAUSSIAN if kind in (capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_GAUSSIAN_ML) else kind


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, proj, use_omega=False, M=M_RIG, N=N_FULL):
    """One engine, the call under test on the first N vertices and everything the restatement needs, computed once."""
    kind, kparams = KINDS_ALL[kind_name]
    P, tu, tv, nrm, dist2, omega = (a[:N] for a in _inputs())
    rest = synth.control_points(M)
    e = _engine(kind, kparams, TERMS[term], rest, synth.rig_deltas(rest, 0))
    W, centres, radii = _model(e, rest)
    frames = (tu, tv, nrm) if proj else None
    kw = dict(dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    _, fall = e.deform(P, **kw)
    e.set_eval_precision(capi.EVAL_FP32)            # the Gram operator is fp64 whatever the context says
    om = omega if use_omega else None
    H = e.deform_gram(P, omega=om, **kw)
    e.close()
    Psi = _psi(_ekind(kind), P, centres, radii, TERM_ROWS[term])
    q, out = _weights(fall, dist2, om, frames)
    return dict(kind_name=kind_name, term=term, rest=rest, W=W, H=H, Psi=Psi, q=q, out=out, kw=kw, omega=om, rows=TERM_ROWS[term],
                fall=fall)


def _case_ratio(c, N=None, got=None):
    n = c["Psi"].shape[0] if N is None else N
    ref, S = _restatement(c["Psi"][:n], c["q"][:n])
    return _ratio(c["H"] if got is None else got, ref, S)


CASES = [(k, t, p, False) for k, t in KIND_TERMS for p in (False, True)] + \
        [("thin_plate", "linear", False, True), ("thin_plate", "linear", True, True), ("multilayer", "linear", True, True)]


# ---- 1: against the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj,use_omega", CASES)
def test_against_the_restatement(hip_lib, kind_name, term, proj, use_omega):
    c = _case(kind_name, term, proj, use_omega)
    n = c["W"].shape[0]
    assert c["H"].shape == (6 if proj else 1, n, n) and np.isfinite(c["H"]).all()
    ratio = _case_ratio(c)
    print(f"restatement {kind_name}/{term} proj={proj} omega={use_omega}: worst |H - ref| / (2^-53 S) = {ratio:.2f}")
    assert ratio <= KAPPA[kind_name]


# ---- 2: symmetry, definiteness, the rows the term lacks -----------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj,use_omega", CASES)
def test_symmetry_and_definiteness(hip_lib, kind_name, term, proj, use_omega):
    c = _case(kind_name, term, proj, use_omega)
    H = c["H"]
    for q in range(H.shape[0]):
        assert np.array_equal(H[q].view(np.uint64), np.ascontiguousarray(H[q].T).view(np.uint64))      # bit for bit
    for q in ((0, 3, 5) if proj else (0,)):                      # xx, yy, zz: sums of squares with weights >= 0
        assert (np.diagonal(H[q]) >= 0).all()
    C = H.shape[1] - 4
    lacking = np.concatenate([H[:, C + c["rows"]:, :].ravel(), H[:, :, C + c["rows"]:].ravel()])
    assert np.array_equal(lacking.view(np.uint64), np.zeros_like(lacking).view(np.uint64))
    assert (np.diagonal(H[0])[:C + c["rows"]] > 0).all()


# ---- 3: dual to the library's own forward map --------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj,use_omega", CASES)
def test_dual_to_the_forward_map(hip_lib, kind_name, term, proj, use_omega):
    c = _case(kind_name, term, proj, use_omega)
    kind, kparams = KINDS[kind_name]
    P = _inputs()[0]
    Ws, Ds = [], []
    for seed in (41, 42):
        delta = (0.05 * np.random.default_rng(seed).standard_normal(c["rest"].shape)).astype(np.float32)
        e = _engine(kind, kparams, TERMS[term], c["rest"], delta)
        Ws.append(e.get_weights()[0].astype(LD))
        e.set_eval_precision(capi.EVAL_FP64)
        e.set_output(capi.OUTPUT_DISPLACEMENT)
        Ds.append(e.deform(P, **c["kw"])[0].astype(np.float64))
        e.close()
    H = c["H"].astype(LD)
    lhs = LD(0)
    for b in range(3):
        for cc in range(3):
            if not proj and b != cc:
                continue
            q = QMAP.index((min(b, cc), max(b, cc))) if proj else 0
            lhs += Ws[0][:, b] @ (H[q] @ Ws[1][:, cc])
    w = np.ones(P.shape[0]) if c["omega"] is None else c["omega"].astype(np.float64)
    rhs = float((w.astype(LD) * (Ds[0].astype(LD) * Ds[1].astype(LD)).sum(axis=1)).sum())
    bar = 2e-7 * float((w * np.linalg.norm(Ds[0], axis=1) * np.linalg.norm(Ds[1], axis=1)).sum())
    print(f"dual {kind_name}/{term} proj={proj} omega={use_omega}: W'HW'' = {float(lhs):.12e}, sum w D'.D'' = {rhs:.12e}, "
          f"|diff| / bar = {abs(float(lhs) - rhs) / bar:.3e}")
    assert bar > 0 and abs(float(lhs) - rhs) <= bar


# ---- 4: exact zeros and selects ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,proj", [("thin_plate", "linear", True), ("qnn", "const", False), ("biharmonic", "linear", False)])
def test_vertices_that_are_out_contribute_nothing(hip_lib, kind_name, term, proj):
    c = _case(kind_name, term, proj, True)
    P, _, _, _, dist2, omega = _inputs()
    gated = dist2 > np.float32(RADIUS2)
    f0 = (c["fall"] == 0) & ~gated
    w0 = omega == 0
    assert gated.any() and f0.any() and (w0 & ~gated & ~f0).any()
    kind, kparams = KINDS[kind_name]
    e = _engine(kind, kparams, TERMS[term], c["rest"], synth.rig_deltas(c["rest"], 0))
    P_nan = P.copy(); P_nan[gated | w0 | f0] = np.nan               # P is not read where the vertex is out
    w_nan = omega.copy(); w_nan[gated | f0] = np.nan               # omega neither, where the gate or f = 0 put it out
    w_inf = omega.copy(); w_inf[gated | f0] = np.inf
    got = [e.deform_gram(p, omega=w, **c["kw"]) for p, w in ((P_nan, omega), (P, w_nan), (P_nan, w_inf))]
    e.close()
    assert np.isfinite(got[0]).all()
    for g in got:
        assert np.array_equal(g.view(np.uint64), c["H"].view(np.uint64))


@pytest.mark.parametrize("kind_name", ["thin_plate", "multilayer"])
def test_no_vertices_gives_zeros(hip_lib, kind_name):
    dev = torch.device("cuda", 0)
    kind, params = KINDS[kind_name]
    rest = synth.control_points(M_RIG)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    n = e.get_weights()[0].shape[0]
    none = np.zeros((0, 3), np.float32)
    for frames, nq in ((None, 1), ((none, none, none), 6)):
        got = e.deform_gram(none, tangents=frames)
        assert got.shape == (nq, n, n) and np.array_equal(got.view(np.uint64), np.zeros_like(got).view(np.uint64))
    d_out = torch.full((n * n + 7,), -7.25, dtype=torch.float64, device=dev)
    d_any = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    e.deform_gram_dev(0, d_any.data_ptr(), d_out.data_ptr())
    e.synchronize()
    assert (d_out[:n * n] == 0).all() and (d_out[n * n:] == -7.25).all()
    e.close()


def test_failed_build_gives_zeros(hip_lib):
    """Coincident control points: the build ends with -5 and is not repaired.  Enqueued right behind the build, whose status
    cannot be known yet, the launches see a model whose forward map is the identity: zeros and FD_OK.  Once the status is in,
    every call returns what fd_deform_dev returns."""
    dev = torch.device("cuda", 0)
    P = _inputs()[0]
    rest = synth.control_points(M_RIG)
    dup = rest.copy(); dup[17] = dup[40]
    e = capi.Engine(device=0)
    e.set_points(dup, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    N, n = P.shape[0], M_RIG + 4
    d_P = torch.from_numpy(P.copy()).to(dev)
    d_out = torch.full((n, n), -7.25, dtype=torch.float64, device=dev)
    d_def = torch.empty_like(d_P)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.deform_gram_dev(N, d_P.data_ptr(), d_out.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert (d_out == 0).all()
    rc_gram = rc_of(lambda: e.deform_gram_dev(N, d_P.data_ptr(), d_out.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_P.data_ptr(), d_def.data_ptr()))
    assert rc_gram == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    assert rc_of(lambda: e.deform_gram(P)) == rc_of(lambda: e.deform(P)) == rc_def
    e.close()


def test_not_built_and_bad_frames(hip_lib):
    P, tu, tv, _, _, _ = _inputs()
    e = capi.Engine(device=0)
    rest = synth.control_points(M_RIG)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    with pytest.raises(capi.FdError) as ei:
        e.deform_gram(P)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    e.build()
    n = M_RIG + 4
    out = np.empty((6, n, n), np.float64)
    ptr = capi._np_ptr
    rc = e.L.fd_deform_gram(e.ctx, P.shape[0], ptr(P), None, None, ptr(tu), ptr(tv), None, 1.0, 1.0, ptr(out))
    assert rc == capi.FD_E_INVALID                                    # the all-or-none rule for the frames
    a = e.deform_gram(P)
    e.set_output(capi.OUTPUT_DISPLACEMENT)                            # fd_set_output has no effect
    b = e.deform_gram(P)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    e.close()


# ---- 5: launch shapes and determinism --------------------------------------------------------------------------------

@pytest.mark.parametrize("proj", [False, True])
def test_launch_shapes_and_determinism(hip_lib, proj):
    """N around the MFMA depth, the staging chunk and the vertices per range, each against the restatement at that N; two
    calls agree; the host call and the device-pointer call agree; entries beyond nq (C + 4)^2 of an oversized output stay
    untouched."""
    dev = torch.device("cuda", 0)
    c = _case("thin_plate", "linear", proj, True)
    P, tu, tv, nrm, dist2, omega = _inputs()
    kind, params = KINDS["thin_plate"]
    e = _engine(kind, params, capi.TERM_LINEAR, c["rest"], synth.rig_deltas(c["rest"], 0))
    for N in (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, SUPER - 1, SUPER, SUPER + 1, 2 * SUPER + 1):
        frames = (tu[:N], tv[:N], nrm[:N]) if proj else None
        got = e.deform_gram(P[:N], omega=omega[:N], dist2=dist2[:N], tangents=frames, radius2=RADIUS2, falloffrate=RATE)
        ratio = _case_ratio(c, N, got)
        print(f"N = {N} proj={proj}: worst ratio {ratio:.2f}")
        assert ratio <= KAPPA["thin_plate"], N
    again = e.deform_gram(P, omega=omega, **c["kw"])
    assert np.array_equal(again.view(np.uint64), c["H"].view(np.uint64))
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_P, d_w, d_d2, d_tu, d_tv, d_nrm = (T(a) for a in (P, omega, dist2, tu, tv, nrm))
    size = c["H"].size
    d_out = torch.full((size + 11,), -7.25, dtype=torch.float64, device=dev)
    fr = (d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr()) if proj else (0, 0, 0)
    for _ in range(2):
        e.deform_gram_dev(P.shape[0], d_P.data_ptr(), d_out.data_ptr(), d_w.data_ptr(), d_d2.data_ptr(), *fr, RADIUS2, RATE)
        e.synchronize()
        assert np.array_equal(d_out[:size].cpu().numpy().view(np.uint64), c["H"].ravel().view(np.uint64))
        assert (d_out[size:] == -7.25).all()
    e.close()


N_LARGE = 1026 * 256 - 3


def test_ranges_of_several_chunks(hip_lib):
    """N = 262 653 with 16 control points: 206 ranges of five super-tiles (40 chunks) each, and the second launch adds 206 blocks
    per entry.  Thin-plate, gate, fall-off and omega, no frames; against the restatement (in chunks of vertices) with the bar
    of test 1, and two calls give the same bits."""
    kind, params = KINDS["thin_plate"]
    rest = synth.control_points(16)
    P = synth.head_mesh(N_LARGE)
    rng = np.random.default_rng(3)
    dist2 = (rng.random(N_LARGE) * 1.5 * RADIUS2).astype(np.float32)
    omega = (2 * rng.random(N_LARGE)).astype(np.float32)
    omega[rng.random(N_LARGE) < 0.1] = 0
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    _, centres, radii = _model(e, rest)
    _, fall = e.deform(P, **kw)
    got = e.deform_gram(P, omega=omega, **kw)
    again = e.deform_gram(P, omega=omega, **kw)
    e.close()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    q, _ = _weights(fall, dist2, omega, None)
    ref = np.zeros((1, 20, 20), LD); S = np.zeros((1, 20, 20), LD)
    for a in range(0, N_LARGE, 1 << 15):
        Psi = _psi(kind, P[a:a + (1 << 15)], centres, radii, 4)
        ref_a, S_a = _restatement(Psi, q[a:a + (1 << 15)])
        ref += ref_a; S += S_a
    ratio = _ratio(got, ref, S)
    print(f"N = {N_LARGE}: worst ratio {ratio:.2f}")
    assert ratio <= KAPPA["thin_plate"]


# ---- 6: record counts --------------------------------------------------------------------------------------------------

# C + 4 = 16, 17, 32, 33 (tile edges), 68, 256, 257 (a second panel of 128), 304, 524 (five panels: fifteen panel pairs);
# projection on where C + 4 <= 68, so that the longdouble restatement stays within seconds
RECORD_CASES = [("thin_plate", M) for M in (12, 13, 28, 29, 64, 252, 253, 300, 520)] + [("qnn", 33), ("qnn", 300)] + \
               [("multilayer4", 64), ("multilayer4", 100)]


@pytest.mark.parametrize("kind_name,M", RECORD_CASES)
def test_record_counts(hip_lib, kind_name, M):
    C = M * 4 if kind_name == "multilayer4" else M
    proj = C + 4 <= 68
    c = _case(kind_name, "linear", proj, True, M, N_SHAPE)
    assert c["H"].shape == (6 if proj else 1, C + 4, C + 4)
    ratio = _case_ratio(c)
    print(f"{kind_name} M = {M} ({C} records) proj={proj}: worst ratio {ratio:.2f}")
    assert ratio <= KAPPA[kind_name]
    for q in range(c["H"].shape[0]):
        assert np.array_equal(c["H"][q].view(np.uint64), np.ascontiguousarray(c["H"][q].T).view(np.uint64))
