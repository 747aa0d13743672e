"""GPU: fd_fit_deltas -- the deltas that minimise E(delta) = sum_v omega_v |D_v(S delta) - (T_v - P_v)|^2 + mu |delta - delta0|^2
(include/facedeform_hip.h states the contract).

The yardstick is this file's own float64 restatement of the normal system (NN, b): the dense 3N x 3M matrix
A[(v, b), (i, c)] = f_v Pi_v[b][c] (Psi_v S)[i] built from the restated Psi (tests/test_gpu_gram.py's, from fd_get_weights'
layout, the rest rig, the reported radii and the fall-off fd_deform reports) and S from fd_solve_operator;
NN = A^T diag(omega) A + mu I, b = A^T (omega t) + mu delta0.  omega takes the values 0, 0.5, 1, 2, so that the fp32 product
omega_v (T_v - P_v) the call forms is exact and the restatement needs no rounding of its own.  Mesh, gate and f = 0 vertices
are tests/test_gpu_adjoint.py's recipe; mu = 1e-8 sum_v omega_v.

The bars:
  optimality   |NN delta_fit - b|_2 <= KAPPA2 2^-53 (|NN|_2 |delta_fit|_2 + |b|_2).  KAPPA2 is four times the worst ratio
               measured on the MI355X over the cases below, rounded up to a power of two, per kind (stricter than one figure):
                 thin-plate  measured 14150.33 (64 points, no projection; 3035.83 with; 1313.00 and 484.11 at 33), asserted 65536;
                 multilayer  measured 489.52 (64 points, no projection; 224.31 with; 41.96 and 20.79 at 33), asserted 2048;
                 QNN         measured 7.83 (64 points, no projection; at least 5.23), asserted 32.
               The figure is the price of composing the system in weight space: S^T H S cancels from entries of S that are
               far larger than the cardinal functions Psi S the restatement forms directly (thin-plate most of all), so H's
               own rounding, 2^-53 of sum |q| |Psi| |Psi|, returns multiplied by |S|^T . |S|.
  energy       E(delta_fit) <= E(delta_lstsq) (1 + 1e-10), E by the restatement; the reported E_fit and E0 agree with the
               restated ones within the same 1e-10.
  planted      after fd_set_deltas(fp32(delta_fit)) + build, fd_deform in fp64 lies within conftest.l2_parity_ulp <= 1 of the
               targets."""
import functools

import numpy as np
import pytest

from conftest import l2_parity_ulp
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
KINDS = {
    "thin_plate": (capi.KERNEL_THIN_PLATE, []),
    "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
    "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 2, 0.1]),
}
RADIUS2, RATE = 0.36, 1.7
KAPPA2 = {"thin_plate": 65536.0, "multilayer": 2048.0, "qnn": 32.0}
N_FULL = 3208
CASES = [(k, M, p) for k in sorted(KINDS) for M in (33, 64) for p in (False, True)]


@functools.lru_cache(maxsize=None)
def _inputs():
    mesh = synth.head_mesh(3000)
    P = np.concatenate([mesh, synth.control_points(64)[:8], (mesh[:200] * np.float32(1.6))]).astype(np.float32)
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(5)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    omega = np.random.default_rng(19).choice(np.array([0, 0.5, 1, 2], np.float32), P.shape[0])
    for a in (P, tu, tv, nrm, dist2, omega):
        a.setflags(write=False)
    assert P.shape[0] == N_FULL
    return P, tu, tv, nrm, dist2, omega


def _engine(kind, params, rest, delta):
    e = capi.Engine(device=0)
    e.set_points(rest, delta)
    e.set_kernel(kind, params)
    e.set_term(capi.TERM_LINEAR)
    e.build()
    return e


def _normalise(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def _projection(tu, tv, nrm):
    u, v, n = (_normalise(a.astype(LD)) for a in (tu, tv, nrm))
    Gm = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = _normalise(np.einsum("bi,bij->bj", u, Gm)); a2 = _normalise(np.einsum("bi,bij->bj", v, Gm))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def _psi(kind, P, centres, radii):
    """Psi, (N, C + 4) longdouble, in the convention of fd_get_weights' W: phi, then 1, x, y, z (linear term)."""
    X = P.astype(LD)
    D = X[:, None, :] - centres.astype(LD)[None]
    r2 = (D * D).sum(axis=-1)
    if kind == capi.KERNEL_THIN_PLATE:
        phi = np.where(r2 > 0, LD(0.5) * r2 * np.log(np.where(r2 > 0, r2, 1)), LD(0))
    else:
        phi = np.exp(-r2 / (radii.astype(LD)[None] ** 2))
    return np.concatenate([phi, np.ones((X.shape[0], 1), LD), X], axis=1)


def _system(e, kind, rest, S, P, T, omega, dist2, frames, mu, delta0):
    """(A, w, t, NN, b) in float64: D(delta) = A delta.ravel() on the live vertices (rows of the others are 0)."""
    W, radii = e.get_weights()
    n = W.shape[0] - 4
    centres = np.tile(rest.astype(np.float64), (n // rest.shape[0], 1))
    kw = dict(dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    _, fall = e.deform(P, **kw)
    B = (_psi(kind, P, centres, radii) @ S.astype(LD))                       # (N, M): the cardinal functions at the vertices
    f = fall.astype(LD)
    out = (fall == 0) if dist2 is None else ((dist2 > np.float32(RADIUS2)) | (fall == 0))
    f = np.where(out, LD(0), f)
    N, M = B.shape
    Pi = _projection(*frames) if frames is not None else np.broadcast_to(np.eye(3, dtype=LD), (N, 3, 3))
    A = (f[:, None, None, None] * Pi[:, :, None, :] * B[:, None, :, None]).astype(np.float64).reshape(3 * N, 3 * M)
    w = np.repeat(omega.astype(np.float64), 3)
    t = (T - P).astype(np.float64).ravel()                                   # the fp32 difference, as the call forms it
    NN = A.T @ (w[:, None] * A) + mu * np.eye(3 * M)
    b = A.T @ (w * t) + mu * delta0.astype(np.float64).ravel()
    return A, w, t, NN, b


def _energy(A, w, t, mu, delta0, delta):
    r = A.astype(LD) @ delta.astype(LD).ravel() - t.astype(LD)
    d = delta.astype(LD).ravel() - delta0.astype(LD).ravel()
    return float((w.astype(LD) * r * r).sum() + LD(mu) * (d * d).sum())


@functools.lru_cache(maxsize=None)
def _case(kind_name, M, proj):
    kind, params = KINDS[kind_name]
    P, tu, tv, nrm, dist2, omega = _inputs()
    rest = synth.control_points(M)
    rng = np.random.default_rng(100 + M)
    e = _engine(kind, params, rest, synth.rig_deltas(rest, 0))
    # targets: the displacement of another pose of the rig plus noise, so that the fit leaves a residual
    pose = _engine(kind, params, rest, (0.05 * rng.standard_normal(rest.shape)).astype(np.float32))
    T = (pose.deform(P)[0] + 0.01 * rng.standard_normal(P.shape)).astype(np.float32)
    pose.close()
    delta0 = (0.01 * rng.standard_normal(rest.shape)).astype(np.float32)
    mu = 1e-8 * float(omega.astype(np.float64).sum())
    frames = (tu, tv, nrm) if proj else None
    kw = dict(omega=omega, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE, mu=mu, delta0=delta0)
    W_before = e.get_weights()[0]
    S = e.solve_operator()
    fit, rep = e.fit_deltas(P, T, S=S, **kw)
    fit_own_S, _ = e.fit_deltas(P, T, S=None, **kw)
    W_after = e.get_weights()[0]
    ekind = capi.KERNEL_THIN_PLATE if kind == capi.KERNEL_THIN_PLATE else capi.KERNEL_GAUSSIAN
    A, w, t, NN, b = _system(e, ekind, rest, S, P, T, omega, dist2, frames, mu, delta0)
    e.close()
    return dict(fit=fit, fit_own_S=fit_own_S, rep=rep, W_before=W_before, W_after=W_after, A=A, w=w, t=t, NN=NN, b=b, mu=mu,
                delta0=delta0, M=M)


@pytest.mark.parametrize("kind_name,M,proj", CASES)
def test_optimality(hip_lib, kind_name, M, proj):
    c = _case(kind_name, M, proj)
    fit = c["fit"]
    assert fit.shape == (M, 3) and np.isfinite(fit).all()
    assert c["rep"].order == (3 * M if proj else M)
    assert 0 < c["rep"].pivot_min <= c["rep"].pivot_max
    res = np.linalg.norm(c["NN"] @ fit.ravel() - c["b"])
    bar1 = 2.0 ** -53 * (np.linalg.norm(c["NN"], 2) * np.linalg.norm(fit) + np.linalg.norm(c["b"]))
    print(f"fit {kind_name} M={M} proj={proj}: |NN d - b| / (2^-53 (|NN| |d| + |b|)) = {res / bar1:.2f}")
    lstsq = np.linalg.solve(c["NN"], c["b"]).reshape(M, 3)
    E_fit, E_ls = (_energy(c["A"], c["w"], c["t"], c["mu"], c["delta0"], d) for d in (fit, lstsq))
    E0 = _energy(c["A"], c["w"], c["t"], c["mu"], c["delta0"], c["delta0"].astype(np.float64))
    print(f"   E0 = {E0:.9e} (reported {c['rep'].E0:.9e}), E(fit) = {E_fit:.12e} (reported {c['rep'].E_fit:.12e}), "
          f"E(numpy) = {E_ls:.12e}, E(fit) / E(numpy) - 1 = {E_fit / E_ls - 1:.2e}")
    assert res <= KAPPA2[kind_name] * bar1
    assert 0 < E_fit <= E_ls * (1 + 1e-10) and E_fit < E0
    assert abs(c["rep"].E_fit - E_fit) <= 1e-10 * E_fit
    assert abs(c["rep"].E0 - E0) <= 1e-10 * E0


@pytest.mark.parametrize("kind_name,M,proj", CASES)
def test_operator_given_or_not_and_state(hip_lib, kind_name, M, proj):
    c = _case(kind_name, M, proj)
    assert np.array_equal(c["fit"].view(np.uint64), c["fit_own_S"].view(np.uint64))           # S given and S = NULL: the same bits
    assert np.array_equal(c["W_before"].view(np.uint64), c["W_after"].view(np.uint64))        # the context's model is as it was


@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_planted(hip_lib, kind_name):
    """Targets from fd_deform (fp64, positions) of a rig built on planted fp32 deltas; no gate, no f = 0, no projection,
    delta0 = 0, mu = 0.  The fitted deltas, rounded to fp32 and built, reproduce the targets."""
    kind, params = KINDS[kind_name]
    P = _inputs()[0]
    M = 64
    rest = synth.control_points(M)
    planted = (0.05 * np.random.default_rng(77).standard_normal(rest.shape)).astype(np.float32)
    pose = _engine(kind, params, rest, planted)
    pose.set_eval_precision(capi.EVAL_FP64)
    T = pose.deform(P)[0]
    pose.close()
    e = _engine(kind, params, rest, np.zeros_like(rest))
    fit, rep = e.fit_deltas(P, T)
    e.set_deltas(fit.astype(np.float32))
    e.build()
    e.set_eval_precision(capi.EVAL_FP64)
    out = e.deform(P)[0]
    e.close()
    ratio = l2_parity_ulp(out, T, P)
    print(f"planted {kind_name}: l2_parity_ulp = {ratio:.3f}; max |fit - planted| = {np.abs(fit - planted).max():.3e}; "
          f"E0 = {rep.E0:.6e}, E_fit = {rep.E_fit:.6e}")
    assert ratio <= 1.0


def test_singular_without_mu(hip_lib):
    """mu = 0 and every control point beyond the gate of every vertex (no live vertex at all): the normal matrix is zero,
    FD_E_SINGULAR; the same case with mu > 0 succeeds and returns delta0."""
    P = _inputs()[0][:500]
    rest = synth.control_points(33)
    e = _engine(capi.KERNEL_THIN_PLATE, [], rest, synth.rig_deltas(rest, 0))
    dist2 = np.full(P.shape[0], 2 * RADIUS2, np.float32)
    T = (P + np.float32(0.01)).astype(np.float32)
    delta0 = (0.01 * np.random.default_rng(2).standard_normal(rest.shape)).astype(np.float32)
    with pytest.raises(capi.FdError) as ei:
        e.fit_deltas(P, T, dist2=dist2, radius2=RADIUS2, falloffrate=RATE, mu=0.0, delta0=delta0)
    assert ei.value.code == capi.FD_E_SINGULAR
    fit, rep = e.fit_deltas(P, T, dist2=dist2, radius2=RADIUS2, falloffrate=RATE, mu=1e-3, delta0=delta0)
    assert np.allclose(fit, delta0.astype(np.float64), rtol=1e-14, atol=0) and rep.pivot_min == rep.pivot_max == 1e-3
    e.close()


def test_limits_answer_before_device_work(hip_lib):
    """C + 4 > 1028 (multilayer, 300 x 4 records) and an order above 3072 (1030 points with projection: 3090) are
    FD_E_INVALID; neither context has a model, so FD_E_NOT_BUILT would be the answer had the limits not come first."""
    arr = np.zeros((1, 3), np.float32)
    out = np.zeros((1100, 3), np.float64)
    ptr = capi._np_ptr
    for kind, params, M, frames in ((capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1], 300, False), (capi.KERNEL_THIN_PLATE, [], 1030, True)):
        e = capi.Engine(device=0)
        rest = synth.control_points(M)
        e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
        fr = ptr(arr) if frames else None
        rc = e.L.fd_fit_deltas(e.ctx, 1, ptr(arr), ptr(arr), None, None, fr, fr, fr, 1.0, 1.0, 0.0, None, None, ptr(out), None)
        assert rc == capi.FD_E_INVALID
        ok_M = 1024 if frames else 64
        rest = synth.control_points(ok_M)
        e.set_points(rest, synth.rig_deltas(rest, 0))
        if kind == capi.KERNEL_GAUSSIAN_ML:
            e.set_kernel(kind, [0.7, 2, 0.1])
        rc = e.L.fd_fit_deltas(e.ctx, 1, ptr(arr), ptr(arr), None, None, fr, fr, fr, 1.0, 1.0, 0.0, None, None, ptr(out), None)
        assert rc == capi.FD_E_NOT_BUILT
        e.close()
