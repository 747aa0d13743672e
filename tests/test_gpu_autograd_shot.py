"""GPU: facedeform_amd.autograd.deform_shot -- the F frames of a shot as one torch.autograd.Function over the batch calls.

F = 3 frames, N = 500 vertices, M = 32 control points, thin-plate and QNN, projection and gate on.

The bars:
  P.grad       against the sum of F autograd.deform backward passes on separate engines.  The fp64 results behind the two
               sides differ by at most twice tests/test_gpu_adjoint_points_shot.py's bar, which with KAPPA <= 4096 stays
               below 2^-40 of the magnitudes; each of the F + 1 fp32 values compared carries half an fp32 ulp of its own:
                   |P.grad - sum_f P.grad_f| <= (2^-24 + 2^-40) (sum_f |P.grad_f| + |P.grad|),   the sum taken in fp64.
  deltas.grad  against S^T grad_W of fd_deform_adjoint_dev per frame, rounded to fp32: one fp32 ulp of the value plus
               1e-10 |S|^T |grad_W| for the order of the fp64 sums.
  differences  tests/test_adjoint_points_restatement.py's convention, with the precision of what is differenced: the
               forward's outputs are fp32 (eps = 2^-24), so the step is h = 2^-7 where the longdouble restatement takes 2^-14.
               D(h) = sum_f g_f . (y_f(x + h e_k) - y_f(x - h e_k)) / (2 h); truncation |D(2h) - D(h)| / 3, bar twice that plus
               16 eps Y / h, Y = sum_f |g_f| . (magnitudes of the terms of y_f) from adjoint_points_cases.forward.  The map is
               linear in the deltas: no truncation there, the roundoff term alone (h = 2^-4)."""
import numpy as np
import pytest
import torch

import adjoint_points_cases as cases
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
F, N, M = 3, 500, 32
RADIUS2, RATE = 0.36, 1.7
KINDS = {"thin_plate": (capi.KERNEL_THIN_PLATE, [], cases.THIN_PLATE), "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0], cases.GAUSSIAN)}
EPS32 = 2.0 ** -24
DEV = lambda: torch.device("cuda", 0)


def _engines(kind_name, n):
    kind, params, _ = KINDS[kind_name]
    out = []
    for _ in range(n):
        e = capi.Engine(device=0)
        e.set_kernel(kind, list(params)); e.set_term(capi.TERM_LINEAR)
        out.append(e)
    return out


def _setup(kind_name):
    from facedeform_amd import autograd
    P = synth.head_mesh(3000)[::6][:N].copy()
    assert P.shape[0] == N
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(7)
    dist2 = (rng.random(N) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    G = rng.standard_normal((F, N, 3)).astype(np.float32)
    rest = synth.control_points(M)
    deltas = np.stack([synth.rig_deltas(rest, f) * np.float32(0.5 + 0.25 * f) for f in range(F)]).astype(np.float32)
    host = dict(P=P, tu=tu, tv=tv, nrm=nrm, dist2=dist2, G=G, rest=rest, deltas=deltas)
    d = {k: torch.from_numpy(v).to(DEV()) for k, v in host.items()}
    kw = dict(dist2=d["dist2"], tangents=(d["tu"], d["tv"], d["nrm"]), radius2=RADIUS2, falloffrate=RATE)
    engines = _engines(kind_name, F)
    batch = capi.Batch(engines)
    return autograd, batch, engines, host, d, kw


def _close(batch, engines):
    batch.close()
    for e in engines:
        e.close()


def _solve_operator(autograd, kind_name, host):
    e = _engines(kind_name, 1)[0]
    e.set_points(host["rest"], host["deltas"][0]); e.build()
    S = autograd.solve_operator_tensor(e)
    e.close()
    return S


@pytest.mark.parametrize("displacement", [False, True])
@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_gradients_against_the_one_frame_function(hip_lib, kind_name, displacement):
    autograd, batch, engines, host, d, kw = _setup(kind_name)
    S = _solve_operator(autograd, kind_name, host)
    P = d["P"].clone().requires_grad_(True)
    deltas = d["deltas"].clone().requires_grad_(True)
    out = autograd.deform_shot(batch, P, d["rest"], deltas, S=S, displacement=displacement, **kw)
    assert out.shape == (F, N, 3) and out.dtype == torch.float32
    (out * d["G"]).sum().backward()
    assert P.grad.shape == (N, 3) and P.grad.dtype == torch.float32 and deltas.grad.shape == (F, M, 3) and deltas.grad.dtype == torch.float32
    # the one-frame Function on separate engines
    singles = _engines(kind_name, F)
    per_P, per_d = [], []
    for f, e in enumerate(singles):
        e.set_points(host["rest"], host["deltas"][f]); e.build(); e.set_eval_precision(capi.EVAL_FP64)
        Pf = d["P"].clone().requires_grad_(True)
        df = d["deltas"][f].clone().requires_grad_(True)
        of = autograd.deform(e, Pf, df, S=S, displacement=displacement, **kw)
        # the forward is the fp64 launch: the same fp32 values up to the order of its fp64 sum
        assert (of.detach() - out.detach()[f]).abs().max().item() <= 2.0 ** -22 * of.detach().abs().max().item()
        (of * d["G"][f]).sum().backward()
        per_P.append(Pf.grad.double().cpu().numpy()); per_d.append(df.grad)
        # deltas.grad[f] against S^T grad_W of fd_deform_adjoint_dev
        gw = torch.empty((S.shape[0], 3), dtype=torch.float64, device=DEV())
        torch.cuda.synchronize()
        e.deform_adjoint_dev(N, d["P"].data_ptr(), d["G"][f].data_ptr(), gw.data_ptr(), d_dist2=d["dist2"].data_ptr(), d_tu=d["tu"].data_ptr(),
                             d_tv=d["tv"].data_ptr(), d_nrm=d["nrm"].data_ptr(), radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
        want = torch.matmul(S.t(), gw)
        slack = 1e-10 * torch.matmul(S.t().abs(), gw.abs())
        diff = (deltas.grad[f].double() - want).abs()
        assert (diff <= 2.0 ** -23 * want.abs() + slack).all(), (kind_name, f, float(diff.max()))
        assert torch.equal(per_d[f], want.to(torch.float32))
    got = P.grad.double().cpu().numpy()
    total = np.sum(per_P, axis=0)
    bar = (EPS32 + 2.0 ** -40) * (np.sum(np.abs(per_P), axis=0) + np.abs(got))
    err = np.abs(got - total)
    print(f"\n{kind_name} displacement={displacement}: worst |P.grad - sum_f P.grad_f| / bar = {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert (err <= bar).all() and np.abs(got).max() > 0
    for e in singles:
        e.close()
    _close(batch, engines)


@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_gradients_against_central_differences(hip_lib, kind_name):
    autograd, batch, engines, host, d, kw = _setup(kind_name)
    S = _solve_operator(autograd, kind_name, host)
    P = d["P"].clone().requires_grad_(True)
    deltas = d["deltas"].clone().requires_grad_(True)
    out = autograd.deform_shot(batch, P, d["rest"], deltas, S=S, **kw)
    (out * d["G"]).sum().backward()
    gP, gD = P.grad.double().cpu().numpy(), deltas.grad.double().cpu().numpy()
    fall = engines[0].deform(host["P"], dist2=host["dist2"], radius2=RADIUS2, falloffrate=RATE)[1]
    moved = ~(host["dist2"] > np.float32(RADIUS2)) & (fall != 0)
    verts = np.flatnonzero(moved)[[0, 50, 100, 150, 200]]
    tverts = torch.from_numpy(verts).to(DEV())
    # Y: the magnitudes of the terms of y_f, weighted by |g_f|
    Pi = cases.projection(host["tu"], host["tv"], host["nrm"])
    G = host["G"].astype(np.float64)
    Yv = np.zeros(N)
    for f, e in enumerate(engines):
        W, radii = e.get_weights()
        _, mag = cases.forward(KINDS[kind_name][2], W, host["rest"].astype(np.float64), radii, host["P"].astype(LD), np.where(moved, fall, 0), Pi)
        Yv += (np.abs(G[f]) * np.asarray(mag, np.float64)).sum(axis=1)

    def forward(Pt, Dt):
        with torch.no_grad():
            return autograd.deform_shot(batch, Pt, d["rest"], Dt, **kw).double().cpu().numpy()

    # positions: every vertex's outputs depend on its own position only, so the five are stepped together
    worst = 0.0
    for k in range(3):
        def quotient(h):
            Pp, Pm = d["P"].clone(), d["P"].clone()
            Pp[tverts, k] += h; Pm[tverts, k] -= h
            step = (Pp[tverts, k].double() - Pm[tverts, k].double()).cpu().numpy()          # what fp32 made of 2 h
            return (G[:, verts] * (forward(Pp, d["deltas"]) - forward(Pm, d["deltas"]))[:, verts]).sum(axis=(0, 2)) / step
        h = 2.0 ** -7
        d1, d2 = quotient(h), quotient(2 * h)
        bar = 2 * np.abs(d2 - d1) / 3 + 16 * EPS32 * Yv[verts] / h
        err = np.abs(gP[verts, k] - d1)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (kind_name, k, err, bar)
        assert (bar < 0.05 * np.abs(gP).max()).all()                                   # the bar is far below the values it guards
    # deltas: linear, the roundoff term alone
    h = 2.0 ** -4
    rng = np.random.default_rng(3)
    for f, j, a in zip(rng.integers(0, F, 5), rng.integers(0, M, 5), rng.integers(0, 3, 5)):
        Dp, Dm = d["deltas"].clone(), d["deltas"].clone()
        Dp[f, j, a] += h; Dm[f, j, a] -= h
        step = float(Dp[f, j, a].double() - Dm[f, j, a].double())
        q = float((G * (forward(d["P"], Dp) - forward(d["P"], Dm))).sum()) / step
        bar = 16 * EPS32 * (float(Yv.sum()) + h * float(np.abs(G[f]).sum())) / h
        worst = max(worst, abs(gD[f, j, a] - q) / bar)
        assert abs(gD[f, j, a] - q) <= bar, (kind_name, f, j, a, gD[f, j, a], q, bar)
    print(f"\n{kind_name}: worst |grad - D(h)| / bar = {worst:.3f}")
    _close(batch, engines)


def test_errors(hip_lib):
    autograd, batch, engines, host, d, kw = _setup("thin_plate")
    deltas = d["deltas"].clone().requires_grad_(True)
    with pytest.raises(ValueError):                       # deltas that require grad need S
        autograd.deform_shot(batch, d["P"], d["rest"], deltas, **kw)
    with pytest.raises(ValueError):
        autograd.deform_shot(batch, d["P"].cpu(), d["rest"], d["deltas"], **kw)
    with pytest.raises(ValueError):
        autograd.deform_shot(batch, d["P"], d["rest"], d["deltas"][:2], **kw)
    # a backward whose models a later forward has replaced
    P1 = d["P"].clone().requires_grad_(True)
    out1 = autograd.deform_shot(batch, P1, d["rest"], d["deltas"], **kw)
    P2 = d["P"].clone().requires_grad_(True)
    out2 = autograd.deform_shot(batch, P2, d["rest"], d["deltas"], **kw)
    with pytest.raises(RuntimeError, match="replaced"):
        out1.sum().backward()
    out2.sum().backward()                                 # the latest forward's backward goes through
    assert P2.grad is not None and P1.grad is None
    _close(batch, engines)
