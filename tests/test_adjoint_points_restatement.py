"""CPU: the longdouble restatement of fd_deform_adjoint_points (tests/adjoint_points_cases.py) held to central differences of
the restated forward map -- the yardstick of tests/test_gpu_adjoint_points.py is itself checked, with no engine.

A synthetic model: 12 centres, random weights with a linear term, every kind, projection on and off; 40 vertices.
For each coordinate k the identity  grad_P[v][k] = g_v . dy_v/dx_k  is checked with
    D(h) = (y(x + h e_k) - y(x - h e_k)) / (2 h),   h = 2^-14,
whose error is c h^2 + O(h^4): D(2h) - D(h) = 3 c h^2 + O(h^4), so the difference's own truncation is |D(2h) - D(h)| / 3.
The bar is twice that (the O(h^4) remainder is a factor h^2 = 4e-9 below it) plus the roundoff of the difference quotient,
16 eps Y / h with eps longdouble's and Y the sum of the magnitudes of the terms of y (cases.forward returns it).
grad_f is the derivative in f, in which the map is linear: its difference quotient has no truncation, only the roundoff.
A wrong factor anywhere (the 0.5 of thin-plate, a sign, a transpose of L or Pi) is an error of order 1."""
import numpy as np
import pytest

import adjoint_points_cases as cases

LD = np.longdouble
H = LD(2) ** -14
EPS = LD(np.finfo(LD).eps)


def _model(kind, seed=1):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (12, 3))
    W = rng.standard_normal((16, 3)) * 0.3
    radii = rng.uniform(0.5, 1.2, 12)
    X = rng.uniform(-1.2, 1.2, (40, 3)).astype(np.float32)
    G = rng.standard_normal((40, 3)).astype(np.float32)
    f = rng.uniform(0.05, 1.0, 40).astype(np.float32)
    frames = tuple(rng.standard_normal((40, 3)).astype(np.float32) for _ in range(3))
    return centres, W, radii, X, G, f, frames


@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_restatement_against_central_differences(kind, proj):
    centres, W, radii, X, G, f, frames = _model(kind)
    Pi = cases.projection(*frames) if proj else None
    grad_P, T_P, grad_f, T_f = cases.restatement(kind, W, centres, radii, X, G, f, Pi)
    assert (T_P > 0).all() and (T_f > 0).all()
    g = G.astype(LD)
    x = X.astype(LD)
    worst = 0.0
    for k in range(3):
        e = np.zeros(3, LD); e[k] = 1

        def quotient(h):
            yp, mp = cases.forward(kind, W, centres, radii, x + h * e, f, Pi)
            ym, mm = cases.forward(kind, W, centres, radii, x - h * e, f, Pi)
            return (g * (yp - ym)).sum(axis=1) / (2 * h), (np.abs(g) * np.maximum(mp, mm)).sum(axis=1)

        d1, mag = quotient(H)
        d2, _ = quotient(2 * H)
        bar = 2 * np.abs(d2 - d1) / 3 + 16 * EPS * mag / H
        err = np.abs(grad_P[:, k] - d1)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (kind, proj, k)
        assert float((bar / np.abs(grad_P[:, k]).max()).max()) < 1e-4          # the bar is far below the values it guards
    # grad_f: y is linear in f
    fl = f.astype(LD)
    yp, mp = cases.forward(kind, W, centres, radii, x, fl + H, Pi)
    ym, mm = cases.forward(kind, W, centres, radii, x, fl - H, Pi)
    q = (g * (yp - ym)).sum(axis=1) / (2 * H)
    bar = 16 * EPS * (np.abs(g) * np.maximum(mp, mm)).sum(axis=1) / H
    assert (np.abs(grad_f - q) <= bar).all(), (kind, proj)
    print(f"{kind} proj={proj}: worst |grad_P - D(h)| / bar = {worst:.3f}")


@pytest.mark.parametrize("kind", cases.KINDS)
def test_restatement_is_the_transposed_jacobian(kind):
    """grad_P = A^T g with the A the helper states for fd_deform_vectors' jacobian output, to longdouble rounding."""
    centres, W, radii, X, G, f, frames = _model(kind, seed=2)
    Pi = cases.projection(*frames)
    grad_P, T_P, _, _ = cases.restatement(kind, W, centres, radii, X, G, f, Pi)
    A = cases.jacobian(kind, W, centres, radii, X, f, Pi)
    viaA = np.einsum("bck,bc->bk", A, G.astype(LD))
    assert (np.abs(viaA - grad_P) <= 64 * EPS * (T_P + np.abs(G.astype(LD)))).all()


def test_identity_and_unmoved_vertices():
    centres, W, radii, X, G, f, frames = _model(cases.THIN_PLATE, seed=3)
    ident = np.zeros(40, bool); ident[::3] = True
    unmoved = np.zeros(40, bool); unmoved[::6] = True
    grad_P, T_P, grad_f, T_f = cases.restatement(cases.THIN_PLATE, W, centres, radii, X, G, f, None, ident, unmoved)
    assert np.array_equal(grad_P[ident], G.astype(LD)[ident]) and (T_P[ident] == 0).all()
    assert (grad_f[unmoved] == 0).all() and (T_f[unmoved] == 0).all()
    assert (grad_f[ident & ~unmoved] != 0).all()                       # f = 0: the formula's value
    # a vertex on a centre: grad phi is 0 there for the two kinds whose table says so
    Xc = np.concatenate([centres[:2].astype(np.float32).astype(np.float64), X[:2]]).astype(np.float32)
    for kind in (cases.THIN_PLATE, cases.BIHARMONIC):
        _, gphi = cases.phi_grad(kind, Xc.astype(LD), Xc[:2].astype(LD), radii[:2])
        assert (gphi[0, 0] == 0).all() and (gphi[1, 1] == 0).all() and np.isfinite(gphi.astype(np.float64)).all()
