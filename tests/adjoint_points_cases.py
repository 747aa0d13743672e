"""The yardstick of fd_deform_adjoint_points*: the deformation, its Jacobian and the two cotangents restated in np.longdouble.

Inputs are what a caller can read off an engine -- the weights in fd_get_weights' layout ((C + 4, 3): C rows of RBF weights,
then the constant row and the three linear rows), the centres in that layout, the radii the engine reports, the fall-off
fd_deform reports -- or any synthetic model of the same shape: nothing here needs an engine or a GPU.

Notation is include/facedeform_hip.h's: P' = x + f Pi d(x), d(x) = sum_j w_j phi_j(x - c_j) + w_C + L x, J = dd/dx,
A = I + f Pi J, r = f Pi g;
    grad_P = A^T g = g + sum_j (w_j . r) grad phi_j(x - c_j) + L^T r,        grad_f = g . Pi d(x).
phi and grad phi per kind are the header's table in W's convention, i.e. with the factors fd_pack.h's weight_scale64 moves
into the evaluation records (the 0.5 of thin-plate, the sign of biharmonic):
    thin-plate   phi = 0.5 r^2 ln r^2     grad phi = (x - c)(ln r^2 + 1), 0 at r = 0
    Gaussian     phi = exp(-r^2 / R_j^2)  grad phi = -2 (x - c) / R_j^2 phi        (QNN and multilayer: one record each)
    biharmonic   phi = -r                 grad phi = -(x - c) / r, 0 at r = 0
    cubic        phi = r^3                grad phi = 3 r (x - c)

Beside each result comes the magnitude its error bar is a multiple of:
    T_P[v][k] = sum_j |grad phi_j|_inf |w_j . r_v| + sum_c |L[c][k]| |r_v[c]|
    T_f[v]    = sum_c |(Pi g)_c| (sum_j |w_j[c]| |phi_j| + |w_C[c]| + sum_k |L[c][k]| |x_k|)
"""
import numpy as np

LD = np.longdouble

THIN_PLATE, GAUSSIAN, BIHARMONIC, CUBIC = "thin_plate", "gaussian", "biharmonic", "cubic"
KINDS = (THIN_PLATE, GAUSSIAN, BIHARMONIC, CUBIC)


def normalise(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def projection(tu, tv, nrm):
    """Pi = a1 a1^T + a2 a2^T as project_to_tangents builds a1, a2, in longdouble, (N, 3, 3)."""
    u, v, n = (normalise(np.asarray(a).astype(LD)) for a in (tu, tv, nrm))
    Gm = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = normalise(np.einsum("bi,bij->bj", u, Gm)); a2 = normalise(np.einsum("bi,bij->bj", v, Gm))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def phi_grad(kind, X, centres, radii):
    """(phi, gphi): phi_j(x_v) as (N, C) and grad phi_j(x_v - c_j) as (N, C, 3), the table above, longdouble."""
    D = X[:, None, :] - centres[None]
    r2 = (D * D).sum(axis=-1)
    pos = r2 > 0
    safe = np.where(pos, r2, LD(1))
    if kind == THIN_PLATE:
        ln = np.log(safe)
        phi = np.where(pos, LD(0.5) * r2 * ln, LD(0))
        s = np.where(pos, ln + 1, LD(0))
    elif kind == GAUSSIAN:
        R2 = (np.asarray(radii).astype(LD) ** 2)[None]
        phi = np.exp(-r2 / R2)
        s = -2 * phi / R2
    elif kind == BIHARMONIC:
        r = np.sqrt(r2)
        phi = -r
        s = np.where(pos, -1 / np.sqrt(safe), LD(0))
    elif kind == CUBIC:
        r = np.sqrt(r2)
        phi = r2 * r
        s = 3 * r
    else:
        raise ValueError(kind)
    return phi, s[:, :, None] * D


def _split(W):
    W = np.asarray(W).astype(LD)
    C = W.shape[0] - 4
    return W[:C], W[C], W[C + 1:].T          # w (C, 3), constant (3,), L[c][k] = W[C + 1 + k][c]


def field(kind, W, centres, radii, X):
    """d(x_v) (N, 3) and, per component, the sum of its terms' magnitudes."""
    w, w0, L = _split(W)
    phi, _ = phi_grad(kind, X, np.asarray(centres).astype(LD), radii)
    d = phi @ w + w0[None] + X @ L.T
    mag = np.abs(phi) @ np.abs(w) + np.abs(w0)[None] + np.abs(X) @ np.abs(L).T
    return d, mag


def forward(kind, W, centres, radii, X, f, Pi=None):
    """y_v = x_v + f_v Pi_v d(x_v), longdouble; Pi None: the identity.  Also the magnitude sum behind each component."""
    d, mag = field(kind, W, centres, radii, X)
    if Pi is not None:
        mag = np.einsum("bij,bj->bi", np.abs(Pi), mag)
        d = np.einsum("bij,bj->bi", Pi, d)
    f = np.asarray(f).astype(LD)[:, None]
    return X + f * d, np.abs(X) + np.abs(f) * mag


def restatement(kind, W, centres, radii, P, G, f, Pi=None, identity=None, unmoved=None):
    """grad_P (N, 3), T_P (N, 3), grad_f (N,), T_f (N,) in longdouble.

    f: the fall-off per vertex; Pi: (N, 3, 3) or None for the identity.  identity: the vertices where A = I by the contract
    (gated, f = 0, or the whole mesh of a model that is not built): grad_P = g there and T_P = 0.  unmoved: the vertices whose
    grad_f is 0.0 by the contract (gated, or a model that is not built; NOT f = 0)."""
    X = np.asarray(P).astype(LD)
    g = np.asarray(G).astype(LD)
    n = X.shape[0]
    identity = np.zeros(n, bool) if identity is None else np.asarray(identity, bool)
    unmoved = np.zeros(n, bool) if unmoved is None else np.asarray(unmoved, bool)
    w, w0, L = _split(W)
    phi, gphi = phi_grad(kind, X, np.asarray(centres).astype(LD), radii)
    pg = g if Pi is None else np.einsum("bij,bj->bi", Pi, g)
    r = np.asarray(f).astype(LD)[:, None] * pg
    r[identity] = 0
    wr = r @ w.T                                                     # (N, C): w_j . r_v
    grad_P = g + np.einsum("bj,bjk->bk", wr, gphi) + r @ L
    T_P = (np.abs(gphi).max(axis=2) * np.abs(wr)).sum(axis=1)[:, None] + np.abs(r) @ np.abs(L)
    grad_P[identity] = g[identity]
    T_P[identity] = 0
    d = phi @ w + w0[None] + X @ L.T
    dmag = np.abs(phi) @ np.abs(w) + np.abs(w0)[None] + np.abs(X) @ np.abs(L).T
    grad_f = (pg * d).sum(axis=1)
    T_f = (np.abs(pg) * dmag).sum(axis=1)
    grad_f[unmoved] = 0
    T_f[unmoved] = 0
    return grad_P, T_P, grad_f, T_f


def jacobian(kind, W, centres, radii, P, f, Pi=None):
    """A = I + f Pi J (N, 3, 3), row c = output c, column k = d/dx_k, longdouble."""
    X = np.asarray(P).astype(LD)
    w, _, L = _split(W)
    _, gphi = phi_grad(kind, X, np.asarray(centres).astype(LD), radii)
    J = np.einsum("jc,bjk->bck", w, gphi) + L[None]
    if Pi is not None:
        J = np.einsum("bij,bjk->bik", Pi, J)
    return np.eye(3, dtype=LD)[None] + np.asarray(f).astype(LD)[:, None, None] * J


def ratios(got_P, got_f, ref):
    """Worst |got - ref| / bar with kappa = 1, for grad_P and for grad_f (None: not asked), and the vertex of each.

    The bar of grad_P is 2^-53 T_P plus 2^-53 |ref|: the second term is the rounding of the stored fp64 value itself (half an
    ulp), which no implementation can avoid and which is all there is where T_P is 0 or small beside g (A = I, f near 0).  It is
    not scaled by kappa (callers add it once): here it is folded in by measuring the excess over it."""
    grad_P, T_P, grad_f, T_f = ref
    u = LD(2) ** -53
    err = np.abs(np.asarray(got_P).astype(LD) - grad_P) - u * np.abs(grad_P)
    err = np.maximum(err, 0)
    assert (err[T_P == 0] == 0).all(), "a vertex with A = I differs from g by more than its rounding"
    q = np.where(T_P > 0, err / np.where(T_P > 0, u * T_P, 1), 0)
    vP = int(np.argmax(q.max(axis=1))) if q.size else 0
    rP = float(q.max()) if q.size else 0.0
    if got_f is None:
        return rP, vP, None, None
    ef = np.abs(np.asarray(got_f).astype(LD) - grad_f)
    assert (ef[T_f == 0] == 0).all()
    qf = np.where(T_f > 0, ef / np.where(T_f > 0, u * T_f, 1), 0)
    return rP, vP, (float(qf.max()) if qf.size else 0.0), (int(np.argmax(qf)) if qf.size else 0)
