"""What tests/test_gpu_bake.py and tests/test_bake_abi.py share: the inputs, the cases and the np.longdouble restatement of
fd_deform_bake* -- B[v][i] = f_v sum_j Psi_vj S_ji (include/facedeform_hip.h states the contract).  Psi is restated here as
tests/test_gpu_gram.py restates it, from the weights' layout, the rest rig and the radii the engine reports; never from the
call's own output.  Nothing here needs a GPU to import."""
import functools

import numpy as np

from facedeform_amd import capi, synth

LD = np.longdouble
KINDS = {
    "thin_plate": (capi.KERNEL_THIN_PLATE, []),
    "gaussian": (capi.KERNEL_GAUSSIAN, [0.35]),
    "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
    "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 2, 0.1]),
    "multilayer4": (capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1]),
    "biharmonic": (capi.KERNEL_BIHARMONIC, []),
    "cubic": (capi.KERNEL_CUBIC, []),
}
FAMILY = {"thin_plate": "polyharmonic", "biharmonic": "polyharmonic", "cubic": "polyharmonic", "gaussian": "gaussian",
          "qnn": "gaussian", "multilayer": "gaussian", "multilayer4": "gaussian"}
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
TERM_ROWS = {"linear": 4, "const": 1, "zero": 0}
RADIUS2, RATE = 0.36, 1.7
M_RIG = 64
N_FULL = 777
# the launch's constants (fd_bake_plan.h): a wave's 16 vertices, a workgroup's 128, a panel's 256 columns
TILE, GROUP, PANEL = 16, 128, 256

# (kind, term, M, frames): every kind at 64 points with and without frames, the terms, the column counts around a tile, two
# and four tiles (17: a second tile; 33: a third; 64: the narrow launch's last; 65 and 80: the wide launch's first), and rigs
# above the column panel.  One and three points cannot carry a linear term (four polynomial columns), and a lone point has no
# neighbour for the QNN radii: those two rigs are plain Gaussians with the term they can carry.
CASES = [(k, "linear", M_RIG, fr) for k in sorted(KINDS) for fr in (False, True)] + \
        [(k, t, M_RIG, False) for k in ("thin_plate", "qnn") for t in ("const", "zero")] + \
        [("gaussian", "zero", 1, False), ("gaussian", "const", 3, False)] + \
        [("thin_plate", "linear", M, False) for M in (15, 16, 17, 33, 65, 80)] + \
        [("qnn", "linear", M, False) for M in (15, 17, 33)] + \
        [("qnn", "linear", PANEL + 1, False), ("thin_plate", "linear", PANEL + 1, False), ("qnn", "linear", 300, True)]
N_SHAPES = (0, 1, TILE - 1, TILE, TILE + 1, GROUP - 1, GROUP, GROUP + 1, N_FULL)


@functools.lru_cache(maxsize=None)
def inputs():
    """tests/test_gpu_gram.py's recipe, cut down to 777 vertices: head-mesh vertices, 8 points on centres, some off the
    surface, a gate that removes about a third, every 97th vertex exactly on the radius (f = 0)."""
    mesh = synth.head_mesh(700)
    P = np.concatenate([mesh, synth.control_points(M_RIG)[:8], (mesh[:69] * np.float32(1.6))]).astype(np.float32)
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(5)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    for a in (P, tu, tv, nrm, dist2):
        a.setflags(write=False)
    assert P.shape[0] == N_FULL
    return P, tu, tv, nrm, dist2


def rig(M):
    return synth.control_points(M)


# ---- the restatement ---------------------------------------------------------------------------------------------

def normalise(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def projection(tu, tv, nrm):
    """Pi = a1 a1^T + a2 a2^T as project_to_tangents builds a1, a2, in longdouble."""
    u, v, n = (normalise(a.astype(LD)) for a in (tu, tv, nrm))
    Gm = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = normalise(np.einsum("bi,bij->bj", u, Gm)); a2 = normalise(np.einsum("bi,bij->bj", v, Gm))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def eval_kind(kind):
    return capi.KERNEL_GAUSSIAN if kind in (capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_GAUSSIAN_ML) else kind


def phi(kind, X, centres, radii):
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


def psi(kind, P, centres, radii, rows):
    """Psi, (N, C + 4) longdouble: phi in W's convention, then 1, x, y, z; columns the term lacks are 0.  centres in W's
    layout: the multilayer model's record l * M + c sits on centre c."""
    X = P.astype(LD)
    Psi = np.concatenate([phi(eval_kind(kind), X, centres.astype(LD), radii), np.ones((X.shape[0], 1), LD), X], axis=1)
    Psi[:, centres.shape[0] + rows:] = 0
    return Psi


def restatement(Psi, S, fall, dist2):
    """(ref, bar1, out): ref = f (Psi @ S) and bar1 = |f| (|Psi| @ |S|), (N, M) longdouble each, rows of the vertices that are
    out -- gated or f = 0 -- exactly 0 in both; `out` says which those are."""
    f = fall.astype(LD)
    out = (fall == 0) if dist2 is None else ((dist2 > np.float32(RADIUS2)) | (fall == 0))
    f = np.where(out, LD(0), f)
    Sl = S.astype(LD)
    ref = f[:, None] * (Psi @ Sl)
    bar1 = np.abs(f)[:, None] * (np.abs(Psi) @ np.abs(Sl))
    ref[out] = 0; bar1[out] = 0
    return ref, bar1, out


def ratio(got, ref, bar1):
    """Worst |got - ref| / (2^-53 bar1) over the entries; where the bar is 0 both sides must be exact zeros."""
    assert got.shape == ref.shape
    err = np.abs(got.astype(LD) - ref)
    bar = LD(2) ** -53 * bar1
    zero = bar == 0
    assert (ref[zero] == 0).all() and np.array_equal(got[zero].view(np.uint64), np.zeros(int(zero.sum()), np.uint64))
    if not (~zero).any():
        return 0.0, None
    r = np.where(zero, LD(0), err / np.where(zero, LD(1), bar))
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), tuple(int(a) for a in at)
