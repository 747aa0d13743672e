"""What tests/test_gpu_bake_grad.py and tests/test_bake_grad_abi.py share: the cases and the np.longdouble restatement of
fd_deform_bake_grad* -- G[v][a][i] = f_v sum_j dPsi_vj/dx_a S_ji (include/facedeform_hip.h states the contract).  dPsi is
restated here from the header's table, in the convention of fd_get_weights' W, from the rest rig and the radii the engine
reports; never from the call's own output.  The inputs, the kinds and Psi itself are tests/bake_cases.py's.  Nothing here needs
a GPU to import."""
import os
import re

import numpy as np

import bake_cases as bc
from facedeform_amd import _build, capi

LD = bc.LD


def _plan_constant(name):
    text = open(os.path.join(_build.CSRC, "fd_bake_plan.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


# the gradient launch's column panel (fd_bake_plan.h): 16 columns per tile, kGradPanelTiles tiles
PG = bc.TILE * _plan_constant("kGradPanelTiles")

# tests/bake_cases.py's cases, and thin-plate and QNN around the gradient launch's own panel: its last column count with one
# panel, the first with two (equalised), and three panels with a sliver
CASES = list(bc.CASES)
for _k in ("thin_plate", "qnn"):
    for _M in (PG - 1, PG, PG + 1, 2 * PG + 1):
        if (_k, "linear", _M, False) not in CASES:
            CASES.append((_k, "linear", _M, False))


def dphi(kind, X, centres, radii):
    """d phi_j / d x_a at x_v in the convention of fd_get_weights' W (the header's table), longdouble, (N, 3, C)."""
    D = X[:, None, :] - centres[None]                      # (N, C, 3)
    r2 = (D * D).sum(axis=-1)
    pos = r2 > 0
    safe = np.where(pos, r2, LD(1))
    if kind == capi.KERNEL_THIN_PLATE:                     # (x - c)(2 ln r + 1) = (x - c)(ln r^2 + 1)
        s = np.where(pos, np.log(safe) + LD(1), LD(0))
    elif kind == capi.KERNEL_BIHARMONIC:                   # -(x - c) / r
        s = np.where(pos, -LD(1) / np.sqrt(safe), LD(0))
    elif kind == capi.KERNEL_CUBIC:                        # 3 r (x - c)
        s = LD(3) * np.sqrt(r2)
    else:                                                  # -2 (x - c) / R^2 . phi
        R2 = radii.astype(LD)[None] ** 2
        s = -LD(2) / R2 * np.exp(-r2 / R2)
    return np.transpose(s[:, :, None] * D, (0, 2, 1))


def dpsi(kind, P, centres, radii, rows):
    """dPsi, (N, 3, C + 4) longdouble: d phi / d x_a in W's convention, then d/dx_a of 1, x, y, z; columns the term lacks are
    0.  centres in W's layout: the multilayer model's record l * M + c sits on centre c."""
    X = P.astype(LD)
    N, Cn = X.shape[0], centres.shape[0]
    out = np.zeros((N, 3, Cn + 4), LD)
    out[:, :, :Cn] = dphi(bc.eval_kind(kind), X, centres.astype(LD), radii)
    for a in range(3):
        out[:, a, Cn + 1 + a] = 1
    out[:, :, Cn + rows:] = 0
    return out


def dpsi_abs(kind, P, centres, radii, rows):
    """The magnitude of dPsi as computed: thin-plate |x_a - c_a| (|ln d2| + 1) -- the logarithm and the 1 are added after each
    is formed -- and |dPsi| for the others."""
    out = np.abs(dpsi(kind, P, centres, radii, rows))
    if bc.eval_kind(kind) == capi.KERNEL_THIN_PLATE:
        X, c = P.astype(LD), centres.astype(LD)
        D = X[:, None, :] - c[None]
        r2 = (D * D).sum(axis=-1)
        pos = r2 > 0
        s = np.where(pos, np.abs(np.log(np.where(pos, r2, LD(1)))) + LD(1), LD(0))
        out[:, :, :c.shape[0]] = np.transpose(s[:, :, None] * np.abs(D), (0, 2, 1))
    return out


def restatement(dPsi, dPsi_abs, S, fall, dist2):
    """(ref, bar1, out): ref = f (dPsi @ S) and bar1 = |f| (dPsi_abs @ |S|), (N, 3, M) longdouble each, the blocks of the
    vertices that are out -- gated or f = 0 -- exactly 0 in both; `out` says which those are."""
    f = fall.astype(LD)
    out = (fall == 0) if dist2 is None else ((dist2 > np.float32(bc.RADIUS2)) | (fall == 0))
    f = np.where(out, LD(0), f)
    Sl = S.astype(LD)
    ref = f[:, None, None] * (dPsi @ Sl)
    bar1 = np.abs(f)[:, None, None] * (dPsi_abs @ np.abs(Sl))
    ref[out] = 0; bar1[out] = 0
    return ref, bar1, out
