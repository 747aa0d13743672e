"""Shared inputs for the tests that hold the morph-space factorisation (csrc/fd_morph.hip, fdo_morph_*) to its
references on every path the host code can take: seeded blendshape sets, two plain fp64 references and the list of cases.

A plain module (no fixture, no test): `from morph_cases import ...`.  Everything is deterministic.

Why these sizes (rows = 3N; the device code works on workgroups of 1024 rows in the blocked factorisation, 2048 in the
one-frame weights, 4096 in the column-by-column factorisation, panels of 8 columns, and takes the column-by-column form
above 256 blendshapes):
  column   S > 256: dense; rows = S + 1 (k crosses the 256-lane strip, the last tails are one or two rows); a second
           workgroup of two rows; three full workgroups and no ragged one; zero columns at both ends of the 256 boundary
  limit    S = 249..256 is the blocked form's largest LDS request; exact multiples of a workgroup's rows; 15 and 17
           workgroups leave slices of the first-stage reduction empty
  many     411 and 513 blocked workgroups: the setup kernel's four-way sweep and its remainder, 257 weight partitions; a
           last panel of three columns and of one
  zero     a zero column first / last in its panel, a whole zero panel, the last column of the matrix; a column whose only
           entry is on the diagonal; duplicated blendshapes in one panel, across panels, on the column-by-column path
  top      FD_MORPH_MAX_SHAPES blendshapes: the one-frame weights' 64 KB of LDS
"""
from collections import namedtuple

import numpy as np

SEED = 20261020
MAX_SHAPES = 2048                                 # FD_MORPH_MAX_SHAPES (include/facedeform_hip.h)

# kind: "dense" (rest + 0.1 normal) or "sparse" (0.05 normal on 30 % of the vertices); zeros: columns equal to the rest
# pose; dup: (dst, src) -- shape dst := shape src; lone: column 0 moves only x of vertex 0, by 0.25
Case = namedtuple("Case", "name N S kind zeros dup lone")


def _c(N, S, kind="dense", zeros=(), dup=None, lone=False):
    name = f"{N}x{S}" + ("-sparse" if kind == "sparse" else "") + ("-z" + "_".join(map(str, zeros)) if zeros else "") + \
        (f"-dup{dup[0]}is{dup[1]}" if dup else "") + ("-lone0" if lone else "")
    return Case(name, N, S, kind, tuple(zeros), dup, lone)


COLUMN = [_c(700, 257), _c(86, 257), _c(1366, 264, "sparse", (0, 255, 256, 263)), _c(4096, 257), _c(700, 300, zeros=(0, 255, 256, 299))]
LIMIT = [_c(700, 249), _c(700, 255), _c(700, 256), _c(86, 256), _c(1024, 16), _c(5000, 20), _c(5462, 20)]
MANY = [_c(140001, 11, "sparse"), _c(175001, 9, "sparse")]
ZERO = [_c(700, 20, zeros=(0,)), _c(700, 20, zeros=(7, 8)), _c(700, 20, zeros=(15, 16, 19)), _c(700, 24, zeros=tuple(range(8, 16))),
        _c(700, 17, zeros=(16,))]
LONE = [_c(700, 20, lone=True)]
DUPLICATE = [_c(700, 20, dup=(4, 3)), _c(700, 20, dup=(12, 3)), _c(700, 300, dup=(290, 10))]
TOP = _c(683, MAX_SHAPES)
REINIT = [_c(700, 9), _c(86, 257), _c(5, 8), _c(700, 256), _c(175001, 9, "sparse"), _c(700, 9)]

ENTRYWISE = COLUMN + LIMIT + MANY + ZERO + LONE          # the two references agree entry by entry
ALL = ENTRYWISE + DUPLICATE + [TOP]


def ids(cases):
    return [c.name for c in cases]


def _rng(case, stream):
    return np.random.default_rng([SEED, case.N, case.S, stream])


def make(case):
    """-> rest (N, 3) float32, shapes: S arrays (N, 3) float32."""
    rng = _rng(case, 0)
    N = case.N
    rest = rng.normal(size=(N, 3)).astype(np.float32)
    shapes = []
    for _ in range(case.S):
        if case.kind == "dense":
            shapes.append((rest + 0.1 * rng.normal(size=(N, 3))).astype(np.float32))
        else:
            shapes.append((rest + (0.05 * rng.normal(size=(N, 3)) * (rng.random((N, 1)) < 0.3)).astype(np.float32)).astype(np.float32))
    for z in case.zeros:
        shapes[z] = rest.copy()
    if case.dup:
        shapes[case.dup[0]] = shapes[case.dup[1]].copy()
    if case.lone:
        shapes[0] = rest.copy()
        shapes[0][0, 0] += np.float32(0.25)
    return rest, shapes


def frames(case, rest, shapes, F=1):
    """F deformed meshes: a mixture of up to three blendshapes plus noise on every vertex, so that every column's weight
    sees every row partition."""
    rng = _rng(case, 1)
    out = []
    for _ in range(F):
        P = rest.copy()
        for _ in range(min(case.S, 3)):
            s = int(rng.integers(case.S))
            P = (P + np.float32(rng.uniform(-0.6, 0.9)) * (shapes[s] - rest)).astype(np.float32)
        out.append((P + (0.002 * rng.normal(size=rest.shape)).astype(np.float32)).astype(np.float32))
    return out


# ---- references --------------------------------------------------------------------------------
def shapes_matrix(rest, shapes):
    """(3N, S) F-ordered float64 of the fp32 deltas shape - rest (reference src/dbse.cpp:16-31), in numpy."""
    rest = np.asarray(rest, np.float32)
    A = np.empty((rest.size, len(shapes)), np.float64, order="F")
    for s, sh in enumerate(shapes):
        A[:, s] = (np.asarray(sh, np.float32) - rest).reshape(-1)
    return A


def lapack_raw(A):
    """LAPACK's dgeqrf through numpy -> (packed QR, F-ordered (rows, S); tau (S,)): the convention of the oracle, of
    Eigen's HouseholderQR and of tests/golden/morph_golden.npz."""
    h, tau = np.linalg.qr(np.asarray(A, np.float64), mode="raw")
    return np.asfortranarray(h.T), np.asarray(tau, np.float64)


def reconstruct(QR, tau):
    """Q R from the packed form, numpy only: H_0 .. H_{S-1} [triu(QR[:S]); 0] with H_k = I - tau_k v_k v_k^T,
    v_k = (0 .. 0, 1, QR[k+1:, k]), applied last to first.  H_k touches rows and columns k.. only: what stands in the
    columns before k has nothing below row k yet."""
    QR = np.asarray(QR, np.float64)
    rows, S = QR.shape
    B = np.zeros((rows, S), np.float64, order="F")
    B[:S] = np.triu(QR[:S])
    for k in range(S - 1, -1, -1):
        if tau[k] == 0.0:
            continue
        v = np.concatenate(([1.0], QR[k + 1:, k]))
        B[k:, k:] -= tau[k] * np.outer(v, v @ B[k:, k:])
    return B


def residual(QR, tau, A):
    """||reconstruct(QR, tau) - A||_F / ||A||_F: the factorisation's backward error."""
    return float(np.linalg.norm(reconstruct(QR, tau) - A) / np.linalg.norm(A))


def weights_numpy(QR, P, rest):
    """w_s = sum_i double(float(P_i - rest_i)) QR[i][s] (dbse.cpp:39-60) as one numpy product."""
    d = (np.asarray(P, np.float32) - np.asarray(rest, np.float32)).reshape(-1).astype(np.float64)
    return d @ np.asarray(QR, np.float64)


_cache = {}


def reference(oracle, case):
    """The oracle's view of a case, computed once per process and read-only: dict of rest, shapes, A (shapes matrix), QR,
    tau (oracle.morph_qr; for TOP, where the oracle takes 8 s, LAPACK's), P (one frame), w (oracle.morph_weights on QR)."""
    if case.name not in _cache:
        rest, shapes = make(case)
        A = oracle.morph_shapes_matrix(rest, shapes)
        QR, tau = lapack_raw(A) if case.S > 1024 else oracle.morph_qr(A)
        P = frames(case, rest, shapes)[0]
        w = oracle.morph_weights(QR, P, rest)
        for a in [rest, A, QR, tau, P, w] + shapes:
            a.setflags(write=False)
        _cache[case.name] = dict(rest=rest, shapes=shapes, A=A, QR=QR, tau=tau, P=P, w=w)
    return _cache[case.name]
