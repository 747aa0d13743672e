"""Shared inputs for the dist2 producer's tests (fd_capture_dist2*, fdo_capture_dist2): an independent
float64 reference and seeded families of single triangles -- well-shaped, degenerate, exactly
collinear, slivers, needles -- each with a point set that reaches every part of the triangle.

A plain module (no fixture): `from capture_cases import ...`.  Everything is deterministic.

Reference: the squared distance to the closed triangle as a point set -- the minimum of the three
segment distances and, where the normal is non-zero and the point projects inside, the plane
distance.  The formulation of tests/golden/make_golden_capture.py, not the Voronoi-region walk the
oracle and the kernel take, so an error the two share shows.

Unit: u = 2^-23 (ref + E^2) with E the longest edge among the triangles of the call.  It does not
move with a translation of the scene, unlike a bound built on max |coordinate|."""
import functools
from collections import namedtuple

import numpy as np

SEED = 20261019
DECADES = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)
COLLINEAR_S = (-0.7, 0.5, 2.0, 37.0)
PER_DECADE = 6
PER_S = 4
REGIONS = ("A", "B", "C", "AB", "AC", "BC", "face")

Case = namedtuple("Case", "family label tri P")          # tri (9,) float32, P (n, 3) float32


# ---- reference -------------------------------------------------------------------------------
def _dot(u, v):
    return np.einsum("...k,...k->...", u, v)


def _seg_d2(p, a, b):
    """p (n, 3), a and b (t, 1, 3) -> (t, n) squared distances to the segments a-b."""
    ab = b - a
    den = _dot(ab, ab)                                            # (t, 1)
    ok = den > 0
    t = np.where(ok, _dot(p - a, ab) / np.where(ok, den, 1.0), 0.0)
    q = p - a - np.clip(t, 0.0, 1.0)[..., None] * ab
    return _dot(q, q)


def ref_dist2(P, tris, chunk=64):
    """float32 P (n, 3) and tris (t, 9) as the engine is given them, widened to float64 ->
    (n,) float64 squared distance to the nearest triangle."""
    P = np.asarray(P, np.float32).reshape(-1, 3).astype(np.float64)
    tris = np.asarray(tris, np.float32).reshape(-1, 9).astype(np.float64)
    best = np.full(P.shape[0], np.inf)
    p = P[None]
    for t0 in range(0, tris.shape[0], chunk):
        t = tris[t0:t0 + chunk]
        a, b, c = t[:, None, 0:3], t[:, None, 3:6], t[:, None, 6:9]
        d = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
        n = np.cross(b - a, c - a)                                # (t, 1, 3)
        nn = _dot(n, n)                                           # (t, 1)
        flat = nn > 0
        if flat.any():
            h = _dot(p - a, n)                                    # (t, n): signed distance * |n|
            inside = (flat & (_dot(np.cross(b - a, p - a), n) >= 0) & (_dot(np.cross(c - b, p - b), n) >= 0)
                      & (_dot(np.cross(a - c, p - c), n) >= 0))
            plane = h * h / np.where(flat, nn, 1.0)
            d = np.where(inside, np.minimum(d, plane), d)
        best = np.minimum(best, d.min(axis=0))
    return best


def longest_edge(tris):
    """Longest edge among the triangles (float32 (t, 9)), in float64."""
    t = np.asarray(tris, np.float32).reshape(-1, 9).astype(np.float64)
    a, b, c = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    e2 = np.maximum(np.maximum(_dot(b - a, b - a), _dot(c - a, c - a)), _dot(c - b, c - b))
    return float(np.sqrt(e2.max())) if e2.size else 0.0


def unit(ref, E):
    """u = 2^-23 (ref + E^2)."""
    return 2.0 ** -23 * (np.asarray(ref, np.float64) + E * E)


def bar(ref, E):
    """The device bar: 2e-6 (ref + E^2) = 16.8 u."""
    return 2e-6 * (np.asarray(ref, np.float64) + E * E)


def ratio(err, allowed):
    """err / allowed element by element with 0 / 0 = 0 (an exact answer under a zero allowance passes) and
    NaN -> inf (no answer never passes)."""
    err, allowed = np.asarray(err, np.float64), np.asarray(allowed, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allowed)
    return np.where(np.isnan(r), np.inf, r)


def exact_dist2(p, tri):
    """The same definition in exact rational arithmetic for one point (slow: a pin for ref_dist2)."""
    from fractions import Fraction as F
    p = [F(float(x)) for x in np.asarray(p, np.float32)]
    a, b, c = ([F(float(x)) for x in np.asarray(tri, np.float32)[k:k + 3]] for k in (0, 3, 6))
    dot = lambda u, v: sum(x * y for x, y in zip(u, v))
    sub = lambda u, v: [x - y for x, y in zip(u, v)]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

    def seg(u, v):
        d = sub(v, u)
        t = min(max(dot(sub(p, u), d) / dot(d, d), F(0)), F(1)) if dot(d, d) else F(0)
        q = sub(sub(p, u), [t * x for x in d])
        return dot(q, q)

    best = min(seg(a, b), seg(b, c), seg(c, a))
    n = cross(sub(b, a), sub(c, a))
    if dot(n, n) > 0 and all(dot(cross(sub(v, u), sub(p, u)), n) >= 0 for u, v in ((a, b), (b, c), (c, a))):
        best = min(best, dot(sub(p, a), n) ** 2 / dot(n, n))
    return float(best)


def voronoi_region(P, tri):
    """float64 classification of points into the seven Voronoi regions of one (well-shaped) triangle:
    indices into REGIONS."""
    p = np.asarray(P, np.float32).astype(np.float64)
    t = np.asarray(tri, np.float32).astype(np.float64)
    a, b, c = t[0:3], t[3:6], t[6:9]
    ab, ac = b - a, c - a
    d1, d2 = (p - a) @ ab, (p - a) @ ac
    d3, d4 = (p - b) @ ab, (p - b) @ ac
    d5, d6 = (p - c) @ ab, (p - c) @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    reg = np.full(p.shape[0], 6)
    todo = np.ones(p.shape[0], bool)
    for code, cond in ((0, (d1 <= 0) & (d2 <= 0)), (1, (d3 >= 0) & (d4 <= d3)), (3, (vc <= 0) & (d1 >= 0) & (d3 <= 0)),
                       (2, (d6 >= 0) & (d5 <= d6)), (4, (vb <= 0) & (d2 >= 0) & (d6 <= 0)),
                       (5, (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))):
        take = todo & cond
        reg[take] = code
        todo &= ~take
    return reg


# ---- point sets ------------------------------------------------------------------------------
def _unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perpendicular(rng, d):
    n = np.cross(d, rng.normal(size=3))
    return n / np.linalg.norm(n)


def point_set(tri, rng, axis=False, n_random=3200, nominal=0.4):
    """About 4000 float32 points for one triangle: random points 1e-3 E ... 10 E from random points of
    the triangle, the three vertices exactly, points on each edge and in the interior, and with
    `axis` points along and beside the longest edge's line."""
    t = np.asarray(tri, np.float32).astype(np.float64)
    a, b, c = t[0:3], t[3:6], t[6:9]
    E = longest_edge(tri) or nominal

    def on_triangle(n):
        u = rng.random((n, 2))
        flip = u.sum(axis=1) > 1
        u[flip] = 1 - u[flip]
        return a + u[:, :1] * (b - a) + u[:, 1:] * (c - a)

    dist = E * 10.0 ** rng.uniform(-3, 1, size=(n_random, 1))
    parts = [on_triangle(n_random) + dist * _unit_vectors(rng, n_random), a[None], b[None], c[None]]
    for u, v in ((a, b), (b, c), (c, a)):
        parts.append(u + rng.random((100, 1)) * (v - u))
    parts.append(on_triangle(300))
    if axis:
        u, v = max(((a, b), (b, c), (c, a)), key=lambda e: _dot(e[1] - e[0], e[1] - e[0]))
        d = (v - u) if _dot(v - u, v - u) > 0 else np.array([nominal, 0.0, 0.0])
        parts.append(u + rng.uniform(-2, 3, size=(200, 1)) * d)
        side = np.cross(d / np.linalg.norm(d), _unit_vectors(rng, 300))
        parts.append(u + rng.uniform(-2, 3, size=(300, 1)) * d + E * 10.0 ** rng.uniform(-4, 0, size=(300, 1)) * side)
    return np.concatenate(parts).astype(np.float32)


# ---- families --------------------------------------------------------------------------------
def _tri(a, b, c):
    return np.concatenate([a, b, c]).astype(np.float32)


def _well_shaped(rng):
    out = []
    for label, angle, lb, lc in (("acute", 65.0, 0.4, 0.37), ("right", 90.0, 0.4, 0.3), ("obtuse150", 150.0, 0.4, 0.3)):
        a = rng.normal(size=3) * 0.3
        e1 = _unit_vectors(rng, 1)[0]
        e2 = _perpendicular(rng, e1)
        th = np.deg2rad(angle)
        tri = _tri(a, a + lb * e1, a + lc * (np.cos(th) * e1 + np.sin(th) * e2))
        out.append(Case("well", label, tri, point_set(tri, rng)))
    return out


def _degenerate(rng):
    a, b, c = np.array([0.1, 0.2, -0.3]), np.array([0.5, -0.1, 0.2]), np.array([-0.2, 0.4, 0.3])
    out = []
    for label, tri in (("a==b", _tri(a, a, c)), ("a==c", _tri(a, b, a)), ("b==c", _tri(a, b, b)), ("a==b==c", _tri(a, a, a))):
        out.append(Case("degenerate", label, tri, point_set(tri, rng, axis=True)))
    return out


def _collinear(rng):
    """c = a + s ab exactly: a on a 2^-12 grid and ab on a 10 * 2^-12 grid, so that b and c (s in tenths)
    are short dyadic numbers that fp32 holds exactly."""
    out = []
    for s in COLLINEAR_S:
        for k in range(PER_S):
            a = rng.integers(-2048, 2049, size=3) / 4096.0
            m = rng.integers(-100, 101, size=3)
            m[np.argmax(np.abs(m))] = rng.choice([-1, 1]) * rng.integers(60, 101)     # |ab| between 0.15 and 0.42
            ab = 10.0 * m / 4096.0
            tri = _tri(a, a + ab, a + s * ab)
            t64 = tri.astype(np.float64)
            assert np.array_equal(t64[3:6], a + ab) and np.array_equal(t64[6:9], a + round(10 * s) * m / 4096.0)
            assert not np.cross(t64[3:6] - t64[0:3], t64[6:9] - t64[0:3]).any()
            out.append(Case("collinear", f"s={s:g}#{k}", tri, point_set(tri, rng, axis=True)))
    return out


def _slivers(rng):
    """Third vertex at a + s ab + eps |ab| n: height eps |ab| over a base |ab|.  s in [-1, 2] puts each of
    the three vertices in the middle in turn."""
    out = []
    for eps in DECADES:
        for k in range(PER_DECADE):
            a = rng.normal(size=3) * 0.5
            ab = rng.normal(size=3) * 0.4
            ab *= max(1.0, 0.15 / np.linalg.norm(ab))
            s = rng.uniform(-1, 2)
            tri = _tri(a, a + ab, a + s * ab + eps * np.linalg.norm(ab) * _perpendicular(rng, ab))
            out.append(Case("sliver", f"eps={eps:g}#{k}", tri, point_set(tri, rng, axis=True)))
    return out


def _needles(rng):
    """c = b + eps |ab| n; the vertex order is rotated from one triangle to the next, so that the short
    edge is bc, ca and ab in turn."""
    out = []
    for eps in DECADES:
        for k in range(PER_DECADE):
            a = rng.normal(size=3) * 0.5
            ab = rng.normal(size=3) * 0.4
            ab *= max(1.0, 0.15 / np.linalg.norm(ab))
            v = [a, a + ab, a + ab + eps * np.linalg.norm(ab) * _perpendicular(rng, ab)]
            tri = _tri(v[k % 3], v[(k + 1) % 3], v[(k + 2) % 3])
            out.append(Case("needle", f"eps={eps:g}#{k}", tri, point_set(tri, rng, axis=True)))
    return out


FAMILIES = ("well", "degenerate", "collinear", "sliver", "needle")


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family, built once; the arrays are read-only."""
    make = {"well": _well_shaped, "degenerate": _degenerate, "collinear": _collinear, "sliver": _slivers, "needle": _needles}
    out = make[family](np.random.default_rng([SEED, FAMILIES.index(family)]))
    for c in out:
        c.tri.setflags(write=False)
        c.P.setflags(write=False)
    return tuple(out)


def all_cases():
    return tuple(c for f in FAMILIES for c in cases(f))


@functools.lru_cache(maxsize=None)
def reference(family):
    """ref_dist2 of every case of a family against its own triangle (T = 1), computed once."""
    out = tuple(ref_dist2(c.P, c.tri[None]) for c in cases(family))
    for r in out:
        r.setflags(write=False)
    return out


def moved(case, offset=0.0, scale=1.0):
    """The case translated and scaled in fp32: the reference is then taken from these arrays, so it sees
    what the kernel sees."""
    f = np.float32
    return Case(case.family, f"{case.label} x{scale:g}+{offset:g}", (case.tri * f(scale) + f(offset)).astype(f),
                (case.P * f(scale) + f(offset)).astype(f))


def decoys(tri, n, rng, factor=3.0):
    """n ordinary triangles (edges about E) whose every point is at least factor * E from every point of
    `tri` -- and from a point at distance below E of it there is still 2 E of margin."""
    t = np.asarray(tri, np.float32).astype(np.float64)
    E = longest_edge(tri) or 0.4
    centre = (t[0:3] + t[3:6] + t[6:9]) / 3.0
    out = np.empty((n, 9), np.float32)
    for i in range(n):
        # |x - centre| >= (factor + 2) E for the decoy's vertices (edges <= E, so all of it is beyond
        # (factor + 1) E of the centre, and the triangle lies within E of its centre)
        o = centre + _unit_vectors(rng, 1)[0] * E * rng.uniform(factor + 3.0, factor + 6.0)
        e1 = _unit_vectors(rng, 1)[0]
        e2 = _perpendicular(rng, e1)
        out[i] = _tri(o, o + 0.9 * E * rng.uniform(0.6, 1.0) * e1, o + 0.9 * E * rng.uniform(0.6, 1.0) * (0.3 * e1 + 0.8 * e2))
    return out
