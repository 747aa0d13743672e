"""CPU: the oracle's dist2 producer (reference src/capture.cpp:46-99) against an independently
formulated numpy computation (tests/golden/make_golden_capture.py).

And, one triangle at a time, against the independent float64 reference of capture_cases.ref_dist2
on well-shaped, degenerate, exactly collinear, sliver and needle triangles.

Bar: |d - ref| <= 1 u, u = 2^-23 (ref + E^2), E the triangle's longest edge: the oracle returns fp32,
so half an ulp of ref is inherent; the walk's own fp64 error is far below that.  And no -1 anywhere
at radius2 = 1e30: a triangle must never drop out of the search (one with a == b did: 0 / 0 in the
edge-AB branch made its distance NaN)."""
import os
import numpy as np
import pytest

import capture_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cap():
    return np.load(os.path.join(HERE, "golden", "capture_golden.npz"))


def test_distances_match_independent_formulation(oracle, cap):
    out = oracle.capture_dist2(cap["P"], cap["tris"], radius2=1e30, dofalloff=True)
    ref = cap["d2"]
    assert np.abs(out - ref).max() <= 1e-6 * max(1.0, ref.max()) and (out >= 0).all()
    assert np.all(out[:150] <= 1e-12)            # points placed on vertices, faces and edges


def test_capture_semantics(oracle, cap):
    P, tris, ref, mask = cap["P"], cap["tris"], cap["d2"], cap["mask"]
    r2 = np.float32(0.09)
    out = oracle.capture_dist2(P, tris, r2, True, mask)
    inside = mask.astype(bool)
    assert np.all(out[~inside] == 0.0)                                   # attribute default (capture.cpp:31)
    near = inside & (ref.astype(np.float32) < r2)
    far = inside & ~(ref.astype(np.float32) < r2)
    assert near.any() and far.any()
    assert np.all(out[far] == -1.0)                                      # nothing within the radius (:76,88)
    assert np.allclose(out[near], ref[near], rtol=1e-6, atol=1e-9)
    assert np.all(oracle.capture_dist2(P, tris, r2, False, mask) == 0.0)   # dofalloff off (:71-75)
    assert np.all(oracle.capture_dist2(P[:10], tris[:0], r2, True) == -1.0)   # no rig surface at all


def _grid_mesh(nx, ny):
    """nx x ny grid in the z = 0 plane with 4-neighbour edges, as a CSR adjacency."""
    idx = np.arange(nx * ny).reshape(ny, nx)
    P = np.stack([np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx), np.zeros(nx * ny)], axis=1).astype(np.float32)
    nbrs = [[] for _ in range(nx * ny)]
    for y in range(ny):
        for x in range(nx):
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < nx and 0 <= y + dy < ny:
                    nbrs[idx[y, x]].append(idx[y + dy, x + dx])
    offsets = np.zeros(nx * ny + 1, np.int64)
    offsets[1:] = np.cumsum([len(n) for n in nbrs])
    return P, offsets, np.concatenate([np.array(n, np.int32) for n in nbrs])


def test_islands_on_a_grid_are_manhattan_balls(oracle):
    """On a 4-connected grid the points within k edges of a seed are its Manhattan ball."""
    P, offsets, nb = _grid_mesh(31, 23)
    rig = np.array([[5.2, 4.9, 0.3], [25.0, 17.6, -0.2]], np.float32)     # nearest grid points (5,5) and (25,18)
    for k in (0, 1, 4):
        mask = oracle.capture_islands(P, offsets, nb, rig, k)
        man = np.minimum(np.abs(P[:, 0] - 5) + np.abs(P[:, 1] - 5), np.abs(P[:, 0] - 25) + np.abs(P[:, 1] - 18))
        assert np.array_equal(mask.astype(bool), man <= k), k
    assert oracle.capture_islands(P, offsets, nb, rig[:0], 3).sum() == 0


# ---- one triangle at a time: well-shaped, degenerate, collinear, sliver, needle ----------------
def test_reference_agrees_with_the_golden_formulation():
    """ref_dist2 (vectorised over triangles) against tri_d2 of tests/golden/make_golden_capture.py on the
    committed golden set, whose d2 that script wrote."""
    g = np.load(os.path.join(HERE, "golden", "capture_golden.npz"))
    ref = cc.ref_dist2(g["P"], g["tris"])
    assert np.all(np.abs(ref - g["d2"]) <= 1e-12 * (g["d2"] + 1.0))


def test_reference_raises_no_warning_and_knows_the_closed_forms():
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    P = np.array([[0.25, 0.25, 2.0], [-3, -4, 0], [2, 0, 0], [0.5, -1, 0], [1, 1, 0], [0.25, 0.25, 0]], np.float32)
    with np.errstate(all="raise"):
        assert np.allclose(cc.ref_dist2(P, tri), [4.0, 25.0, 1.0, 1.0, 0.5, 0.0], rtol=1e-15, atol=0)
        seg = np.array([[0, 0, 0, 0, 0, 0, 2, 0, 0], [5, 5, 5, 5, 5, 5, 5, 5, 5]], np.float32)       # a == b, and a point
        assert np.allclose(cc.ref_dist2(P[:3], seg), [4.0625, 25.0, 0.0], rtol=1e-15, atol=0)
        for c in cc.cases("degenerate") + cc.cases("collinear")[:2]:
            assert np.all(np.isfinite(cc.ref_dist2(c.P, c.tri[None])))


def test_reference_against_exact_rational_arithmetic():
    """ref_dist2 is float64; on slivers its own cancellation has to stay far below the unit it is used to
    measure in.  Sixteen points of every case in exact arithmetic: ten spread over the set, the three
    vertices, one point on an edge and two inside."""
    worst = 0.0
    for f in cc.FAMILIES:
        for c, ref in zip(cc.cases(f), cc.reference(f)):
            idx = np.r_[np.linspace(0, c.P.shape[0] - 1, 10).astype(int), 3200, 3201, 3202, 3250, 3600, 3700]
            ex = np.array([cc.exact_dist2(c.P[i], c.tri) for i in idx])
            worst = max(worst, float(cc.ratio(np.abs(ref[idx] - ex), cc.unit(ex, cc.longest_edge(c.tri))).max()))
    print(f"ref_dist2 vs exact: worst {worst:.2e} u")
    assert worst <= 1e-3


def test_well_shaped_points_reach_every_voronoi_region():
    """A condition on the inputs: at least 100 points in each of the seven regions of every well-shaped
    triangle."""
    for c in cc.cases("well"):
        n = np.bincount(cc.voronoi_region(c.P, c.tri), minlength=7)
        assert n.min() >= 100, (c.label, dict(zip(cc.REGIONS, n)))


def test_point_sets_hold_what_they_promise():
    for c in cc.all_cases():
        assert 3800 <= c.P.shape[0] <= 4600 and c.P.dtype == np.float32 and c.tri.dtype == np.float32
    for f in cc.FAMILIES:
        for c, ref in zip(cc.cases(f), cc.reference(f)):
            E = cc.longest_edge(c.tri) or 0.4
            assert (ref == 0).sum() >= 3                                  # the vertices themselves
            assert (ref <= (1e-6 * E) ** 2).sum() >= 400                  # on the edges and inside, to fp32 rounding
            assert ref.max() >= (3 * E) ** 2 and (ref[ref > (1e-5 * E) ** 2]).min() <= (1e-2 * E) ** 2


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_oracle_against_reference_one_triangle_at_a_time(oracle, family):
    worst, missing, worst_label = 0.0, [], None
    for c, ref in zip(cc.cases(family), cc.reference(family)):
        d = oracle.capture_dist2(c.P, c.tri[None], 1e30, True).astype(np.float64)
        miss = ~(d >= 0)                                                  # -1 and NaN alike
        if miss.any():
            missing.append((c.label, int(miss.sum())))
        r = cc.ratio(np.abs(d - ref), cc.unit(ref, cc.longest_edge(c.tri)))[~miss]
        if r.size and r.max() > worst:
            worst, worst_label = float(r.max()), c.label
    print(f"oracle vs reference, {family}: worst {worst:.3f} u ({worst_label}); points without an answer: {missing}")
    assert not missing, missing
    assert worst <= 1.0, (worst, worst_label)
