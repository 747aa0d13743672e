"""GPU: fd_batch_deform_vectors_shared_ml_dev -- the Jacobian and the vectors it carries for every frame of a shot of
multilayer models in fp32, one matrix-pipe launch (k_vectors32_shared_ml).

Yardsticks, fixed in advance (include/facedeform_hip.h states them):
  * test_gpu_vectors.py's fp64 restatement in numpy (_field) on the oracle's multilayer weights (oracle/fd_oracle.py
    build_multilayer: M L layer-major records), at the one-layer fp32 shot launch's bar, per vertex and frame
        ||A - A_ref||_F <= 2^-22 ||A_ref||_F + 2^-21 f S'
    with t' and n' at test_gpu_vectors_shared._check_frame's bars carried through;
  * the per-context fp32 launches on the same inputs (fd_batch_deform_vectors_shared_dev on the same batch) against THEIR
    bar, 2^-22 ||A_ref||_F + 2^-22 f S' (test_gpu_vectors._check_A): printed, not asserted;
  * P_out and fd_falloff bit-identical to fd_batch_deform_shared_ml_dev in the same run, in both fd_set_output modes.

The grid test prints, for every size and before it asserts, the launch's worst ratio and the per-context launches' own.
Measured on an MI355X: over the grid the launch's worst ratio is 0.343, the per-context launches' own 0.259;
the range cases 0.317 and 0.404."""
import ctypes as C

import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_shared_ml import DEV, GRID as GRID_ML, TERMS, _close, _deltas, _engines, _mesh
from test_gpu_vectors import RADIUS2, RATE, _check_A, _field, _projection, _rotation
from test_gpu_vectors_shared import BAR_ABS, BAR_REL, SENTINEL, _check_frame, _device_inputs
from test_gpu_vectors_shared_fp64 import EYE, _assert_passed_through
from test_gpu_vectors_shared_ml_fp64 import Outs as OutsMl64, _same
from test_vectors_shared_ml_abi import MIN_FRAMES, NAME

pytestmark = pytest.mark.gpu

ML = capi.KERNEL_GAUSSIAN_ML
NEW, CTX, POS = "deform_vectors_shared_ml_dev", "deform_vectors_shared_dev", "deform_shared_ml_dev"
N_GRID = 4099
# test_gpu_shared_ml.py's sizes with its R, lambda and terms (ragged padding, share 1 / 2 / 4, full tiles, several chunks, one
# layer), every one at N = 4099
GRID = [(M, L, F, N_GRID, R, lam, term) for M, L, F, _, R, lam, term in GRID_ML]


class Outs(OutsMl64):
    """test_gpu_vectors_shared_fp64's outputs (N + 64 entries, a sentinel tail on every output), filled by the call named."""
    def call(self, batch, d, proj, dist2=True, stream_ptr=None, N=None, off=0, which=NEW):
        super().call(batch, d, proj, dist2=dist2, stream_ptr=stream_ptr, N=N, off=off, which=which)


def _positions(batch, d, N, F, proj):
    """fd_batch_deform_shared_ml_dev with the same arguments: the bits P_out and fd_falloff must have."""
    Pref = [torch.full((N, 3), float(SENTINEL), device=DEV()) for _ in range(F)]
    fref = [torch.zeros(N, device=DEV()) for _ in range(F)]
    torch.cuda.synchronize()
    getattr(batch, POS)(N, d["P"].data_ptr(), [t.data_ptr() for t in Pref], d_dist2=d["d2"].data_ptr(),
                        d_falloff=[t.data_ptr() for t in fref],
                        d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if proj else None,
                        radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in Pref], [t.cpu().numpy() for t in fref]


def _refs(oracle, rest, deltas, X, R, L, lam, term):
    """(J, S') per frame at the points X: test_gpu_vectors._field on the oracle's M L layer-major records."""
    out = []
    for f in range(deltas.shape[0]):
        # The oracle's table holds the displacement as deformed - rest, and rest + delta is rounded to fp32 on the way in: up
        # to 6e-8 of absolute error in the values the oracle fits, where the device is handed the deltas themselves.  At the
        # smallest radii that is 0.86 / R_l times as much in J (3.2 times the bar at R = 0.0196, for the per-context launches
        # as well), so the table's displacement columns are set to the deltas the device gets, exactly.
        table = oracle.control_table(rest, rest + deltas[f])
        assert np.abs(table[:, 3:6] - deltas[f]).max() <= 2.0 ** -23 * (1.0 + np.abs(rest).max())
        table[:, 3:6] = deltas[f].astype(np.float64)
        tt, table_ml, Wo, radii = oracle.build_multilayer(table, R, L, lam, term)
        assert tt == 1
        n = Wo.shape[0] - 4
        _, J, S = _field(ML, X, table_ml[:, :3], Wo[:n], Wo[n:], radii)
        out.append((J, S))
    return out


def _ratios(outs, f, lv, proj, Pi_all, J, S, tu, tv, Nv, ctx=None):
    """Worst ratio of frame f of the new launch against its bar and, with `ctx`, of the per-context launches against theirs."""
    _, fall, No, tuo, tvo, A = outs.host(f)
    assert np.isfinite(A).all()
    Pi = Pi_all if proj else None
    r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], None, Pi, J, S, tu[lv], tv[lv], Nv[lv])
    rc = 0.0
    if ctx is not None:
        _, cfall, _, _, _, cA = ctx.host(f)
        rc = _check_A(cA[lv], cfall[lv].astype(np.float64), Pi, J, S, capi.EVAL_FP32)
    return r, rc


def _run(oracle, M, L, F, N, R, lam, term, projs=(False, True), per_context=True, modes=True):
    """The new call against the restatement and against the position call's bits (in both fd_set_output modes); returns the
    worst ratios (the launch's against its bar, the per-context launches' against theirs)."""
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == (NAME if F >= MIN_FRAMES[L] else "")
    P = _mesh(N); rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, TERMS[term])
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)            # (a third of the vertices gated, a few exactly on the radius)
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv]) if lv.size else None
    refs = _refs(oracle, rest, deltas, P[lv].astype(np.float64), R, L, lam, TERMS[term]) if lv.size else None
    worst = worst_ctx = 0.0
    for proj in projs:
        outs = Outs(N, F)
        outs.call(batch, d, proj)
        ctx = None
        if per_context:
            ctx = Outs(N, F)
            ctx.call(batch, d, proj, which=CTX)
        Pref, fref = _positions(batch, d, N, F, proj)
        for f in range(F):
            Pg, fall, No, tuo, tvo, A = outs.host(f)                # (host() checks the sentinel tails of every output)
            assert np.array_equal(Pg, Pref[f]) and np.array_equal(fall, fref[f]), f
            _assert_passed_through(outs, f, ~live, tu, tv, Nv)
            z = live & (fall == 0)
            if N >= 97:
                assert z.any()
            _assert_passed_through(outs, f, z, tu, tv, Nv)
            if not lv.size:
                continue
            J, S = refs[f]
            r, rc = _ratios(outs, f, lv, proj, Pi_all, J, S, tu, tv, Nv, ctx)
            worst, worst_ctx = max(worst, r), max(worst_ctx, rc)
            if N >= 97:
                moving = live & (fall != 0)
                assert not np.array_equal(A[moving], np.broadcast_to(EYE, A[moving].shape))
    if modes:
        # the position call's bits in the other fd_set_output mode as well
        for e in engines:
            e.set_output(capi.OUTPUT_DISPLACEMENT)
        outs = Outs(N, F)
        outs.call(batch, d, True)
        Pref, fref = _positions(batch, d, N, F, True)
        for f in range(F):
            Pg, fall = outs.host(f)[:2]
            assert np.array_equal(Pg, Pref[f]) and np.array_equal(fall, fref[f]), f
        for e in engines:
            e.set_output(capi.OUTPUT_POSITION)
    _close(engines, batch)
    print(f"\nvectors shared ml M={M} L={L} F={F} N={N} {term}: worst ratio of the launch against its bar {worst:.3f}; "
          f"of the per-context fp32 launches against theirs {worst_ctx:.3f}")
    return worst, worst_ctx


# ---- 1. accuracy against the bar; 4. positions and fall-off in both output modes ----------------------------------------
@pytest.mark.parametrize("M,L,F,N,R,lam,term", GRID)
def test_restatement_and_position_bits(hip_lib, oracle, M, L, F, N, R, lam, term):
    """(The per-context figure is printed and recorded in DESIGN.md 4.7e, not asserted: it is the one-frame kernel's, whose
    own bar is 1.0; the bar on the new launch is unconditional.)"""
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    r, rc = _run(oracle, M, L, F, N, R, lam, term)
    assert r <= 1.0, (M, L, F, r, rc)


# ---- 2. vertex edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 129])
def test_one_vertex_one_past_a_tile_one_past_a_group(hip_lib, oracle, N):
    r, rc = _run(oracle, 64, 4, 13, N, 0.5, 0.05, "const", per_context=False, modes=False)
    assert r <= 1.0, (N, r)


# ---- 3. row-tile edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 5, 12, 13, 16, 17])
def test_every_row_tile_edge(hip_lib, oracle, F):
    """16-row tiles: one / two tiles (4 | 5), the padded and the dense order (12 | 13), three / six tiles (16 | 17).  Under the
    bar against the restatement, and against the per-context launches within the sum of the two bars (both are within
    their own bar of one reference: 2 x 2^-22 ||A|| + (2^-21 + 2^-22) f S')."""
    M, L, N, R, lam, term = 64, 4, 1500, 0.5, 0.05, "linear"
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, TERMS[term])
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    lv = np.arange(N)[~(dist2 > RADIUS2)]
    Pi = _projection(tu[lv], tv[lv], nrm[lv])
    refs = _refs(oracle, rest, deltas, P[lv].astype(np.float64), R, L, lam, TERMS[term])
    outs, ctx = Outs(N, F), Outs(N, F)
    outs.call(batch, d, True)
    ctx.call(batch, d, True, which=CTX)
    torch.cuda.synchronize()            # (the calls run on the contexts' stream, host() copies on torch's)
    worst = 0.0
    for f in range(F):
        J, S = refs[f]
        r, _ = _ratios(outs, f, lv, True, Pi, J, S, tu, tv, Nv)
        worst = max(worst, r)
        _, fall, _, _, _, A = outs.host(f)
        cA = ctx.host(f)[5]
        fl = fall[lv].astype(np.float64)
        Aref = np.eye(3)[None] + fl[:, None, None] * (Pi @ J)
        both = 2 * BAR_REL * np.linalg.norm(Aref, axis=(1, 2)) + (BAR_ABS + 2.0 ** -22) * fl * S
        assert (np.linalg.norm(A[lv].astype(np.float64) - cA[lv], axis=(1, 2)) <= both).all(), (F, f)
        assert not np.array_equal(A[lv], np.broadcast_to(EYE, A[lv].shape))
    print(f"\nvectors shared ml row tiles F={F}: worst ratio {worst:.3f}")
    assert worst <= 1.0, (F, worst)
    _close(engines, batch)


# ---- 5. pass-through ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 20])
def test_gated_vertices_zero_falloff_and_a_frame_on_another_rig_pass_through(hip_lib, oracle, F):
    """The last frame is built on other rest points than frame 0 (the rest array rewritten between two builds, as in
    test_gpu_vectors_shared.py): the pack kernel's frame record says so, and its vectors come out bit for bit with A = I at
    every vertex, P_out = P_in.  In the other frames the gated vertices and those with f = 0 pass through, the rest meet the
    bar.  host() checks the sentinel tails of 64 entries on every output."""
    M, L, N, R, lam = 64, 4, 2000, 1.0, 0.1
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    other = (rest * np.float32(1.01)).astype(np.float32)
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, build=False)
    head, lone = capi.Batch(engines[:-1]), capi.Batch([engines[-1]])
    d_rest, d_del = keep
    head.set_points_dev([d_rest.data_ptr()] * (F - 1), [d_del[k].data_ptr() for k in range(F - 1)], M)
    head.build_async(); assert [r.terminationtype for r in head.build_result()] == [1] * (F - 1)
    d_rest.copy_(torch.from_numpy(other).to(DEV()))               # the same array, another rig
    torch.cuda.synchronize()
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(); assert lone.build_result()[0].terminationtype == 1
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, True)                                     # same address everywhere: accepted by the host
    torch.cuda.synchronize()
    assert np.array_equal(outs.host(F - 1)[0], P)
    _assert_passed_through(outs, F - 1, np.ones(N, bool), tu, tv, Nv)
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    Pi = _projection(tu[lv], tv[lv], nrm[lv])
    refs = _refs(oracle, rest, deltas[:F - 1], P[lv].astype(np.float64), R, L, lam, capi.TERM_LINEAR)
    for f in range(F - 1):
        fall = outs.host(f)[1]
        _assert_passed_through(outs, f, ~live, tu, tv, Nv)
        z = live & (fall == 0)
        assert z.any()
        _assert_passed_through(outs, f, z, tu, tv, Nv)
        J, S = refs[f]
        r, _ = _ratios(outs, f, lv, True, Pi, J, S, tu, tv, Nv)
        assert r <= 1.0, (f, r)
        assert not np.array_equal(outs.host(f)[5][lv], np.broadcast_to(EYE, (lv.size, 3, 3)))
    _close(engines, head, lone, batch)


# ---- 6. range -----------------------------------------------------------------------------------------------------------
def _range_points(rest, R, L, n_each=200):
    """Vertices on the centres, next to them and far from them.  Among those next to them is the ring d = R_finest / sqrt 2,
    R_finest = R / 2^(L - 1), on which the finest layer's basis |g (x' - c')| has its maximum: the point at which a radius
    limit stated too small would overflow first."""
    rng = np.random.default_rng(11)
    c = rest[rng.integers(0, rest.shape[0], n_each)]
    u = rng.normal(size=(n_each, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    peak = R / 2.0 ** (L - 1) / np.sqrt(2.0)
    parts = [c] + [c + np.float32(s) * u.astype(np.float32) for s in (peak, R / 181.0, R / 128.0, R / 16.0, R / np.sqrt(2.0), 3.0 * R, 40.0 * R)]
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


@pytest.mark.parametrize("case", ["deepest_of_the_grid", "four_layers_at_the_limit"])
def test_range_of_the_basis(hip_lib, oracle, case):
    """The fp16 basis 2^8 g (x' - c') is finite down to a finest-layer radius of 0.00245 rig radii (the header's limit:
    2^8 0.5151 sqrt(log2 e) / R' <= 65504 from R' = 0.00242 on).  deepest_of_the_grid: (33, 8) at R = 0.7, finest radius
    R / 128.  four_layers_at_the_limit: the smallest base radius the limit allows for 4 layers, 0.00245 x 8 rig radii, the
    rig radius formed as the build forms it (fd_pack.h: the largest distance of a centre from the centroid -- from the
    origin where the centroid is within a sixteenth of it -- rounded to a power of two)."""
    F, lam, term = 5, 0.1, "linear"
    if case == "deepest_of_the_grid":
        M, L, R = 33, 8, 0.7
        rest = synth.control_points(M, "head")
    else:
        M, L = 64, 4
        rest = synth.control_points(M, "head")
        c = rest.astype(np.float64)
        rad_c, rad_o = np.linalg.norm(c - c.mean(0), axis=1).max(), np.linalg.norm(c, axis=1).max()
        rad = rad_c if np.linalg.norm(c.mean(0)) > rad_c * 0.0625 else rad_o
        R = 0.00245 * 2 ** (L - 1) * 2.0 ** np.rint(np.log2(rad))
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _range_points(rest, R, L)
    N = P.shape[0]
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, TERMS[term])
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    lv = np.arange(N)[~(dist2 > RADIUS2)]
    refs = _refs(oracle, rest, deltas, P[lv].astype(np.float64), R, L, lam, TERMS[term])
    outs, ctx = Outs(N, F), Outs(N, F)
    outs.call(batch, d, False)
    ctx.call(batch, d, False, which=CTX)
    torch.cuda.synchronize()
    worst = worst_ctx = 0.0
    for f in range(F):
        J, S = refs[f]
        r, rc = _ratios(outs, f, lv, False, None, J, S, tu, tv, Nv, ctx)    # (asserts every A finite)
        worst, worst_ctx = max(worst, r), max(worst_ctx, rc)
        assert not np.array_equal(outs.host(f)[5][lv], np.broadcast_to(EYE, (lv.size, 3, 3)))
    print(f"\nvectors shared ml range {case}: R = {R:.5f}, worst ratio {worst:.3f}; the per-context fp32 launches against theirs {worst_ctx:.3f}")
    assert worst <= 1.0, (case, worst)
    _close(engines, batch)


# ---- 7. rigid motion ----------------------------------------------------------------------------------------------------
def test_rigid_motion_gives_the_rotation(hip_lib):
    """Linear term, every frame a rigidly moved rig: the polynomial reproduces the motion, the layers fit a zero residual,
    A = R_f and N_out = R_f N for every frame to 1e-5 (test_gpu_vectors_shared.py's analogue takes no lambda: thin-plate;
    here the model's lambda = 0.1 stands -- the residual the layers see is zero whatever it is)."""
    M, L, F, N = 64, 4, 5, 2000
    rest = synth.control_points(M, "head")
    P = _mesh(N)
    p0 = np.array([0.4, -0.3, 0.25])
    Rs = [_rotation(0.05 + 0.04 * f, [0.3, 1.0 - 0.2 * f, -0.2]) for f in range(F)]
    deltas = np.stack([((rest.astype(np.float64) - p0) @ R.T + p0 - rest).astype(np.float32) for R in Rs])
    engines, batch, keep = _engines(M, L, F, rest, deltas, 1.0, 0.1)
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    (tu, tv, nrm, Nv, _), d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, False, dist2=False)
    torch.cuda.synchronize()
    for f in range(F):
        _, _, No, _, _, A = outs.host(f)
        print(f"rigid motion frame {f}: |A - R| {np.abs(A - Rs[f][None]).max():.2e}, |N' - R N| {np.abs(No - Nv.astype(np.float64) @ Rs[f].T).max():.2e}")
        assert np.abs(A - Rs[f][None]).max() <= 1e-5, f
        assert np.abs(No - Nv.astype(np.float64) @ Rs[f].T).max() <= 1e-5, f
    _close(engines, batch)


# ---- 8. bits ------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_in_two_ranges_and_on_fewer_cus(hip_lib):
    N, M, L, F, cut = 1500, 96, 6, 17, 700                     # (700 is no multiple of 16)
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    _, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), 0.7, 0.1)
    one, again, two, few = Outs(N, F), Outs(N, F), Outs(N, F), Outs(N, F)
    one.call(batch, d, True)
    again.call(batch, d, True)
    two.call(batch, d, True, N=cut)
    two.call(batch, d, True, N=N - cut, off=cut)
    batch.set_eval_cus(8)
    few.call(batch, d, True)
    batch.set_eval_cus(0)
    torch.cuda.synchronize()
    assert not np.array_equal(one.host(0)[5], np.broadcast_to(EYE, (N, 3, 3)))
    for other in (again, two, few):
        _same(one, other, F)
    _close(engines, batch)


# ---- 9. consumed --------------------------------------------------------------------------------------------------------
def test_rebuild_behind_wait_consumed(hip_lib):
    """The call on one stream, fd_batch_wait_consumed on a second, new deltas and a rebuild there while the launches are in
    flight: the outputs equal those of the same call without the rebuild."""
    N, M, L, F = 50_000, 64, 4, 16
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    sA, sB = torch.cuda.Stream(device=DEV()), torch.cuda.Stream(device=DEV())
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), stream=sA.cuda_stream)
    _, d = _device_inputs(P)
    other = torch.from_numpy(_deltas(rest, F, flip=True)).to(DEV())
    quiet, raced = Outs(N, F), Outs(N, F)
    quiet.call(batch, d, True, stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    raced.call(batch, d, True, stream_ptr=sA.cuda_stream)
    batch.wait_consumed(sB.cuda_stream)
    batch.set_points_dev([keep[0].data_ptr()] * F, [other.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(sB.cuda_stream)
    torch.cuda.synchronize()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    _same(quiet, raced, F)                                              # the first models' outputs
    after = Outs(N, F)
    after.call(batch, d, True, stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    assert not np.array_equal(after.host(0)[5], quiet.host(0)[5])          # and now the second models'
    _close(engines, batch)


# ---- 10. delegation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["thin_plate", "qnn", "ml_fp64", "ml_eval_variant", "ml_one_frame", "ml_nine_layers"])
def test_everything_else_is_the_one_layer_call_bit_for_bit(hip_lib, case):
    N, M, L = 1500, 64, 4
    F = 1 if case == "ml_one_frame" else 5
    P = _mesh(N); rest = synth.control_points(M, "head")
    _, d = _device_inputs(P)
    kw = {"thin_plate": dict(kind=capi.KERNEL_THIN_PLATE, params=[]), "qnn": dict(kind=capi.KERNEL_GAUSSIAN_QNN, params=[1.0, 5.0]),
          "ml_fp64": dict(precision=capi.EVAL_FP64), "ml_eval_variant": dict(variant=2), "ml_one_frame": {}, "ml_nine_layers": {}}[case]
    if case == "ml_nine_layers":
        # no context can hold such a model: fd_set_kernel refuses more than 8 layers, so the delegation of "layer counts
        # outside 1..8" has no batch to act on; what is left of it is the name query's answer
        assert capi.fd_shared_vectors_ml_kernel_name(M, 9, F) == "" and capi.fd_shared_vectors_ml_kernel_name(M, 0, F) == ""
        e = capi.Engine()
        with pytest.raises(capi.FdError):
            e.set_kernel(ML, [1.0, 9, 0.1])
        e.close()
        return
    if case == "ml_one_frame":
        assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == ""
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), **kw)
    before, new, after = Outs(N, F), Outs(N, F), Outs(N, F)
    before.call(batch, d, True, which=CTX)
    new.call(batch, d, True)
    after.call(batch, d, True, which=CTX)                           # ... and the existing call after it is unaffected
    torch.cuda.synchronize()
    assert not np.array_equal(before.host(0)[5], np.broadcast_to(EYE, (N, 3, 3)))
    _same(before, new, F); _same(before, after, F)
    _close(engines, batch)


def test_below_the_vector_threshold_the_vectors_are_the_per_context_launches(hip_lib):
    """A multilayer batch the position launch takes, of fewer frames than the measured vector threshold: positions
    fd_batch_deform_shared_ml_dev's, vectors what fd_deform_vectors_dev writes per context, bit for bit.  (A layer count
    whose threshold is the position launch's own two frames has no such batch: the name query says so.)"""
    N, M = 1500, 64
    ran = 0
    for L in range(1, 9):
        F = MIN_FRAMES[L] - 1
        assert capi.fd_shared_vectors_ml_kernel_name(M, L, MIN_FRAMES[L]) == NAME
        if capi.fd_shared_ml_kernel_name(M, L, F) == "" or ran >= 2:
            continue
        ran += 1
        assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == ""
        P = _mesh(N); rest = synth.control_points(M, "head")
        _, d = _device_inputs(P)
        engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
        outs = Outs(N, F)
        outs.call(batch, d, True)
        Pref, fref = _positions(batch, d, N, F, True)
        for f, e in enumerate(engines):
            ref = Outs(N, 1)
            e.deform_vectors_dev(N, d["P"].data_ptr(), ref.P[0].data_ptr(), d["d2"].data_ptr(), ref.fall[0].data_ptr(),
                                 d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr(), d["Nv"].data_ptr(), ref.No[0].data_ptr(),
                                 d["tu"].data_ptr(), ref.tuo[0].data_ptr(), d["tv"].data_ptr(), ref.tvo[0].data_ptr(), ref.A[0].data_ptr(),
                                 radius2=RADIUS2, falloffrate=RATE)
            torch.cuda.synchronize()
            got, want = outs.host(f), ref.host(0)
            assert np.array_equal(got[0], Pref[f]) and np.array_equal(got[1], fref[f])
            for a, b in zip(got[2:], want[2:]):
                assert np.array_equal(a, b), (L, f)
            assert not np.array_equal(got[5], np.broadcast_to(EYE, (N, 3, 3)))
        _close(engines, batch)


def _raw(batch, outs, d, N, **over):
    """The C call itself, with the tables and the struct built here."""
    vp = C.c_void_p
    n = len(outs.P)
    tab = lambda ts: None if ts is None else (vp * n)(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])
    a = dict(P_in=d["P"].data_ptr(), P_out=outs.P, d2=d["d2"].data_ptr(), fall=outs.fall, tu=d["tu"].data_ptr(), tv=d["tv"].data_ptr(),
             nrm=d["nrm"].data_ptr(), size=C.sizeof(capi.FdBatchVectors), vN=d["Nv"].data_ptr(), No=outs.No, vtu=d["tu"].data_ptr(),
             tuo=outs.tuo, vtv=d["tv"].data_ptr(), tvo=outs.tvo, jac=outs.A, N=N, vec=True)
    a.update(over)
    vec = capi.FdBatchVectors(a["size"], vp(a["vN"]), tab(a["No"]), vp(a["vtu"]), tab(a["tuo"]), vp(a["vtv"]), tab(a["tvo"]), tab(a["jac"]))
    return capi.load().fd_batch_deform_vectors_shared_ml_dev(batch.h, None, a["N"], vp(a["P_in"]), tab(a["P_out"]), vp(a["d2"]), tab(a["fall"]),
                                                             vp(a["tu"]), vp(a["tv"]), vp(a["nrm"]), RADIUS2, RATE,
                                                             C.byref(vec) if a["vec"] else None)


def test_without_vectors_it_is_the_position_call(hip_lib):
    N, M, L, F = 1500, 64, 4, max(5, MIN_FRAMES[4])
    P = _mesh(N); rest = synth.control_points(M, "head")
    _, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    Pref, fref = _positions(batch, d, N, F, True)
    for how in (dict(vec=False), dict(vN=None, No=None, vtu=None, tuo=None, vtv=None, tvo=None, jac=None)):
        outs = Outs(N, F)
        assert _raw(batch, outs, d, N, **how) == capi.FD_OK
        torch.cuda.synchronize()
        for f in range(F):
            Pg, fall, No, tuo, tvo, A = outs.host(f)
            assert np.array_equal(Pg, Pref[f]) and np.array_equal(fall, fref[f])
            for t in (No, tuo, tvo, A):
                assert (t == SENTINEL).all()                          # no vector output written
    _close(engines, batch)


# ---- 11. argument errors ------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(hip_lib):
    N, M, L, F = 500, 64, 4, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    one = capi.Batch(engines[:1])
    _, d = _device_inputs(P)
    outs, outs1 = Outs(N, F), Outs(N, 1)
    for t in outs.fall + outs1.fall:
        t.fill_(float(SENTINEL))
    torch.cuda.synchronize()
    shared = [d[k].data_ptr() for k in ("P", "d2", "tu", "tv", "nrm", "Nv")]
    for table, ts in (("P_out", outs.P), ("fall", outs.fall), ("No", outs.No), ("tuo", outs.tuo), ("tvo", outs.tvo), ("jac", outs.A)):
        for s in shared:                                                    # every aliasing pair (N_out == d_nrm among them)
            assert _raw(batch, outs, d, N, **{table: [ts[0], s, ts[2]]}) == capi.FD_E_INVALID, (table, s)
        assert _raw(batch, outs, d, N, **{table: [ts[0], None, ts[2]]}) == capi.FD_E_INVALID, table          # a NULL table entry
    for s in shared:
        assert _raw(one, outs1, d, N, P_out=[s]) == capi.FD_E_INVALID      # a batch of one in place, and over any other input
    assert _raw(one, outs1, d, N, No=[d["nrm"].data_ptr()]) == capi.FD_E_INVALID
    assert _raw(batch, outs, d, N, size=C.sizeof(capi.FdBatchVectors) - 8) == capi.FD_E_INVALID          # a short struct_size
    assert _raw(batch, outs, d, N, No=None) == capi.FD_E_INVALID           # an input without its output table
    assert _raw(batch, outs, d, N, vtu=None) == capi.FD_E_INVALID          # an output table without its input
    assert _raw(batch, outs, d, 0) == capi.FD_OK
    torch.cuda.synchronize()
    for o in (outs, outs1):
        for ts in (o.P, o.fall, o.No, o.tuo, o.tvo, o.A):
            for t in ts:
                assert bool((t == float(SENTINEL)).all())                   # nothing was written
    one.close()
    _close(engines, batch)


# ---- 12. the seven other calls ------------------------------------------------------------------------------------------
def test_the_other_shared_calls_between_two_launches_change_nothing(hip_lib):
    """The new call, then the seven other shared calls on the same batch, then the new call again: the same bits, and the
    launch is not the per-context launch (other bits somewhere)."""
    N, M, L, F = 1500, 64, 4, 13
    assert capi.fd_shared_vectors_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    _, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    new, again = Outs(N, F), Outs(N, F)
    new.call(batch, d, True)
    pos_kw = dict(d_dist2=d["d2"].data_ptr(), d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()),
                  radius2=RADIUS2, falloffrate=RATE)
    others = {}
    for which in ("deform_shared_dev", "deform_shared_fp64_dev", "deform_shared_ml_dev", "deform_shared_ml_fp64_dev"):
        o = Outs(N, F)
        getattr(batch, which)(N, d["P"].data_ptr(), [t.data_ptr() for t in o.P], d_falloff=[t.data_ptr() for t in o.fall], **pos_kw)
        others[which] = o
    for which in ("deform_vectors_shared_dev", "deform_vectors_shared_fp64_dev", "deform_vectors_shared_ml_fp64_dev"):
        o = Outs(N, F)
        o.call(batch, d, True, which=which)
        others[which] = o
    again.call(batch, d, True)
    torch.cuda.synchronize()
    _same(new, again, F)
    # ... and the position launch this call runs first is untouched by the vector launch behind it
    for f in range(F):
        a, b = new.host(f), others["deform_shared_ml_dev"].host(f)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ctx = others["deform_vectors_shared_dev"]
    assert any(not np.array_equal(new.host(f)[5], ctx.host(f)[5]) for f in range(F))
    _close(engines, batch)
