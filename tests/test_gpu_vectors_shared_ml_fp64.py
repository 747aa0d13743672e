"""GPU: fd_batch_deform_vectors_shared_ml_fp64_dev -- the Jacobian and the vectors it carries for every frame of a shot of
multilayer models in fp64, one matrix-pipe launch (k_vectors64_shared_ml).

Yardsticks, fixed in advance (include/facedeform_hip.h states them):
  * test_gpu_vectors.py's fp64 restatement in numpy on the layer-major records of fd_get_weights, at the project's fp64 bar:
        ||A - A_ref||_F <= 2^-22 ||A_ref||_F + 1e-12 f S'
    t' and n' at test_gpu_vectors_shared_fp64._check_frame's bars;
  * the per-context fp64 launches (fd_batch_deform_vectors_shared_fp64_dev on the same batch: k_vectors64_gaussian over the
    M L records, once per context):
        ||A - A_ctx||_F <= 2^-23 ||A_ctx||_F + (104 + 2 M L) 2^-53 f S'
    -- 96 for the chain, 8 for the products' associations on both sides, M L per side for the summation order;
  * P_out and fd_falloff bit-identical to fd_batch_deform_shared_ml_fp64_dev in the same run, in both fd_set_output modes.

The grid test prints the worst ratios -- the launch's and the per-context launches' own against the restatement -- before it
asserts.  Measured on an MI355X over the grid and the vertex edges: 0.247 against the restatement, the per-context launches'
own 0.247, and every A bit-identical to theirs (ratio 0.000)."""
import ctypes as C

import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_shared_ml import DEV, TERMS, _close, _deltas, _engines, _mesh
from test_gpu_vectors import RADIUS2, RATE, _field, _model, _projection
from test_gpu_vectors_shared import SENTINEL, _device_inputs
from test_gpu_vectors_shared_fp64 import BAR_FRAME, EYE, Outs as Outs64, _assert_passed_through, _check_frame
from test_vectors_shared_ml_fp64_abi import MIN_FRAMES, NAME

pytestmark = pytest.mark.gpu

ML = capi.KERNEL_GAUSSIAN_ML
NEW, CTX = "deform_vectors_shared_ml_fp64_dev", "deform_vectors_shared_fp64_dev"

#        M   L  F   N     R    lam   term      what this size reaches
GRID = [(33, 8, 5, 1500, 0.7, 0.1, "zero"),      # centres padded 33 -> 36; restart at layer 4; padded rows
        (40, 3, 13, 1500, 0.5, 0.05, "const"),   # odd L; first dense row layout
        (96, 6, 17, 1500, 0.7, 0.1, "linear"),   # partial second chain; NT = 6
        (64, 4, 32, 1500, 0.5, 0.05, "zero"),    # full tiles; no restart
        (64, 1, 4, 1500, 1.0, 0.1, "const"),     # one layer, one row tile
        (256, 4, 32, 1500, 1.0, 0.1, "linear"),  # several LDS chunks; the SOP's defaults
        (256, 8, 32, 600, 0.7, 0.05, "zero")]    # smallest chunks; restart inside every chunk
# a row whose F is below the measured threshold of its L runs the per-context launches: the threshold's own F beside it
GRID += [(M, L, MIN_FRAMES[L], N, R, lam, term) for M, L, F, N, R, lam, term in GRID if F < MIN_FRAMES[L]]


class Outs(Outs64):
    """test_gpu_vectors_shared_fp64's outputs (N + 64 entries, a sentinel tail), filled by the call named."""
    def call(self, batch, d, proj, dist2=True, stream_ptr=None, N=None, off=0, which=NEW):
        o = lambda t, w: t.data_ptr() + 4 * w * off
        ptr = lambda ts, w: [o(t, w) for t in ts]
        getattr(batch, which)(self.N if N is None else N, o(d["P"], 3), ptr(self.P, 3), d_dist2=o(d["d2"], 1) if dist2 else 0,
                              d_falloff=ptr(self.fall, 1), d_tangents=(o(d["tu"], 3), o(d["tv"], 3), o(d["nrm"], 3)) if proj else None,
                              d_N=o(d["Nv"], 3), d_N_out=ptr(self.No, 3), d_vtu=o(d["tu"], 3), d_vtu_out=ptr(self.tuo, 3),
                              d_vtv=o(d["tv"], 3), d_vtv_out=ptr(self.tvo, 3), d_jacobian=ptr(self.A, 9),
                              radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream_ptr)


def _positions(batch, d, N, F, proj):
    """fd_batch_deform_shared_ml_fp64_dev with the same arguments: the bits P_out and fd_falloff must have."""
    Pref = [torch.full((N, 3), float(SENTINEL), device=DEV()) for _ in range(F)]
    fref = [torch.zeros(N, device=DEV()) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_ml_fp64_dev(N, d["P"].data_ptr(), [t.data_ptr() for t in Pref], d_dist2=d["d2"].data_ptr(),
                                    d_falloff=[t.data_ptr() for t in fref],
                                    d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if proj else None,
                                    radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in Pref], [t.cpu().numpy() for t in fref]


def _refs(engines, rest, X):
    """(J, S') per frame at the points X: test_gpu_vectors._field on the M L layer-major records of fd_get_weights."""
    out = []
    for e in engines:
        centres, Wr, aff, radii = _model(e, ML, rest)
        _, J, S = _field(ML, X, centres, Wr, aff, radii)
        out.append((J, S))
    return out


def _check_against(outs, f, lv, proj, Pi_all, J, S, tu, tv, Nv, M, L, ctx=None):
    """Worst ratios of frame f against the restatement and, with `ctx`, against the per-context launches (and theirs against
    the restatement)."""
    Pg, fall, No, tuo, tvo, A = outs.host(f)
    assert np.isfinite(A).all()
    r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], Pi_all if proj else None, J, S, tu[lv], tv[lv], Nv[lv])
    rc = rr = 0.0
    if ctx is not None:
        _, cfall, cNo, ctuo, ctvo, cA = ctx.host(f)
        Af = cA[lv].astype(np.float64)
        bar = BAR_FRAME * np.linalg.norm(Af, axis=(1, 2)) + (104 + 2 * M * L) * 2.0 ** -53 * fall[lv].astype(np.float64) * S
        rc = float((np.linalg.norm(A[lv].astype(np.float64) - Af, axis=(1, 2)) / bar).max())
        rr = _check_frame(cA[lv], cNo[lv], ctuo[lv], ctvo[lv], cfall[lv], Pi_all if proj else None, J, S, tu[lv], tv[lv], Nv[lv])
    return r, rc, rr


def _run(M, L, F, N, R, lam, term):
    """The new call against the restatement, against the per-context fp64 launches and against the position call's bits in
    both fd_set_output modes; returns the worst ratios (restatement, per-context, per-context against the restatement)."""
    assert capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, F) == (NAME if F >= MIN_FRAMES[L] else "")
    P = _mesh(N); rest = synth.control_points(M, "head")
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), R, lam, TERMS[term])
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv]) if lv.size else None
    refs = _refs(engines, rest, P[lv].astype(np.float64)) if lv.size else None
    worst = worst_ctx = worst_ctx_ref = 0.0
    for proj in (False, True):
        outs, ctx = Outs(N, F), Outs(N, F)
        outs.call(batch, d, proj)
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
            r, rc, rr = _check_against(outs, f, lv, proj, Pi_all, J, S, tu, tv, Nv, M, L, ctx)
            worst, worst_ctx, worst_ctx_ref = max(worst, r), max(worst_ctx, rc), max(worst_ctx_ref, rr)
            if N >= 97:
                moving = live & (fall != 0)
                assert not np.array_equal(A[moving], np.broadcast_to(EYE, A[moving].shape))
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
    print(f"\nvectors shared ml fp64 M={M} L={L} F={F} N={N} {term}: worst ratio against the restatement {worst:.3f}, against the "
          f"per-context launches {worst_ctx:.3f}; the per-context launches against the restatement {worst_ctx_ref:.3f}")
    return worst, worst_ctx


# ---- 1. against the numpy restatement, the per-context launches and the position call -----------------------------------
@pytest.mark.parametrize("M,L,F,N,R,lam,term", GRID)
def test_restatement_per_context_launches_and_position_bits(hip_lib, M, L, F, N, R, lam, term):
    r, rc = _run(M, L, F, N, R, lam, term)
    assert r <= 1.0 and rc <= 1.0, (M, L, F, r, rc)


# ---- 2. vertex edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 129])
def test_one_vertex_one_past_a_tile_one_past_a_group(hip_lib, N):
    r, rc = _run(40, 3, 13, N, 0.5, 0.05, "const")
    assert r <= 1.0 and rc <= 1.0, (N, r, rc)


# ---- 3. chunks ----------------------------------------------------------------------------------------------------------
def _chunks(M, L, F):
    """The launcher's arithmetic (fd_vectors_shared_ml64.hip): whole centre steps of four centres and L layers, staged in
    even chunks under 158 KiB of LDS."""
    NT = 3 * ((F + 15) // 16) if F > 12 else (F + 3) // 4
    nkc = (M + 3) // 4
    fixed = 8 * (80 + NT * 64) + 8 * 4 * 32              # head + affine tiles, output pointers
    per_kc = 8 * (4 * 6 + L * NT * 64)
    kmax = (158 * 1024 - fixed) // per_kc
    return (nkc + kmax - 1) // kmax


def test_the_grid_holds_a_resident_model_and_a_staged_one():
    n = [_chunks(M, L, F) for M, L, F, *_ in GRID]
    assert min(n) == 1 and max(n) >= 2, n
    assert _chunks(64, 1, 4) == 1 and _chunks(256, 4, 32) == 6 and _chunks(256, 8, 32) == 11
    assert 8 * (4 * 6 + 8 * 6 * 64) == 24768              # 8 layers at NT = 6: 24.2 KiB a step


# ---- 4. an unbuilt frame ------------------------------------------------------------------------------------------------
def test_an_unbuilt_frame_passes_through(hip_lib):
    """The last frame's rest rig has two coincident centres: its build ends with terminationtype = -5, enqueued with
    build_async and not collected before the call (as in test_gpu_shared_ml_fp64.py), so the DEVICE decides -- that frame's
    vectors are the inputs bit for bit with A = I, the other frames meet the bars."""
    N, M, L, F, big = 1500, 64, 4, max(5, MIN_FRAMES[4]), 1_000_000
    P = _mesh(N); rest = synth.control_points(M, "head")
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    S = torch.cuda.Stream(device=DEV())
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), stream=S.cuda_stream, build=False)
    head, lone = capi.Batch(engines[:-1]), capi.Batch([engines[-1]])
    d_rest, d_del = keep
    head.set_points_dev([d_rest.data_ptr()] * (F - 1), [d_del[k].data_ptr() for k in range(F - 1)], M)
    head.build_async(S.cuda_stream); assert [r.terminationtype for r in head.build_result()] == [1] * (F - 1)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream); assert lone.build_result()[0].terminationtype == 1
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    refs = _refs(engines[:-1], rest, P[lv].astype(np.float64))              # the sound models, before the rig is spoilt
    dup = rest.copy(); dup[1] = dup[0]
    d_rest.copy_(torch.from_numpy(dup).to(DEV()))               # the same array, now with two coincident control points
    d_big = torch.from_numpy(synth.head_mesh(big)).to(DEV())
    scratch = [torch.empty_like(d_big) for _ in range(F - 1)]
    outs = Outs(N, F)
    torch.cuda.synchronize()
    for _ in range(60):          # keeps the stream busy for several milliseconds: the failure is still unknown to the host below
        head.deform_shared_ml_fp64_dev(big, d_big.data_ptr(), [t.data_ptr() for t in scratch], stream_ptr=S.cuda_stream)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream)
    outs.call(batch, d, True, stream_ptr=S.cuda_stream)
    torch.cuda.synchronize()
    assert lone.build_result(check=False)[0].terminationtype == -5
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv])
    for f in range(F - 1):
        _assert_passed_through(outs, f, ~live, tu, tv, Nv)
        J, Sf = refs[f]
        r, _, _ = _check_against(outs, f, lv, True, Pi_all, J, Sf, tu, tv, Nv, M, L)
        assert r <= 1.0, (f, r)
    assert np.array_equal(outs.host(F - 1)[0], P)
    _assert_passed_through(outs, F - 1, np.ones(N, bool), tu, tv, Nv)          # the failed frame: every vertex
    _close(engines, head, lone, batch)


# ---- 5. delegation ------------------------------------------------------------------------------------------------------
def _same(a, b, F):
    for f in range(F):
        for x, y in zip(a.host(f), b.host(f)):
            assert np.array_equal(x, y), f


@pytest.mark.parametrize("case", ["thin_plate", "ml_eval_variant"])
def test_everything_else_is_the_one_layer_call_bit_for_bit(hip_lib, case):
    N, M, L, F = 1500, 64, 4, 5
    P = _mesh(N); rest = synth.control_points(M, "head")
    _, d = _device_inputs(P)
    kw = dict(kind=capi.KERNEL_THIN_PLATE, params=[]) if case == "thin_plate" else dict(variant=2)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), **kw)
    before, new, after = Outs(N, F), Outs(N, F), Outs(N, F)
    before.call(batch, d, True, which=CTX)
    new.call(batch, d, True)
    after.call(batch, d, True, which=CTX)                           # ... and the existing call after it is unaffected
    torch.cuda.synchronize()
    assert not np.array_equal(before.host(0)[5], np.broadcast_to(EYE, (N, 3, 3)))
    _same(before, new, F); _same(before, after, F)
    _close(engines, batch)


def test_below_the_threshold_the_vectors_are_the_per_context_launches(hip_lib):
    """A multilayer batch of fewer frames than the measured threshold: positions fd_batch_deform_shared_ml_fp64_dev's,
    vectors what fd_deform_vectors_dev writes per FD_EVAL_FP64 context, bit for bit.  (Where the threshold of every layer
    count is one frame there is no such batch: the name query says so.)"""
    N, M = 1500, 64
    for L in (4, 8):
        F = MIN_FRAMES[L] - 1
        assert capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, MIN_FRAMES[L]) == NAME
        if F < 1:
            continue
        assert capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, F) == ""
        P = _mesh(N); rest = synth.control_points(M, "head")
        _, d = _device_inputs(P)
        engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
        outs = Outs(N, F)
        outs.call(batch, d, True)
        Pref, fref = _positions(batch, d, N, F, True)
        for f, e in enumerate(engines):
            e.set_eval_precision(capi.EVAL_FP64)
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
    return capi.load().fd_batch_deform_vectors_shared_ml_fp64_dev(batch.h, None, a["N"], vp(a["P_in"]), tab(a["P_out"]), vp(a["d2"]), tab(a["fall"]),
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


# ---- 6. argument errors -------------------------------------------------------------------------------------------------
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
        for s in shared:                                                    # every aliasing pair
            assert _raw(batch, outs, d, N, **{table: [ts[0], s, ts[2]]}) == capi.FD_E_INVALID, (table, s)
        assert _raw(batch, outs, d, N, **{table: [ts[0], None, ts[2]]}) == capi.FD_E_INVALID, table          # a NULL table entry
    for s in shared:
        assert _raw(one, outs1, d, N, P_out=[s]) == capi.FD_E_INVALID      # a batch of one in place, and over any other input
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


# ---- 7. bits ------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_in_two_ranges_and_on_fewer_cus(hip_lib):
    N, M, L, F, cut = 1500, 96, 6, 17, 700
    assert capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, F) == NAME
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


# ---- 8. consumed --------------------------------------------------------------------------------------------------------
def test_rebuild_behind_wait_consumed(hip_lib):
    """The call on one stream, fd_batch_wait_consumed on a second, new deltas and a rebuild there while the launches are in
    flight: the outputs equal those of the same call without the rebuild."""
    N, M, L, F = 50_000, 64, 4, 16
    assert capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, F) == NAME
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
