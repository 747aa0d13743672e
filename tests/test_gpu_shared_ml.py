"""GPU: fd_batch_deform_shared_ml_dev -- the frames of a shot of multilayer models in one matrix-pipe launch
(facedeform_amd/csrc/fd_eval_shared_ml.hip) against the numpy oracle (oracle/fd_oracle.py
build_multilayer), against the per-frame launches, and the contract of include/facedeform_hip.h: pass-through,
repeatability, rebuild behind fd_batch_wait_consumed, delegation and errors."""
import numpy as np
import pytest
import torch

from conftest import parity_ratio
from facedeform_amd import capi, synth
from oracle import fd_oracle as fo
from test_shared_ml_abi import NAME, threshold

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
RADIUS2, RATE = 1.0, 1.5
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
DEV = lambda: torch.device("cuda", 0)


def _deltas(rest, F, flip=False):
    d = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    return np.ascontiguousarray(d[::-1] * np.float32(0.5)) if flip else d


def _mesh(N):
    return synth.head_mesh(max(N, 20_000))[:: max(N, 20_000) // N][:N].copy()


def _dist2(N):
    return np.linspace(0.0, 1.2, N).astype(np.float32)           # gate and fall-off in play


def _engines(M, L, F, rest, deltas, R=1.0, lam=0.1, term=capi.TERM_LINEAR, kind=capi.KERNEL_GAUSSIAN_ML, params=None,
             precision=capi.EVAL_FP32, variant=0, stream=None, build=True):
    d_rest = torch.from_numpy(rest).to(DEV())
    d_del = torch.from_numpy(np.ascontiguousarray(deltas)).to(DEV())
    engines = []
    for _ in range(F):
        e = capi.Engine(precision=precision, variant=variant)
        if stream is not None:
            e.set_stream(stream)
        e.set_kernel(kind, [R, L, lam] if params is None else list(params)); e.set_term(term)
        engines.append(e)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    if build:
        batch.build_async(stream)
        assert [r.terminationtype for r in batch.build_result()] == [1] * F
    return engines, batch, (d_rest, d_del)


def _close(engines, *batches):
    for b in batches:
        b.close()
    for e in engines:
        e.set_stream(None); e.close()


class Outs:
    """Outputs of one call, N + 64 entries each: the tail is a canary (entries past N are not touched)."""
    def __init__(self, N, F):
        full = lambda w: torch.full((N + 64, w) if w else (N + 64,), SENTINEL, device=DEV())
        self.N, self.F = N, F
        self.P = [full(3) for _ in range(F)]
        self.fall = [full(0) for _ in range(F)]
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() for t in self.P], [t.data_ptr() for t in self.fall]

    def host(self):
        P = [t.cpu().numpy() for t in self.P]; fall = [t.cpu().numpy() for t in self.fall]
        for p, f in zip(P, fall):
            assert (p[self.N:] == np.float32(SENTINEL)).all() and (f[self.N:] == np.float32(SENTINEL)).all()
        return [p[:self.N] for p in P], [f[:self.N] for f in fall]


def _call(batch, which, N, d_P, d_d2, outs, stream=None):
    po, fo_ = outs.ptrs()
    getattr(batch, which)(N, d_P.data_ptr(), po, d_dist2=d_d2.data_ptr() if d_d2 is not None else 0, d_falloff=fo_,
                          radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream)


def _per_frame(batch, N, d_P, d_d2, outs):
    po, fo_ = outs.ptrs()
    F = outs.F
    batch.deform_dev(N, [d_P.data_ptr()] * F, po, d_dist2=[d_d2.data_ptr()] * F if d_d2 is not None else None, d_falloff=fo_,
                     radius2=RADIUS2, falloffrate=RATE)


# ---- 1. oracle parity, 2. against the per-frame launches -----------------------------------------------------------------
#        M   L  F   N     R    lam   term      why this size
GRID = [(33, 8, 5, 4099, 0.7, 0.1, "zero"),      # ragged padding; a centre's layers span both lane halves
        (40, 3, 17, 4099, 0.5, 0.05, "const"),   # share 1
        (96, 6, 16, 6000, 0.7, 0.1, "linear"),   # share 2
        (64, 4, 32, 4099, 0.5, 0.05, "zero"),    # share 4, full tiles
        (256, 4, 32, 6000, 1.0, 0.1, "linear"),  # staged in several chunks; the SOP's defaults
        (64, 1, 4, 4099, 1.0, 0.1, "const"),     # one layer
        (64, 1, 32, 4099, 0.7, 0.1, "linear")]   # one layer, full tiles


@pytest.mark.parametrize("M,L,F,N,R,lam,term", GRID)
def test_oracle_parity_and_the_per_frame_launches(hip_lib, oracle, M, L, F, N, R, lam, term):
    """Every frame within the project's bar (parity_ratio <= 1 at 1e-5) of the oracle, in both output modes, and of the
    per-frame launches; fd_falloff bit-identical to theirs, the same entries written.  Prints, per frame and before it
    asserts, the ratio of the new launch and of the per-context fp32 launches on the same inputs (DESIGN.md 4.1f records
    them).  Measured so far: the per-context fp32 launches reach 0.889 of the bar on the first size (M = 33, L = 8, R = 0.7,
    zero term, frame 0) -- the finest layer's radius is R / 128 and the fp32 exponent carries the rounding of the normalised
    coordinates; the new launch's own figures have not been collected."""
    assert capi.fd_shared_ml_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head"); dist2 = _dist2(N)
    deltas = _deltas(rest, F)
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(dist2).to(DEV())
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, TERMS[term])
    refs = []
    for f in range(F):
        table = oracle.control_table(rest, rest + deltas[f])
        tt, table_ml, Wo, radii = oracle.build_multilayer(table, R, L, lam, TERMS[term])
        assert tt == 1
        refs.append(oracle.deform(table_ml, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P, dist2=dist2, radius2=RADIUS2, falloffrate=RATE))
    gated = dist2 > np.float32(RADIUS2)
    worst_new = worst_old = 0.0
    for output in (capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT):
        for e in engines:
            e.set_output(output)
        new, old = Outs(N, F), Outs(N, F)
        _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, new)
        _per_frame(batch, N, d_P, d_d2, old)
        torch.cuda.synchronize()
        Pn, fn = new.host(); Po, fo_ = old.host()
        for f in range(F):
            ref, rfall = refs[f]
            a, b = Pn[f], Po[f]
            if output == capi.OUTPUT_DISPLACEMENT:         # P + (d f) as the reference adds it: the same bar on the same quantity
                assert np.array_equal(a[gated], np.zeros_like(a[gated]))
                a, b = P + a, P + b
            assert np.isfinite(a).all()
            r_new, r_old = parity_ratio(a, ref, P, 1e-5), parity_ratio(b, ref, P, 1e-5)
            worst_new, worst_old = max(worst_new, r_new), max(worst_old, r_old)
            # (r_old is recorded, not asserted: it is the one-frame kernel's figure, whose own bar is 1.0.  Where it is above
            #  0.25 a miss of the new launch would call for another input before it counts as a defect of the launch; the bar
            #  on the new launch itself is unconditional.)
            print(f"shared ml M={M} L={L} F={F} {term} output {output} frame {f}: new {r_new:.3f}, per-context fp32 {r_old:.3f}")
            assert r_new <= 1.0, (output, f, r_new)
            assert parity_ratio(a, b, P, 1e-5) <= 1.0, (output, f)
            assert np.array_equal(fn[f], fo_[f])                                         # bit-identical, the same entries written
            assert np.array_equal(fn[f] == np.float32(SENTINEL), gated)
            assert np.abs(fn[f][~gated] - rfall[~gated]).max() <= 3e-7
    print(f"\nshared ml M={M} L={L} F={F} N={N} {term}: worst parity ratio new {worst_new:.3f}, per-context fp32 {worst_old:.3f}")
    for e in engines:
        e.set_output(capi.OUTPUT_POSITION)
    _close(engines, batch)


# ---- 3. frame counts -------------------------------------------------------------------------------------------------------
def test_every_frame_count_edge(hip_lib):
    """Every tile count and the three-rows-per-frame packing at its edges: each frame of each count against its own
    one-frame launch."""
    M, L, N = 64, 4, 2051
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(_dist2(N)).to(DEV())
    engines, batch32, keep = _engines(M, L, 32, rest, _deltas(rest, 32))
    old = Outs(N, 32)
    _per_frame(batch32, N, d_P, d_d2, old)
    torch.cuda.synchronize()
    Po, fo_ = old.host()
    for F in sorted({threshold(), 3, 12, 16, 17, 20, 31, 32}):
        if F < threshold():
            continue
        batch = capi.Batch(engines[:F])
        new = Outs(N, F)
        _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, new)
        torch.cuda.synchronize()
        Pn, fn = new.host()
        for f in range(F):
            assert parity_ratio(Pn[f], Po[f], P, 1e-5) <= 1.0, (F, f)
            assert not np.array_equal(Pn[f], P)
            assert np.array_equal(fn[f], fo_[f]), (F, f)
        batch.close()
    _close(engines, batch32)


# ---- 4. pass-through --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output", [capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT])
def test_gated_vertices_and_a_failed_build_pass_through(hip_lib, output):
    """The last frame's rest rig has two coincident centres: its build ends with terminationtype = -5, enqueued with
    build_async and not collected before the call, so the DEVICE decides -- that frame is passed through like the gated
    vertices of the others, fd_falloff untouched there, nothing written past N."""
    N, M, L, F, big = 3001, 64, 4, 5, 1_000_000
    P = _mesh(N); rest = synth.control_points(M, "head"); dist2 = _dist2(N)
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(dist2).to(DEV())
    S = torch.cuda.Stream(device=DEV())
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), stream=S.cuda_stream, build=False)
    head, lone = capi.Batch(engines[:-1]), capi.Batch([engines[-1]])
    d_rest, d_del = keep
    head.set_points_dev([d_rest.data_ptr()] * (F - 1), [d_del[k].data_ptr() for k in range(F - 1)], M)
    head.build_async(S.cuda_stream); assert [r.terminationtype for r in head.build_result()] == [1] * (F - 1)
    # (the lone context's build path once on the sound rig: its second enqueue below is then a matter of microseconds)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream); assert lone.build_result()[0].terminationtype == 1
    dup = rest.copy(); dup[1] = dup[0]
    d_rest.copy_(torch.from_numpy(dup).to(DEV()))               # the same array, now with two coincident control points
    for e in engines:
        e.set_output(output)
    d_big = torch.from_numpy(synth.head_mesh(big)).to(DEV())
    scratch = [torch.empty_like(d_big) for _ in range(F - 1)]
    out = Outs(N, F)
    po, fo_ = out.ptrs()
    torch.cuda.synchronize()
    for _ in range(60):          # keeps the stream busy for several milliseconds: the failure is still unknown to the host below
        head.deform_shared_ml_dev(big, d_big.data_ptr(), [t.data_ptr() for t in scratch], stream_ptr=S.cuda_stream)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream)
    batch.deform_shared_ml_dev(N, d_P.data_ptr(), po, d_dist2=d_d2.data_ptr(), d_falloff=fo_, radius2=RADIUS2, falloffrate=RATE,
                               stream_ptr=S.cuda_stream)
    torch.cuda.synchronize()
    assert lone.build_result(check=False)[0].terminationtype == -5
    Pn, fn = out.host()
    gated = dist2 > np.float32(RADIUS2)
    assert gated.sum() > N // 8
    want = np.zeros_like(P) if output == capi.OUTPUT_DISPLACEMENT else P
    for k in range(F - 1):
        assert np.array_equal(Pn[k][gated], want[gated])
        assert (fn[k][gated] == np.float32(SENTINEL)).all()           # fd_falloff untouched
        assert (fn[k][~gated] != np.float32(SENTINEL)).all()
        assert np.isfinite(Pn[k]).all() and not np.array_equal(Pn[k][~gated], want[~gated])
    assert np.array_equal(Pn[F - 1], want)                            # the failed frame: every vertex passed through
    assert (fn[F - 1] == np.float32(SENTINEL)).all()
    for e in engines:
        e.set_output(capi.OUTPUT_POSITION)
    _close(engines, head, lone, batch)


# ---- 5. repeatability, 6. rebuild behind fd_batch_wait_consumed ----------------------------------------------------------
def test_same_bits_on_every_call_in_two_ranges_and_on_fewer_cus(hip_lib):
    N, M, L, F, cut = 70_001, 96, 4, 17, 12_345
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(_dist2(N)).to(DEV())
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    one, again, two, few = Outs(N, F), Outs(N, F), Outs(N, F), Outs(N, F)
    _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, one)
    _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, again)
    po, fo_ = two.ptrs()
    kw = dict(radius2=RADIUS2, falloffrate=RATE)
    batch.deform_shared_ml_dev(cut, d_P.data_ptr(), po, d_dist2=d_d2.data_ptr(), d_falloff=fo_, **kw)
    batch.deform_shared_ml_dev(N - cut, d_P.data_ptr() + 12 * cut, [p + 12 * cut for p in po], d_dist2=d_d2.data_ptr() + 4 * cut,
                               d_falloff=[p + 4 * cut for p in fo_], **kw)
    batch.set_eval_cus(64)
    _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, few)
    batch.set_eval_cus(0)
    torch.cuda.synchronize()
    P1, f1 = one.host()
    assert not np.array_equal(P1[0], P)
    for other in (again, two, few):
        P2, f2 = other.host()
        for f in range(F):
            assert np.array_equal(P1[f], P2[f]) and np.array_equal(f1[f], f2[f])
    _close(engines, batch)


def test_rebuild_behind_wait_consumed(hip_lib, oracle):
    """Evaluate on one stream, fd_batch_wait_consumed on the build stream, rebuild the contexts with other deltas there,
    then synchronise: the outputs are those of the FIRST deltas."""
    N, M, L, F = 200_000, 64, 4, 8
    P = synth.head_mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    sA, sB = torch.cuda.Stream(device=DEV()), torch.cuda.Stream(device=DEV())
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, stream=sA.cuda_stream)
    other = torch.from_numpy(_deltas(rest, F, flip=True)).to(DEV())
    out = [torch.empty_like(d_P) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_ml_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], stream_ptr=sA.cuda_stream)
    batch.wait_consumed(sB.cuda_stream)
    batch.set_points_dev([keep[0].data_ptr()] * F, [other.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(sB.cuda_stream)
    torch.cuda.synchronize()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    idx = np.arange(0, N, 97)
    for f in (0, F - 1):
        table = oracle.control_table(rest, rest + deltas[f])
        tt, table_ml, Wo, radii = oracle.build_multilayer(table, 1.0, L, 0.1, capi.TERM_LINEAR)
        ref, _ = oracle.deform(table_ml, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P[idx])
        assert parity_ratio(out[f].cpu().numpy()[idx], ref, P[idx], 1e-5) <= 1.0
    _close(engines, batch)


# ---- 7. delegation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["thin_plate", "qnn", "ml_fp64", "ml_eval_variant", "ml_below_threshold"])
def test_everything_else_is_the_existing_call_bit_for_bit(hip_lib, case):
    N, M, L = 4000, 64, 4
    F = 1 if case == "ml_below_threshold" else 3
    if case == "ml_below_threshold" and threshold() < 2:
        pytest.skip("no frame count below the threshold")
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(_dist2(N)).to(DEV())
    kw = {"thin_plate": dict(kind=capi.KERNEL_THIN_PLATE, params=[]), "qnn": dict(kind=capi.KERNEL_GAUSSIAN_QNN, params=[1.0, 5.0]),
          "ml_fp64": dict(precision=capi.EVAL_FP64), "ml_eval_variant": dict(variant=2), "ml_below_threshold": {}}[case]
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), **kw)
    before, new, after = Outs(N, F), Outs(N, F), Outs(N, F)
    _call(batch, "deform_shared_dev", N, d_P, d_d2, before)
    _call(batch, "deform_shared_ml_dev", N, d_P, d_d2, new)
    _call(batch, "deform_shared_dev", N, d_P, d_d2, after)        # ... and the existing call after it is unaffected
    torch.cuda.synchronize()
    Pb, fb = before.host(); Pn, fn = new.host(); Pa, fa = after.host()
    for f in range(F):
        assert not np.array_equal(Pb[f], P)
        assert np.array_equal(Pb[f], Pn[f]) and np.array_equal(fb[f], fn[f])
        assert np.array_equal(Pb[f], Pa[f]) and np.array_equal(fb[f], fa[f])
    _close(engines, batch)


def test_the_existing_call_between_two_launches_changes_nothing(hip_lib):
    """The new launch, fd_batch_deform_shared_dev (the per-context launches for this model) and the new launch again on one
    batch: the scratch of the new call survives the call between, and the new launch is not the per-frame launch (other bits
    somewhere, within the bar)."""
    N, M, L, F = 6000, 64, 4, 20
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    new, again, old = Outs(N, F), Outs(N, F), Outs(N, F)
    _call(batch, "deform_shared_ml_dev", N, d_P, None, new)
    _call(batch, "deform_shared_dev", N, d_P, None, old)           # the per-context launches for this model
    _call(batch, "deform_shared_ml_dev", N, d_P, None, again)
    torch.cuda.synchronize()
    Pn, _ = new.host(); Pa, _ = again.host(); Po, _ = old.host()
    differs = False
    for f in range(F):
        assert np.array_equal(Pn[f], Pa[f])
        assert parity_ratio(Pn[f], Po[f], P, 1e-5) <= 1.0
        differs |= not np.array_equal(Pn[f], Po[f])
    assert differs
    _close(engines, batch)


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------
def test_errors(hip_lib):
    N, M, L, F = 1000, 64, 4, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    outs = [torch.empty_like(d_P) for _ in range(F)]
    ptr = [t.data_ptr() for t in outs]
    # a context without a model
    engines = [capi.Engine() for _ in range(F)]
    for e in engines:
        e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [1.0, L, 0.1])
    batch = capi.Batch(engines)
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    _close(engines, batch)
    # different rest arrays
    d_rest = [torch.from_numpy(rest).to(DEV()) for _ in range(F)]
    d_del = torch.from_numpy(_deltas(rest, F)).to(DEV())
    engines = [capi.Engine() for _ in range(F)]
    for e in engines:
        e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [1.0, L, 0.1]); e.set_term(capi.TERM_LINEAR)
    batch = capi.Batch(engines)
    batch.set_points_dev([t.data_ptr() for t in d_rest], [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr)
    assert ei.value.code == capi.FD_E_INVALID and "one rest rig" in str(ei.value)
    _close(engines, batch)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F))
    # mixed fd_set_output settings
    engines[1].set_output(capi.OUTPUT_DISPLACEMENT)
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr)
    assert ei.value.code == capi.FD_E_INVALID and "fd_set_output" in str(ei.value)
    engines[1].set_output(capi.OUTPUT_POSITION)
    # an output over a shared input
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_ml_dev(N, d_P.data_ptr(), [ptr[0], d_P.data_ptr(), ptr[2]])
    assert ei.value.code == capi.FD_E_INVALID and "shared input" in str(ei.value)
    batch.deform_shared_ml_dev(N, d_P.data_ptr(), ptr)             # and the batch still works
    torch.cuda.synchronize()
    assert not torch.equal(outs[0], d_P)
    _close(engines, batch)
