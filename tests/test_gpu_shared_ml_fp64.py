"""GPU: fd_batch_deform_shared_ml_fp64_dev -- the frames of a shot of multilayer models evaluated in fp64 by one
matrix-pipe launch (k_deform64_shared_ml, facedeform_amd/csrc/fd_eval_shared_ml64.hip).

Yardsticks, fixed in advance (include/facedeform_hip.h states them):
  * the per-context fp64 launches on the same batch (fd_batch_deform_shared_fp64_dev, which runs them for a multilayer
    batch): the two fp64 sums ahead of the one rounding differ by at most (96 + M L) 2^-53 S_f, S_f = max_a sum_r |w_f[r][a]|
    -- 96 = 4^3 x 1.5 ulp for the chain E_{l+1} = E_l^4 restarted at layer 4, M L for the summation order -- so every
    component is within ulp32(b) + that bound; every fd_falloff value is bit-identical;
  * the oracle (oracle/fd_oracle.py build_multilayer + deform) at the project's fp64 bar: parity_ratio <= 1 at 2e-7."""
import numpy as np
import pytest
import torch

from conftest import parity_ratio
from facedeform_amd import capi, synth
from oracle import fd_oracle as fo
from test_gpu_shared_ml import DEV, SENTINEL, TERMS, Outs, _close, _deltas, _engines, _mesh
from test_gpu_vectors import RADIUS2, RATE, _inputs
from test_shared_ml_fp64_abi import NAME

pytestmark = pytest.mark.gpu

#        M   L  F   N     R    lam   term      what this size reaches
GRID = [(33, 8, 5, 1500, 0.7, 0.1, "zero"),      # centres padded 33 -> 36; restart at layer 4; padded rows
        (40, 3, 13, 1500, 0.5, 0.05, "const"),   # odd L; first dense row layout
        (96, 6, 17, 1500, 0.7, 0.1, "linear"),   # partial second chain; NT = 6
        (64, 4, 32, 1500, 0.5, 0.05, "zero"),    # full tiles; no restart
        (64, 1, 1, 1500, 1.0, 0.1, "const"),     # one layer, one frame
        (256, 4, 32, 1500, 1.0, 0.1, "linear"),  # several LDS chunks; the SOP's defaults
        (256, 8, 32, 600, 0.7, 0.05, "zero")]    # smallest chunks; restart inside every chunk


def _device_inputs(P):
    tu, tv, nrm, _, dist2 = _inputs(P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV())
    return dist2, {"P": t(P), "tu": t(tu), "tv": t(tv), "nrm": t(nrm), "d2": t(dist2)}


def _mode_args(d, full):
    return dict(d_dist2=d["d2"].data_ptr() if full else 0, d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if full else None,
                radius2=RADIUS2, falloffrate=RATE)


def _call(batch, which, N, d, outs, full, stream=None):
    po, fo_ = outs.ptrs()
    getattr(batch, which)(N, d["P"].data_ptr(), po, d_falloff=fo_, stream_ptr=stream, **_mode_args(d, full))


def _table(rest, delta):
    """The oracle's control table from the very fp32 numbers the engine is given (rest | delta, widened), as
    tests/test_gpu_raw_delta.py builds it: control_table(rest, rest + delta) would round the sum to fp32 first, which moves the
    deltas by up to 2^-24 |rest| -- 1.1 to 2.1 times the 2e-7 bar on these inputs, whatever R and lambda."""
    return np.concatenate([np.asarray(rest, np.float32), np.asarray(delta, np.float32)], axis=1).astype(np.float64)


def _weight_sums(engines, M, L):
    """S_f = max_a sum_r |w_f[r][a]| over the M L Gaussian records of frame f (fd_get_weights; the affine rows left out)."""
    return [float(np.abs(e.get_weights()[0][:M * L]).sum(axis=0).max()) for e in engines]


def _bound(b, M, L, S):
    """ulp32(b) + (96 + M L) 2^-53 S_f, per component."""
    return np.spacing(np.abs(np.asarray(b, np.float32))).astype(np.float64) + (96 + M * L) * 2.0 ** -53 * S


def _assert_within_bound(a, b, M, L, S, what):
    err = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    lim = _bound(b, M, L, S)
    worst = float((err / lim).max())
    assert worst <= 1.0, (what, worst)
    return worst


# ---- 1. against the per-context fp64 launches, 2. against the oracle ---------------------------------------------------
@pytest.mark.parametrize("M,L,F,N,R,lam,term", GRID)
def test_per_context_fp64_launches_and_oracle(hip_lib, oracle, M, L, F, N, R, lam, term):
    """Both output modes, with and without dist2 and tangent frames: every component within ulp32(b) + (96 + M L) 2^-53 S_f of
    fd_batch_deform_shared_fp64_dev (the per-context fp64 launches), fd_falloff bit-identical with the same entries written,
    canary tails untouched; without gate and projection, parity_ratio <= 1 at 2e-7 against the oracle in both output modes.
    Prints, before it asserts, the share of components that are not bit-identical and both launches' oracle ratios
    (DESIGN.md 4.1g records them).  Measured on an MI355X: 0 of 2.0 million components not bit-identical over the seven
    sizes, both oracle ratios 0.000 on every size."""
    assert capi.fd_shared_ml_fp64_kernel_name(M, L, F) == NAME
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, R, lam, TERMS[term])
    S = _weight_sums(engines, M, L)
    refs = []
    for f in range(F):
        tt, table_ml, Wo, radii = oracle.build_multilayer(_table(rest, deltas[f]), R, L, lam, TERMS[term])
        assert tt == 1
        refs.append(oracle.deform(table_ml, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P)[0])
    gated = dist2 > np.float32(RADIUS2)
    differ = total = 0
    worst = worst_new = worst_old = 0.0
    for output in (capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT):
        for e in engines:
            e.set_output(output)
        for full in (False, True):
            new, old = Outs(N, F), Outs(N, F)
            _call(batch, "deform_shared_ml_fp64_dev", N, d, new, full)
            _call(batch, "deform_shared_fp64_dev", N, d, old, full)
            torch.cuda.synchronize()
            Pn, fn = new.host(); Po, fo_ = old.host()             # (host() checks the canary tails)
            for f in range(F):
                a, b = Pn[f], Po[f]
                assert np.isfinite(a).all()
                differ += int((a != b).sum()); total += a.size
                if not full:
                    an, bn = (P + a, P + b) if output == capi.OUTPUT_DISPLACEMENT else (a, b)
                    r_new, r_old = parity_ratio(an, refs[f], P, 2e-7), parity_ratio(bn, refs[f], P, 2e-7)
                    worst_new, worst_old = max(worst_new, r_new), max(worst_old, r_old)
                    print(f"shared ml fp64 M={M} L={L} F={F} {term} output {output} frame {f}: oracle ratio at 2e-7 new {r_new:.3f}, "
                          f"per-context fp64 {r_old:.3f}")
            print(f"shared ml fp64 M={M} L={L} F={F} N={N} {term} output {output} full {full}: {differ} of {total} components not "
                  f"bit-identical so far; worst oracle ratio new {worst_new:.3f}, per-context fp64 {worst_old:.3f}")
            for f in range(F):
                a, b = Pn[f], Po[f]
                worst = max(worst, _assert_within_bound(a, b, M, L, S[f], (output, full, f)))
                assert np.array_equal(fn[f], fo_[f])                                     # bit-identical, the same entries written
                if full:
                    assert np.array_equal(fn[f] == np.float32(SENTINEL), gated)
                    assert np.array_equal(a[gated], np.zeros_like(a[gated]) if output == capi.OUTPUT_DISPLACEMENT else P[gated])
                else:
                    assert np.array_equal(fn[f], np.ones(N, np.float32))
                    an = P + a if output == capi.OUTPUT_DISPLACEMENT else a
                    r = parity_ratio(an, refs[f], P, 2e-7)
                    assert r <= 1.0, (output, f, r)
    print(f"\nshared ml fp64 M={M} L={L} F={F} N={N} {term}: {differ} of {total} components not bit-identical ({differ / total:.2e}); "
          f"worst |a - b| / bound {worst:.3f}; worst oracle ratio new {worst_new:.3f}, per-context fp64 {worst_old:.3f}")
    for e in engines:
        e.set_output(capi.OUTPUT_POSITION)
    _close(engines, batch)


@pytest.mark.parametrize("N", [1, 257])
def test_one_vertex_and_one_past_a_group(hip_lib, N):
    M, L, F, R, lam = 40, 3, 13, 0.5, 0.05
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), R, lam, capi.TERM_CONST)
    S = _weight_sums(engines, M, L)
    for full in (False, True):
        new, old = Outs(N, F), Outs(N, F)
        _call(batch, "deform_shared_ml_fp64_dev", N, d, new, full)
        _call(batch, "deform_shared_fp64_dev", N, d, old, full)
        torch.cuda.synchronize()
        Pn, fn = new.host(); Po, fo_ = old.host()
        for f in range(F):
            _assert_within_bound(Pn[f], Po[f], M, L, S[f], (N, full, f))
            assert np.array_equal(fn[f], fo_[f])
            assert full or not np.array_equal(Pn[f], P)           # (with dist2 the one vertex may be a gated one)
    _close(engines, batch)


# ---- 3. the chain -------------------------------------------------------------------------------------------------------
def _chain_sums(d2, s0, w, L, restart):
    """numpy restatement of the kernel's chain for one vertex: sum_c sum_l E_l(c) w[c, l], E_0 = exp(d2 s0), E_{l+1} = E_l^4,
    a fresh exponential every `restart` layers (restart >= L: never)."""
    acc = np.zeros(w.shape[2])
    for l in range(L):
        if l % restart == 0:
            E = np.exp(d2 * (s0 * 4.0 ** l))
        acc = acc + (E[:, None] * w[:, l, :]).sum(axis=0)
        E2 = E * E
        E = E2 * E2
    return acc


def _chain_terms(d2, s0, L, restart):
    """E_l per (centre, layer) of the same chain."""
    out = np.zeros((d2.shape[0], L))
    for l in range(L):
        if l % restart == 0:
            E = np.exp(d2 * (s0 * 4.0 ** l))
        out[:, l] = E
        E2 = E * E
        E = E2 * E2
    return out


def test_chain_restart_keeps_the_bound(hip_lib):
    """L = 8, M = 33, R = 0.7, displacement output, at vertices next to the centres (within the finest radius R / 128, where
    E_7 is largest): within the bound of (1) of the per-context launches.  The bound's chain term, 96 ulp, is 64 times
    tighter than an unrestarted chain's 4^7 x 1.5 ulp; a numpy restatement of both chains on the same vertices and the
    device's weights is printed beside it (DESIGN.md 4.1g records the two figures): the restarted chain must sit inside
    96 x 2^-53 S_f of the direct exponentials, the unrestarted one is reported."""
    M, L, F, R, lam = 33, 8, 5, 0.7, 0.1
    rest = synth.control_points(M, "head")
    rng = np.random.default_rng(11)
    k = 16                                                   # vertices per centre, 0.05 .. 0.9 of the finest radius away
    dirs = rng.normal(size=(M, k, 3)); dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    dist = (R / 2 ** (L - 1)) * np.linspace(0.05, 0.9, k)[None, :, None]
    P = (rest[:, None, :].astype(np.float64) + dirs * dist).reshape(-1, 3).astype(np.float32)
    N = P.shape[0]
    dist2, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), R, lam, capi.TERM_ZERO)
    S = _weight_sums(engines, M, L)
    for e in engines:
        e.set_output(capi.OUTPUT_DISPLACEMENT)
    new, old = Outs(N, F), Outs(N, F)
    _call(batch, "deform_shared_ml_fp64_dev", N, d, new, False)
    _call(batch, "deform_shared_fp64_dev", N, d, old, False)
    torch.cuda.synchronize()
    Pn, _ = new.host(); Po, _ = old.host()
    # the numpy restatement on frame 0's weights (layer-major in fd_get_weights: record l M + c)
    W, radii = engines[0].get_weights()
    w = W[:M * L].reshape(L, M, 3).transpose(1, 0, 2)
    s0 = -1.0 / radii[:M] ** 2
    Pd = P.astype(np.float64); C = rest.astype(np.float64)
    worst_restart = worst_plain = term_restart = term_plain = 0.0
    for v in range(0, N, 7):
        diff = Pd[v] - C
        d2 = diff[:, 2] * diff[:, 2] + (diff[:, 1] * diff[:, 1] + diff[:, 0] * diff[:, 0])
        # per term (phi <= 1, so absolute): the own centre's eight layers, whatever the weights are
        c = v // k
        t = lambda restart: _chain_terms(d2[c:c + 1], s0[c:c + 1], L, restart)
        term_restart = max(term_restart, float(np.abs(t(4) - t(1)).max())); term_plain = max(term_plain, float(np.abs(t(L) - t(1)).max()))
        direct = _chain_sums(d2, s0, w, L, 1)
        worst_restart = max(worst_restart, float(np.abs(_chain_sums(d2, s0, w, L, 4) - direct).max()))
        worst_plain = max(worst_plain, float(np.abs(_chain_sums(d2, s0, w, L, L) - direct).max()))
    unit = 2.0 ** -53 * S[0]
    print(f"\nchain, numpy restatement, per term: restarted at 4 within {term_restart * 2.0 ** 53:.0f} x 2^-53 of the direct exponential, "
          f"unrestarted {term_plain * 2.0 ** 53:.0f} x 2^-53")
    assert term_restart <= 96 * 2.0 ** -53 < term_plain          # the restart is what keeps a term inside the bound's 96
    print(f"\nchain, numpy restatement, M={M} L={L} R={R}: restarted at 4 within {worst_restart / unit:.1f} x 2^-53 S_f of the direct "
          f"exponentials, unrestarted {worst_plain / unit:.1f} x 2^-53 S_f (bound's chain term: 96)")
    worst = 0.0
    for f in range(F):
        assert np.abs(Po[f]).max() > 0
        worst = max(worst, _assert_within_bound(Pn[f], Po[f], M, L, S[f], f))
    print(f"chain, device: worst |a - b| / bound {worst:.3f}")
    assert worst_restart <= 96 * unit
    for e in engines:
        e.set_output(capi.OUTPUT_POSITION)
    _close(engines, batch)


# ---- 4. contract -----------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_in_two_ranges_and_on_fewer_cus(hip_lib):
    N, M, L, F, cut = 1500, 96, 6, 17, 700
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), 0.7, 0.1)
    one, again, two, few = Outs(N, F), Outs(N, F), Outs(N, F), Outs(N, F)
    _call(batch, "deform_shared_ml_fp64_dev", N, d, one, True)
    _call(batch, "deform_shared_ml_fp64_dev", N, d, again, True)
    a = _mode_args(d, True)
    po, fo_ = two.ptrs()
    batch.deform_shared_ml_fp64_dev(cut, d["P"].data_ptr(), po, d_falloff=fo_, **a)
    off = lambda p, w: p + 4 * w * cut
    a2 = dict(a, d_dist2=off(a["d_dist2"], 1), d_tangents=tuple(off(p, 3) for p in a["d_tangents"]))
    batch.deform_shared_ml_fp64_dev(N - cut, off(d["P"].data_ptr(), 3), [off(p, 3) for p in po], d_falloff=[off(p, 1) for p in fo_], **a2)
    batch.set_eval_cus(3)
    _call(batch, "deform_shared_ml_fp64_dev", N, d, few, True)
    batch.set_eval_cus(0)
    torch.cuda.synchronize()
    P1, f1 = one.host()
    assert not np.array_equal(P1[0], P)
    for other in (again, two, few):
        P2, f2 = other.host()
        for f in range(F):
            assert np.array_equal(P1[f], P2[f]) and np.array_equal(f1[f], f2[f])
    _close(engines, batch)


@pytest.mark.parametrize("output", [capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT])
def test_an_unbuilt_frame_passes_through(hip_lib, output):
    """The last frame's rest rig has two coincident centres: its build ends with terminationtype = -5, enqueued with
    build_async and not collected before the call, so the DEVICE decides -- that frame is passed through like the gated
    vertices of the others (position bit for bit, 0 as a displacement), fd_falloff not written."""
    N, M, L, F, big = 1500, 64, 4, 5, 1_000_000
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
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
    torch.cuda.synchronize()
    for _ in range(60):          # keeps the stream busy for several milliseconds: the failure is still unknown to the host below
        head.deform_shared_ml_fp64_dev(big, d_big.data_ptr(), [t.data_ptr() for t in scratch], stream_ptr=S.cuda_stream)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream)
    _call(batch, "deform_shared_ml_fp64_dev", N, d, out, True, stream=S.cuda_stream)
    torch.cuda.synchronize()
    assert lone.build_result(check=False)[0].terminationtype == -5
    Pn, fn = out.host()
    gated = dist2 > np.float32(RADIUS2)
    assert gated.sum() > N // 4
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


def test_rebuild_behind_wait_consumed(hip_lib):
    """Evaluate on one stream, fd_batch_wait_consumed on the build stream, rebuild the contexts with other deltas there while
    the evaluation is in flight: its outputs equal those of an undisturbed run."""
    N, M, L, F = 200_000, 64, 4, 8
    P = synth.head_mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    sA, sB = torch.cuda.Stream(device=DEV()), torch.cuda.Stream(device=DEV())
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(M, L, F, rest, deltas, stream=sA.cuda_stream)
    other = torch.from_numpy(_deltas(rest, F, flip=True)).to(DEV())
    calm = [torch.empty_like(d_P) for _ in range(F)]
    out = [torch.empty_like(d_P) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_ml_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in calm], stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    batch.deform_shared_ml_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], stream_ptr=sA.cuda_stream)
    batch.wait_consumed(sB.cuda_stream)
    batch.set_points_dev([keep[0].data_ptr()] * F, [other.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(sB.cuda_stream)
    torch.cuda.synchronize()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    for a, b in zip(calm, out):
        assert torch.equal(a, b)                     # the first models' outputs
    assert not torch.equal(calm[0], d_P)
    batch.deform_shared_ml_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    assert not torch.equal(calm[0], out[0])          # and now the second models'
    _close(engines, batch)


def test_a_second_rest_array_is_invalid(hip_lib):
    N, M, L, F = 1000, 64, 4, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    outs = [torch.empty_like(d_P) for _ in range(F)]
    d_rest = [torch.from_numpy(rest).to(DEV()) for _ in range(2)]
    d_del = torch.from_numpy(_deltas(rest, F)).to(DEV())
    engines = [capi.Engine() for _ in range(F)]
    for e in engines:
        e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [1.0, L, 0.1]); e.set_term(capi.TERM_LINEAR)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rest[0].data_ptr(), d_rest[1].data_ptr(), d_rest[0].data_ptr()], [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_ml_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in outs])
    assert ei.value.code == capi.FD_E_INVALID and "one rest rig" in str(ei.value)
    _close(engines, batch)


@pytest.mark.parametrize("case", ["thin_plate", "qnn", "ml_eval_variant", "ml_imported"])
def test_everything_else_is_the_fp64_call_bit_for_bit(hip_lib, case):
    N, M, L, F = 1500, 64, 4, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    kw = {"thin_plate": dict(kind=capi.KERNEL_THIN_PLATE, params=[]), "qnn": dict(kind=capi.KERNEL_GAUSSIAN_QNN, params=[1.0, 5.0]),
          "ml_eval_variant": dict(variant=2), "ml_imported": {}}[case]
    engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), **kw)
    extra = []
    if case == "ml_imported":
        for e in engines:
            peer = capi.Engine(); peer.import_model(e.export_model()); extra.append(peer)
        target = capi.Batch(extra)
    else:
        target = batch
    before, new, after = Outs(N, F), Outs(N, F), Outs(N, F)
    _call(target, "deform_shared_fp64_dev", N, d, before, True)
    _call(target, "deform_shared_ml_fp64_dev", N, d, new, True)
    _call(target, "deform_shared_fp64_dev", N, d, after, True)      # ... and the existing call after it is unaffected
    torch.cuda.synchronize()
    Pb, fb = before.host(); Pn, fn = new.host(); Pa, fa = after.host()
    for f in range(F):
        assert not np.array_equal(Pb[f], P)
        assert np.array_equal(Pb[f], Pn[f]) and np.array_equal(fb[f], fn[f])
        assert np.array_equal(Pb[f], Pa[f]) and np.array_equal(fb[f], fa[f])
    if extra:
        target.close()
        for e in extra:
            e.close()
    _close(engines, batch)


# ---- 5. the contexts' precision setting does not matter ------------------------------------------------------------------
def test_fp32_and_fp64_contexts_give_the_same_bits(hip_lib):
    N, M, L, F = 1500, 40, 3, 13
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    outs = {}
    for precision in (capi.EVAL_FP32, capi.EVAL_FP64):
        engines, batch, keep = _engines(M, L, F, rest, _deltas(rest, F), 0.5, 0.05, capi.TERM_CONST, precision=precision)
        o = Outs(N, F)
        _call(batch, "deform_shared_ml_fp64_dev", N, d, o, True)
        torch.cuda.synchronize()
        outs[precision] = o.host()
        _close(engines, batch)
    (Pa, fa), (Pb, fb) = outs[capi.EVAL_FP32], outs[capi.EVAL_FP64]
    assert not np.array_equal(Pa[0], P)
    for f in range(F):
        assert np.array_equal(Pa[f], Pb[f]) and np.array_equal(fa[f], fb[f])
