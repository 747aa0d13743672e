"""GPU: fd_batch_deform_shared_fp64_dev -- every frame of a shared-rig batch evaluated in fp64 by one matrix-pipe launch
(k_deform64_shared).

Yardsticks, fixed in advance:
  * the per-frame fp64 evaluation (fd_batch_deform_dev on FD_EVAL_FP64 contexts): the two differ only in the order of the
    fp64 summation ahead of ONE rounding to fp32, so every output component is within one fp32 ulp and every fd_falloff
    value is bit-identical; the share of components that are not bit-identical is printed, not bounded;
  * the oracle, at the bars the project applies to its fp64 evaluation: parity_ratio at 2e-7 on the golden cases
    (test_gpu_parity.py) and the raw displacement figure <= 1e-5 at C2 (test_gpu_raw_delta.py)."""
import numpy as np
import pytest
import torch

from conftest import case_kind_term, parity_ratio
from facedeform_amd import capi, synth
from oracle import fd_oracle as fo
from test_gpu_bench_launch import _sample_indices
from test_gpu_raw_delta import TOL, _ref_delta, raw_delta_metric
from test_gpu_vectors import _inputs, RADIUS2, RATE

pytestmark = pytest.mark.gpu

NAME = "k_deform64_shared"
KINDS = {
    "thin_plate": (capi.KERNEL_THIN_PLATE, lambda M: []),
    "gaussian": (capi.KERNEL_GAUSSIAN, lambda M: [1.2 / M ** (1 / 3)]),
    "qnn": (capi.KERNEL_GAUSSIAN_QNN, lambda M: [1.0, 5.0]),
    "biharmonic": (capi.KERNEL_BIHARMONIC, lambda M: []),
    "cubic": (capi.KERNEL_CUBIC, lambda M: []),
}
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
SENTINEL = -7.25
DEV = lambda: torch.device("cuda", 0)


def _deltas(rest, F):
    return np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)


def _engines(kind, params, term, M, F, rest, deltas, precision=capi.EVAL_FP64, stream=None):
    d_rest = torch.from_numpy(rest).to(DEV())
    d_del = torch.from_numpy(np.ascontiguousarray(deltas)).to(DEV())
    engines = []
    for _ in range(F):
        e = capi.Engine(precision=precision)
        if stream is not None:
            e.set_stream(stream)
        e.set_kernel(kind, list(params)); e.set_term(term)
        engines.append(e)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(stream)
    return engines, batch, (d_rest, d_del)


def _close(engines, *batches):
    for b in batches:
        b.close()
    for e in engines:
        e.set_stream(None); e.close()


def _mesh(N):
    return synth.head_mesh(max(N, 20_000))[:: max(N, 20_000) // N][:N].copy()


class Outs:
    """Outputs of one call, N + 64 entries each: the tail is a canary (entries past N are not touched)."""
    def __init__(self, N, F, fall_fill=SENTINEL):
        full = lambda w, v: torch.full((N + 64, w) if w else (N + 64,), float(v), device=DEV())
        self.N, self.F = N, F
        self.P = [full(3, SENTINEL) for _ in range(F)]
        self.fall = [full(0, fall_fill) for _ in range(F)]
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() for t in self.P], [t.data_ptr() for t in self.fall]

    def host(self):
        P = [t.cpu().numpy() for t in self.P]; fall = [t.cpu().numpy() for t in self.fall]
        for p, f in zip(P, fall):
            assert (p[self.N:] == np.float32(SENTINEL)).all() and (f[self.N:] == np.float32(SENTINEL)).all()
        return [p[:self.N] for p in P], [f[:self.N] for f in fall]


def _mode_args(d, full):
    return dict(d_dist2=d["d2"].data_ptr() if full else 0, d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if full else None,
                radius2=RADIUS2, falloffrate=RATE)


def _device_inputs(P):
    tu, tv, nrm, _, dist2 = _inputs(P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV())
    return dist2, {"P": t(P), "tu": t(tu), "tv": t(tv), "nrm": t(nrm), "d2": t(dist2)}


def _within_one_ulp(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)).all())


# ---- 1. against the per-frame fp64 evaluation ------------------------------------------------------------------------
@pytest.mark.parametrize("term", list(TERMS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_matches_the_per_frame_fp64_evaluation(hip_lib, kind, term):
    kc, params = KINDS[kind]
    N = 1500
    P = _mesh(N)
    dist2, d = _device_inputs(P)
    differ = total = 0
    for M in (32, 96, 256, 512):
        rest = synth.control_points(M, "head")
        engines, batch32, keep = _engines(kc, params(M), TERMS[term], M, 32, rest, _deltas(rest, 32))
        assert [r.terminationtype for r in batch32.build_result()] == [1] * 32
        for F in (1, 3, 13, 17, 20, 32):
            assert capi.fd_shared_fp64_kernel_name(M, F, kc) == NAME
            batch = capi.Batch(engines[:F])
            for output in (capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT):
                for e in engines[:F]:
                    e.set_output(output)
                for full in (False, True):
                    new, ref = Outs(N, F), Outs(N, F)
                    a = _mode_args(d, full)
                    po, fo_ = new.ptrs()
                    batch.deform_shared_fp64_dev(N, d["P"].data_ptr(), po, d_falloff=fo_, **a)
                    po, fo_ = ref.ptrs()
                    tang = None if not full else tuple([p] * F for p in a["d_tangents"])
                    batch.deform_dev(N, [d["P"].data_ptr()] * F, po, d_dist2=[a["d_dist2"]] * F if full else None, d_falloff=fo_,
                                     d_tangents=tang, radius2=RADIUS2, falloffrate=RATE)
                    torch.cuda.synchronize()
                    Pn, fn = new.host(); Pr, fr = ref.host()
                    for f in range(F):
                        assert np.isfinite(Pn[f]).all()
                        assert _within_one_ulp(Pn[f], Pr[f]), (kind, term, M, F, output, full, f)
                        assert np.array_equal(fn[f], fr[f]), (kind, term, M, F, output, full, f)
                        differ += int((Pn[f] != Pr[f]).sum()); total += Pn[f].size
            batch.close()
        for e in engines:
            e.set_output(capi.OUTPUT_POSITION)
        _close(engines, batch32)
    print(f"\nshared fp64 vs per-frame fp64, {kind}/{term}: {differ} of {total} components not bit-identical ({differ / total:.2e})")


# ---- 2. against the oracle --------------------------------------------------------------------------------------------
def test_golden_cases_at_the_fp64_bar(hip_lib, golden):
    """Every golden case (cubic among them, which fp32 holds only to 3e-5) as a 3-frame shot of its own deltas scaled."""
    for name in [str(n) for n in golden["names"]]:
        kind, term = case_kind_term(name)
        rest, deform, params = golden[name + "/rest"].astype(np.float32), golden[name + "/deform"], golden[name + "/params"]
        P = golden[name + "/x"].astype(np.float32)
        M, N, F = rest.shape[0], P.shape[0], 3
        assert capi.fd_shared_fp64_kernel_name(M, F, kind) == NAME
        delta = (np.asarray(deform, np.float32) - rest).astype(np.float32)
        engines, batch, keep = _engines(kind, list(params), term, M, F, rest, np.stack([delta] * F), precision=capi.EVAL_FP32)
        assert [r.terminationtype for r in batch.build_result()] == [1] * F
        out = Outs(N, F)
        po, fo_ = out.ptrs()
        d_P = torch.from_numpy(P).to(DEV())
        torch.cuda.synchronize()
        batch.deform_shared_fp64_dev(N, d_P.data_ptr(), po, d_falloff=fo_)
        torch.cuda.synchronize()
        Pn, fn = out.host()
        ref = P + golden[name + "/delta"].astype(np.float32)
        for f in range(F):
            r = parity_ratio(Pn[f], ref, P, 2e-7)
            print(f"golden {name} frame {f}: parity ratio at 2e-7 = {r:.3f}")
            assert r <= 1.0, (name, f, r)
            assert np.array_equal(fn[f], np.ones(N, np.float32))
        _close(engines, batch)


def _raw_case(oracle, N, M, F, phases, kind=capi.KERNEL_THIN_PLATE, okind=fo.KERNEL_THIN_PLATE, params=(), sample=None, tag=""):
    P = synth.head_mesh(N); rest = synth.control_points(M, "head")
    P[:8] = rest[:8]
    deltas = np.stack([synth.rig_deltas(rest, f) for f in phases])
    d_P = torch.from_numpy(P).to(DEV())
    engines, batch, keep = _engines(kind, list(params), capi.TERM_LINEAR, M, F, rest, deltas[:F], precision=capi.EVAL_FP32)
    d_rest, _ = keep
    d_del = torch.from_numpy(deltas).to(DEV())
    assert capi.fd_shared_fp64_kernel_name(M, F, kind) == NAME
    for e in engines:
        e.set_output(capi.OUTPUT_DISPLACEMENT)
    idx = _sample_indices(N, 256) if sample is None else sample
    Ps = np.ascontiguousarray(P[idx]); sel = torch.from_numpy(idx).to(DEV())
    dels = [torch.empty_like(d_P) for _ in range(F)]
    worst = 0.0
    for first in range(0, len(phases), F):
        batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + (first + k) * M * 12 for k in range(F)], M)
        batch.build_async()
        batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [o.data_ptr() for o in dels])
        torch.cuda.synchronize()
        assert [r.terminationtype for r in batch.build_result()] == [1] * F
        for k in range(F):
            d_gpu = dels[k][sel].cpu().numpy()
            assert np.isfinite(d_gpu).all()
            if okind == fo.KERNEL_THIN_PLATE:
                d_ref = _ref_delta(oracle, rest, deltas[first + k], Ps)
            else:
                table = np.concatenate([rest, deltas[first + k]], axis=1).astype(np.float64)
                rc, tt, W, radii = oracle.build(table, okind, list(params), fo.TERM_LINEAR)
                assert tt == 1
                d_ref = oracle.eval(table, okind, radii, W, Ps.astype(np.float64))
            m = raw_delta_metric(d_gpu, d_ref)
            worst = max(worst, m)
            assert m <= TOL, (tag, phases[first + k], m)
    print(f"\n{tag}: worst raw displacement metric {worst:.3e} over {len(phases)} phases, {idx.size} sampled vertices")
    _close(engines, batch)
    return worst


def test_raw_displacement_c2_all_64_phases_32_frames(hip_lib, oracle):
    _raw_case(oracle, 1_000_000, 256, 32, list(range(64)), tag="C2 x 32 frames, shared fp64")


def test_raw_displacement_c2_20_frames_per_launch(hip_lib, oracle):
    _raw_case(oracle, 1_000_000, 256, 20, list(range(60)), tag="C2 x 20 frames, shared fp64")


def test_raw_displacement_fixed_radius_gaussian(hip_lib, oracle):
    _raw_case(oracle, 200_000, 256, 32, list(range(32)), kind=capi.KERNEL_GAUSSIAN, okind=fo.KERNEL_GAUSSIAN, params=(0.5,),
              sample=np.arange(0, 200_000, 97), tag="Gaussian R = 0.5, M = 256, shared fp64")


def test_raw_displacement_2048_control_points(hip_lib, oracle):
    idx = np.unique(np.concatenate([np.arange(0, 8), np.arange(0, 1_000_000, 997), np.arange(999_936, 1_000_000)]))
    _raw_case(oracle, 1_000_000, 2048, 32, list(range(32)), sample=idx, tag="C3 (M = 2048) x 32 frames, shared fp64")


# ---- 3. pass-through, 4. range split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("output", [capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT])
def test_gated_vertices_and_a_failed_build_pass_through(hip_lib, output):
    """A third of the vertices gated, and the last frame's build failed on coincident centres.  The failure is still unknown
    to the host when the call is made (the build sits on the stream behind a long evaluation), so the call is accepted and
    the DEVICE decides: that frame is passed through, like the gated vertices of the others; fd_falloff untouched there."""
    N, M, F, big = 3001, 96, 5, 1_000_000
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    S = torch.cuda.Stream(device=DEV())
    d_rest = torch.from_numpy(rest).to(DEV()); d_del = torch.from_numpy(_deltas(rest, F)).to(DEV())
    engines = []
    for _ in range(F):
        e = capi.Engine(); e.set_stream(S.cuda_stream); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR); engines.append(e)
    head, lone, batch = capi.Batch(engines[:-1]), capi.Batch([engines[-1]]), capi.Batch(engines)
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
    for _ in range(60):          # keeps the stream busy for several milliseconds
        head.deform_shared_fp64_dev(big, d_big.data_ptr(), [t.data_ptr() for t in scratch], stream_ptr=S.cuda_stream)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream)
    batch.deform_shared_fp64_dev(N, d["P"].data_ptr(), po, d_falloff=fo_, stream_ptr=S.cuda_stream, **_mode_args(d, True))
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


@pytest.mark.parametrize("kind", ["thin_plate", "cubic"])
def test_range_split_is_bit_identical(hip_lib, kind):
    kc, params = KINDS[kind]
    N, M, F, cut = 5003, 256, 17, 1237
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    engines, batch, keep = _engines(kc, params(M), capi.TERM_LINEAR, M, F, rest, _deltas(rest, F))
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    one, two = Outs(N, F), Outs(N, F)
    a = _mode_args(d, True)
    po, fo_ = one.ptrs()
    batch.deform_shared_fp64_dev(N, d["P"].data_ptr(), po, d_falloff=fo_, **a)
    po, fo_ = two.ptrs()
    batch.deform_shared_fp64_dev(cut, d["P"].data_ptr(), po, d_falloff=fo_, **a)
    off = lambda p, w: p + 4 * w * cut
    a2 = dict(a, d_dist2=off(a["d_dist2"], 1), d_tangents=tuple(off(p, 3) for p in a["d_tangents"]))
    batch.deform_shared_fp64_dev(N - cut, off(d["P"].data_ptr(), 3), [off(p, 3) for p in po], d_falloff=[off(p, 1) for p in fo_], **a2)
    torch.cuda.synchronize()
    P1, f1 = one.host(); P2, f2 = two.host()
    for f in range(F):
        assert np.array_equal(P1[f], P2[f]) and np.array_equal(f1[f], f2[f])
    _close(engines, batch)


# ---- 5. repeatability, 8. rebuild behind fd_batch_wait_consumed --------------------------------------------------------
@pytest.mark.parametrize("kind", ["thin_plate", "qnn"])
def test_two_launches_give_the_same_bits_and_rebuild_behind_wait_consumed(hip_lib, kind):
    kc, params = KINDS[kind]
    N, M, F = 1_000_000, 256, 32
    P = synth.head_mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    sA, sB = torch.cuda.Stream(device=DEV()), torch.cuda.Stream(device=DEV())
    deltas = _deltas(rest, F)
    engines, batch, keep = _engines(kc, params(M), capi.TERM_LINEAR, M, F, rest, deltas, precision=capi.EVAL_FP32, stream=sA.cuda_stream)
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    first = [torch.empty_like(d_P) for _ in range(F)]
    second = [torch.empty_like(d_P) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in first], stream_ptr=sA.cuda_stream)
    batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in second], stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], d_P)
    # the same launch again, and the NEXT models built on another stream behind fd_batch_wait_consumed while it runs
    other = torch.from_numpy(np.ascontiguousarray(deltas[::-1] * np.float32(0.5))).to(DEV())
    torch.cuda.synchronize()
    batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in second], stream_ptr=sA.cuda_stream)
    batch.wait_consumed(sB.cuda_stream)
    batch.set_points_dev([keep[0].data_ptr()] * F, [other.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(sB.cuda_stream)
    torch.cuda.synchronize()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    for a, b in zip(first, second):
        assert torch.equal(a, b)                 # the first models' outputs
    batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [t.data_ptr() for t in second], stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    assert not torch.equal(first[0], second[0])  # and now the second models'
    _close(engines, batch)


# ---- 6. fallback, 7. settings left alone, 9. errors -------------------------------------------------------------------
def test_multilayer_runs_the_per_context_fp64_launches(hip_lib):
    N, M, F = 4000, 64, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    dist2, d = _device_inputs(P)
    assert capi.fd_shared_fp64_kernel_name(M, F, capi.KERNEL_GAUSSIAN_ML) == ""
    engines, batch, keep = _engines(capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1], capi.TERM_LINEAR, M, F, rest, _deltas(rest, F), precision=capi.EVAL_FP32)
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    new, ref = Outs(N, F), Outs(N, F)
    a = _mode_args(d, True)
    po, fo_ = new.ptrs()
    batch.deform_shared_fp64_dev(N, d["P"].data_ptr(), po, d_falloff=fo_, **a)
    torch.cuda.synchronize()
    po, fo_ = ref.ptrs()
    for f, e in enumerate(engines):
        e.set_eval_precision(capi.EVAL_FP64)
        tu, tv, nr = a["d_tangents"]
        e.deform_dev(N, d["P"].data_ptr(), po[f], d_dist2=a["d_dist2"], d_falloff=fo_[f], d_tu=tu, d_tv=tv, d_nrm=nr, radius2=RADIUS2, falloffrate=RATE)
        e.synchronize()
    Pn, fn = new.host(); Pr, fr = ref.host()
    for f in range(F):
        assert np.array_equal(Pn[f], Pr[f]) and np.array_equal(fn[f], fr[f])
    _close(engines, batch)


def test_contexts_settings_and_the_fp32_scratch_are_left_alone(hip_lib):
    N, M, F = 20_000, 256, 20
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    engines, batch, keep = _engines(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest, _deltas(rest, F), precision=capi.EVAL_FP32)
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    assert capi.load().fd_shared_kernel_name(M, F, capi.KERNEL_THIN_PLATE).decode() != ""
    before, mid, after = Outs(N, F), Outs(N, F), Outs(N, F)
    po, fo_ = before.ptrs()
    batch.deform_shared_dev(N, d_P.data_ptr(), po, d_falloff=fo_)
    po, fo_ = mid.ptrs()
    batch.deform_shared_fp64_dev(N, d_P.data_ptr(), po, d_falloff=fo_)
    po, fo_ = after.ptrs()
    batch.deform_shared_dev(N, d_P.data_ptr(), po, d_falloff=fo_)
    torch.cuda.synchronize()
    Pb, _ = before.host(); Pm, _ = mid.host(); Pa, _ = after.host()
    differs = False
    for f in range(F):
        assert np.array_equal(Pb[f], Pa[f])                       # the fp32 launch before and after: same bits
        differs |= not np.array_equal(Pb[f], Pm[f])
    assert differs                                                # ... and the call between them was not the fp32 launch
    # the contexts still evaluate in fp32: their own launch gives the fp32 one-frame kernel's bits, not the fp64 one's
    own32 = torch.empty_like(d_P); own64 = torch.empty_like(d_P)
    engines[0].deform_dev(N, d_P.data_ptr(), own32.data_ptr()); engines[0].synchronize()
    engines[0].set_eval_precision(capi.EVAL_FP64)
    engines[0].deform_dev(N, d_P.data_ptr(), own64.data_ptr()); engines[0].synchronize()
    assert not torch.equal(own32, own64)
    assert _within_one_ulp(Pm[0], own64.cpu().numpy())
    _close(engines, batch)


def test_errors(hip_lib):
    N, M, F = 1000, 64, 3
    P = _mesh(N); rest = synth.control_points(M, "head")
    d_P = torch.from_numpy(P).to(DEV())
    outs = [torch.empty_like(d_P) for _ in range(F)]
    ptr = [t.data_ptr() for t in outs]
    # a context without a model
    engines = [capi.Engine() for _ in range(F)]
    batch = capi.Batch(engines)
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_fp64_dev(N, d_P.data_ptr(), ptr)
    assert ei.value.code == capi.FD_E_NOT_BUILT
    _close(engines, batch)
    # different rest arrays
    d_rest = [torch.from_numpy(rest).to(DEV()) for _ in range(F)]
    d_del = torch.from_numpy(_deltas(rest, F)).to(DEV())
    engines = [capi.Engine() for _ in range(F)]
    for e in engines:
        e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    batch = capi.Batch(engines)
    batch.set_points_dev([t.data_ptr() for t in d_rest], [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_fp64_dev(N, d_P.data_ptr(), ptr)
    assert ei.value.code == capi.FD_E_INVALID
    _close(engines, batch)
    # an output over a shared input, more than one frame
    engines, batch, keep = _engines(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest, _deltas(rest, F))
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    with pytest.raises(capi.FdError) as ei:
        batch.deform_shared_fp64_dev(N, d_P.data_ptr(), [ptr[0], d_P.data_ptr(), ptr[2]])
    assert ei.value.code == capi.FD_E_INVALID
    # one frame in place is allowed, and gives the out-of-place bits
    one = capi.Batch(engines[:1])
    one.deform_shared_fp64_dev(N, d_P.data_ptr(), ptr[:1])
    inplace = d_P.clone(); torch.cuda.synchronize()
    one.deform_shared_fp64_dev(N, inplace.data_ptr(), [inplace.data_ptr()])
    torch.cuda.synchronize()
    assert torch.equal(inplace, outs[0])
    _close(engines, one, batch)
