"""GPU: fd_batch_set_shared_lu -- a shot of QNN models (the SOP's default, reference src/SOP_FaceDeform.cpp:342-345) built
from ONE LU of the rest rig's kernel block, every frame's right-hand sides through it in one launch
(facedeform_amd/csrc/fd_build_qnn_shared.hip k_qnn_solve_shared) -- against the oracle
(oracle.build(table, KERNEL_GAUSSIAN_QNN, [q, z, smoothing], term)), against the per-context builds, and the contract of
include/facedeform_hip.h: delegation bit for bit, the fall-back to the pivoted LU, statuses, repeatability.

The bar on weights is the project's bar for builds, 1e-8 of max |W|.  The QNN kernel blocks have condition
numbers of 10 - 20 at q = 1: eps * cond is about 4e-15 and the bar leaves decades."""
import numpy as np
import pytest
import torch

from conftest import parity_ratio
from facedeform_amd import capi, synth
from oracle import fd_oracle as fo
from test_shared_qnn_build_abi import NAME, threshold

pytestmark = pytest.mark.gpu

RADIUS2, RATE = 1.0, 1.5
Z = 5.0
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
DEV = lambda: torch.device("cuda", 0)

#        M    F   q    lam  term       why this size
GRID = [(20, 2, 1.0, 0.0, "zero"),        # one block, smallest batch, partial tile
        (33, 5, 1.0, 0.0, "linear"),      # ragged second block, 15 columns
        (40, 17, 1.0, 0.0, "const"),      # 51 columns, frame 5 straddles two tiles
        (100, 32, 1.0, 0.0, "linear"),    # six full tiles
        (256, 32, 1.0, 0.0, "linear"),    # node defaults, z = 5
        (64, 4, 2.0, 0.0, "linear"),      # multipliers between 1 and 4 let through
        (64, 3, 1.0, 0.1, "linear"),      # lambda on the diagonal
        (700, 6, 1.0, 0.0, "linear"),     # many blocks
        (1000, 2, 1.0, 0.0, "linear")]    # the largest M tests/test_gpu_qnn_nopivot.py builds


def _deltas(rest, F, flip=False):
    """The deltas the device is given are those of the oracle's table: control_table(rest, rest + delta) holds the fp32 sum,
    whose distance from rest is the delta only to fp32 rounding -- so the deformed rig is formed first and the deltas are
    taken from it, as tests/test_gpu_shared_ml_build.py does."""
    d = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    d = np.ascontiguousarray(d[::-1] * np.float32(0.5)) if flip else d
    deform = (rest[None] + d).astype(np.float32)
    return np.ascontiguousarray((deform - rest[None]).astype(np.float32))


def _oracle(oracle, rest, delta, q, lam, term):
    table = oracle.control_table(rest, rest + delta)
    rc, tt, Wo, radii = oracle.build(table, fo.KERNEL_GAUSSIAN_QNN, [q, Z, lam], TERMS[term])
    return tt, table, Wo, radii


_CASES = {}


def _case(oracle, row):
    """Rest rig, deltas and the oracle's model per frame of one grid row: computed once, shared, never changed."""
    if row not in _CASES:
        M, F, q, lam, term = row
        rest = synth.control_points(M, "head")
        deltas = _deltas(rest, F)
        refs = []
        for f in range(F):
            tt, table, Wo, radii = _oracle(oracle, rest, deltas[f], q, lam, term)
            assert tt == 1
            for a in (table, Wo, radii):
                a.setflags(write=False)
            refs.append((table, Wo, radii))
        rest.setflags(write=False); deltas.setflags(write=False)
        _CASES[row] = (rest, deltas, refs)
    return _CASES[row]


class Shot:
    """F contexts of one model in one batch (QNN unless `kernel` says otherwise), the device arrays they read in place."""
    def __init__(self, M, F, q, lam, term, stream=None, kernel=None):
        self.M, self.F = M, F
        self.engines = []
        for _ in range(F):
            e = capi.Engine()
            if stream is not None:
                e.set_stream(stream)
            e.set_kernel(*(kernel or (capi.KERNEL_GAUSSIAN_QNN, [q, Z, lam]))); e.set_term(TERMS[term])
            self.engines.append(e)
        self.batch = capi.Batch(self.engines)
        self.keep = []

    def build(self, rest, deltas, on, stream=None, wait=True, rest_ptrs=None, check=False):
        """rest, deltas: numpy arrays (uploaded here, then a device synchronisation) or tensors already on the device."""
        fresh = not (isinstance(rest, torch.Tensor) and isinstance(deltas, torch.Tensor))
        d_rest = rest if isinstance(rest, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rest)).to(DEV())
        d_del = deltas if isinstance(deltas, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(deltas)).to(DEV())
        self.keep += [d_rest, d_del]
        if fresh:
            torch.cuda.synchronize()
        self.batch.set_shared_lu(on)
        self.batch.set_points_dev(rest_ptrs or [d_rest.data_ptr()] * self.F, [d_del.data_ptr() + f * self.M * 12 for f in range(self.F)], self.M)
        self.batch.build_async(stream)
        if wait:
            self.reports = self.batch.build_result(check=check)
            return [r.terminationtype for r in self.reports]

    def weights(self):
        return [e.get_weights()[0] for e in self.engines]

    def radii(self):
        return [e.get_weights()[1] for e in self.engines]

    def close(self):
        self.batch.close()
        for e in self.engines:
            e.set_stream(None); e.close()


# ---- 1. weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", GRID, ids=lambda r: f"M{r[0]}_F{r[1]}_q{r[2]:g}_lam{r[3]:g}_{r[4]}")
def test_weights_against_the_oracle_with_the_switch_on_and_off(hip_lib, oracle, row):
    """Both paths within 1e-8 of max |W| of the oracle, per frame; the on-to-off distance is printed (DESIGN.md 4.2i records
    it; it has no bar of its own).  Radii, solver, iteration count and order are those of the per-context build."""
    M, F, q, lam, term = row
    assert F >= threshold() and capi.fd_shared_qnn_build_kernel_name(M, F) == NAME
    rest, deltas, refs = _case(oracle, row)
    shot = Shot(*row)
    got, radii, reps = {}, {}, {}
    for on in (True, False):
        tts = shot.build(rest, deltas, on)
        assert shot.batch.last_build_shared_factor() is on
        assert tts == [1] * F
        got[on], radii[on], reps[on] = shot.weights(), shot.radii(), shot.reports
    worst = {True: 0.0, False: 0.0}
    apart = 0.0
    for f in range(F):
        Wo = refs[f][1]
        scale = np.abs(Wo).max()
        for on in (True, False):
            assert got[on][f].shape == Wo.shape
            worst[on] = max(worst[on], np.abs(got[on][f] - Wo).max() / scale)
        apart = max(apart, np.abs(got[True][f] - got[False][f]).max() / scale)
        assert np.array_equal(radii[True][f], radii[False][f])
        a, b = reps[True][f], reps[False][f]
        assert a.solver_used == capi.SOLVER_LU_NOPIVOT and b.solver_used == capi.SOLVER_LU_NOPIVOT
        assert a.iterationscount == b.iterationscount and a.n == b.n
        assert a.pivot_ratio == b.pivot_ratio          # the same matrix, the same factorisation kernels
    print(f"shared qnn build M={M} F={F} q={q:g} lam={lam:g} {term}: on {worst[True]:.3e}, off {worst[False]:.3e}, on-to-off {apart:.3e} (of max |W|)")
    assert worst[True] <= 1e-8 and worst[False] <= 1e-8
    shot.close()


# ---- 2. through the evaluation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [GRID[2], GRID[4]], ids=lambda r: f"M{r[0]}_F{r[1]}")
def test_models_built_this_way_evaluate_within_the_bar(hip_lib, oracle, row):
    M, F, q, lam, term = row
    N = 4099
    P = synth.head_mesh(20_000)[:: 20_000 // N][:N].copy()
    dist2 = np.linspace(0.0, 1.2, N).astype(np.float32)
    rest, deltas, refs = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(dist2).to(DEV())
    out = [torch.empty_like(d_P) for _ in range(F)]
    fall = [torch.empty(N, device=DEV()) for _ in range(F)]
    shot.batch.deform_shared_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], d_dist2=d_d2.data_ptr(),
                                 d_falloff=[t.data_ptr() for t in fall], radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    for f in range(F):
        table, Wo, radii = refs[f]
        ref, _ = oracle.deform(table, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P, dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
        r = parity_ratio(out[f].cpu().numpy(), ref, P, 1e-5)
        print(f"shared qnn build M={M} F={F} evaluated, frame {f}: {r:.3f} of the bar")
        assert r <= 1.0, (f, r)
    shot.close()


# ---- 3. delegation, bit for bit ----------------------------------------------------------------------------------------------
def _on_equals_off(shot, rest, deltas, rest_ptrs=None):
    """Both settings of the switch build per context: the same statuses, and where a model was built the same bits."""
    got = {}
    for on in (True, False):
        tts = shot.build(rest, deltas, on, rest_ptrs=rest_ptrs)
        assert shot.batch.last_build_shared_factor() is False
        got[on] = (tts, [e.get_weights()[0] if tt == 1 else None for e, tt in zip(shot.engines, tts)],
                   [r.solver_used for r in shot.reports])
    assert got[True][0] == got[False][0] and got[True][2] == got[False][2]
    for a, b in zip(got[True][1], got[False][1]):
        assert (a is None and b is None) or np.array_equal(a, b)
    return got[True][0]


@pytest.mark.parametrize("case", ["second_rest_array", "one_context", "below_threshold", "m1025", "m3_linear"])
def test_a_batch_that_misses_a_condition_is_built_as_without_the_switch(hip_lib, case):
    t = threshold()
    if case == "below_threshold" and t <= 2:
        # (no frame count between "one context alone" and the threshold: "one_context" is that case)
        assert t == 2
        case = "one_context"
    M, F = {"second_rest_array": (64, 4), "one_context": (64, 1), "below_threshold": (64, t - 1), "m1025": (1025, 2), "m3_linear": (3, 2)}[case]
    rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    shot = Shot(M, F, 1.0, 0.0, "linear")
    if case == "second_rest_array":
        shared = torch.from_numpy(rest).to(DEV()); other = torch.from_numpy((rest * np.float32(1.01)).astype(np.float32)).to(DEV())
        d_del = torch.from_numpy(deltas).to(DEV())
        shot.keep += [other]
        torch.cuda.synchronize()
        tts = _on_equals_off(shot, shared, d_del, rest_ptrs=[other.data_ptr() if f == 2 else shared.data_ptr() for f in range(F)])
    else:
        tts = _on_equals_off(shot, rest, deltas)
    if case != "m3_linear":                       # (fewer points than polynomial columns: there is no fit at all, with either setting)
        assert tts == [1] * F
    shot.close()


def test_contexts_that_fell_back_to_the_pivoted_lu_keep_the_batch_per_context(hip_lib):
    """q = 3 built with the switch OFF: every context comes back through the pivoted LU and keeps it for this rig; the batch then
    misses the condition with the switch on."""
    M, F = 100, 3
    rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    shot = Shot(M, F, 3.0, 0.0, "linear")
    assert shot.build(rest, deltas, False) == [1] * F
    assert [r.solver_used for r in shot.reports] == [capi.SOLVER_LU] * F
    assert _on_equals_off(shot, rest, deltas) == [1] * F
    assert [r.solver_used for r in shot.reports] == [capi.SOLVER_LU] * F
    shot.close()


@pytest.mark.parametrize("family", ["thin_plate", "multilayer"])
def test_the_switch_does_not_touch_other_families(hip_lib, family):
    M, F = 64, 3
    rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    kernel = (capi.KERNEL_THIN_PLATE, []) if family == "thin_plate" else (capi.KERNEL_GAUSSIAN_ML, [0.7, 3, 0.1])
    shot = Shot(M, F, 1.0, 0.0, "linear", kernel=kernel)
    assert _on_equals_off(shot, rest, deltas) == [1] * F
    shot.close()


def test_set_shared_factor_alone_still_builds_a_qnn_batch_per_frame(hip_lib, oracle):
    """What tests/test_gpu_shared_factor.py holds of fd_batch_set_shared_factor, next to the new switch: that switch alone
    leaves a QNN batch to the per-context builds, whose bits are those of a build with neither switch."""
    row = GRID[1]
    M, F, q, lam, term = row
    rest, deltas, _ = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, False) == [1] * F
    plain = shot.weights()
    shot.batch.set_shared_factor(True)
    assert shot.build(rest, deltas, False) == [1] * F
    assert shot.batch.last_build_shared_factor() is False
    for a, b in zip(plain, shot.weights()):
        assert np.array_equal(a, b)
    # ... and both switches: the new one decides for a QNN batch
    assert shot.build(rest, deltas, True) == [1] * F
    assert shot.batch.last_build_shared_factor() is True
    shot.close()


def test_with_the_switch_off_the_batch_equals_single_builds_bitwise(hip_lib, oracle):
    row = GRID[3]
    M, F, q, lam, term = row
    rest, deltas, _ = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, False) == [1] * F
    Wb = shot.weights()
    for f in (0, 5, F - 1):
        e = capi.Engine()
        e.set_kernel(capi.KERNEL_GAUSSIAN_QNN, [q, Z, lam]); e.set_term(TERMS[term])
        e.set_points(rest, deltas[f])
        assert e.build().terminationtype == 1
        assert np.array_equal(e.get_weights()[0], Wb[f])
        e.close()
    shot.close()


# ---- 4. fallback -----------------------------------------------------------------------------------------------------------
def test_q3_takes_the_shared_path_reports_minus_4_and_comes_back_through_the_pivoted_lu(hip_lib, oracle):
    """The rig of test_q3_falls_back_to_the_pivoted_lu (multipliers in the thousands): the shared factorisation flags it, every
    frame reports -4, fd_build_result repairs every context with the pivoted LU; the batch then builds per context."""
    M, F = 100, 4
    assert capi.fd_shared_qnn_build_kernel_name(M, F) == NAME
    rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    shot = Shot(M, F, 3.0, 0.0, "linear")
    tts = shot.build(rest, deltas, True)
    assert shot.batch.last_build_shared_factor() is True          # the path was taken; its factorisation asked for the pivoted LU
    assert tts == [1] * F
    assert [r.solver_used for r in shot.reports] == [capi.SOLVER_LU] * F
    for f, W in enumerate(shot.weights()):
        tt, _, Wo, _ = _oracle(oracle, rest, deltas[f], 3.0, 0.0, "linear")
        assert tt == 1
        assert np.abs(W - Wo).max() <= 1e-8 * np.abs(Wo).max()
    first = shot.weights()
    assert shot.build(rest, deltas, True) == [1] * F
    assert shot.batch.last_build_shared_factor() is False         # the contexts keep the pivoted LU: the condition is missed
    assert [r.solver_used for r in shot.reports] == [capi.SOLVER_LU] * F
    for a, b in zip(first, shot.weights()):
        assert np.array_equal(a, b)
    shot.close()


# ---- 5. status and repeatability -----------------------------------------------------------------------------------------
def test_coincident_centres_reach_every_frame_and_the_batch_recovers(hip_lib, oracle):
    row = (64, 5, 1.0, 0.0, "linear")
    M, F, q, lam, term = row
    rest, deltas, refs = _case(oracle, row)
    dup = rest.copy(); dup[5] = dup[30]
    shot = Shot(*row)
    assert shot.build(dup, deltas, True) == [-5] * F
    assert shot.batch.last_build_shared_factor()
    assert shot.build(rest, deltas, True) == [1] * F
    assert shot.batch.last_build_shared_factor()
    for f, W in enumerate(shot.weights()):
        assert np.abs(W - refs[f][1]).max() <= 1e-8 * np.abs(refs[f][1]).max()
    shot.close()


def test_two_builds_give_the_same_bits_and_set_deltas_stays_not_built(hip_lib, oracle):
    row = GRID[3]
    M, F, q, lam, term = row
    rest, deltas, _ = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    first = shot.weights()
    assert [r.iterationscount for r in shot.reports] == [M + 4] * F and [r.n for r in shot.reports] == [M + 4] * F
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    for a, b in zip(first, shot.weights()):
        assert np.array_equal(a, b)
    # the factor lived in the batch's scratch: nothing of it in the context
    with pytest.raises(capi.FdError) as ei:
        shot.engines[0].set_deltas(deltas[0])
    assert ei.value.code == capi.FD_E_NOT_BUILT
    shot.close()


# ---- 6. behind fd_batch_wait_consumed ----------------------------------------------------------------------------------------
def test_a_build_behind_wait_consumed_leaves_the_running_evaluation_alone(hip_lib, oracle):
    """Evaluate on one stream, fd_batch_wait_consumed on the build stream, a switch-on build with other deltas there while
    the evaluation runs: its outputs equal an undisturbed run's, and the new models are sound."""
    row = (64, 8, 1.0, 0.0, "linear")
    M, F, q, lam, term = row
    N = 200_000
    rest, deltas, _ = _case(oracle, row)
    other = _deltas(rest, F, flip=True)
    P = synth.head_mesh(N)
    d_P = torch.from_numpy(P).to(DEV())
    d_rest = torch.from_numpy(np.ascontiguousarray(rest)).to(DEV())
    d_first = torch.from_numpy(np.ascontiguousarray(deltas)).to(DEV()); d_other = torch.from_numpy(other).to(DEV())
    sA, sB = torch.cuda.Stream(device=DEV()), torch.cuda.Stream(device=DEV())
    torch.cuda.synchronize()
    shot = Shot(*row, stream=sA.cuda_stream)
    outs = []
    for disturbed in (False, True):
        assert shot.build(d_rest, d_first, True, stream=sA.cuda_stream) == [1] * F and shot.batch.last_build_shared_factor()
        out = [torch.empty_like(d_P) for _ in range(F)]
        torch.cuda.synchronize()
        shot.batch.deform_shared_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], stream_ptr=sA.cuda_stream)
        if disturbed:
            shot.batch.wait_consumed(sB.cuda_stream)
            shot.build(d_rest, d_other, True, stream=sB.cuda_stream, wait=False)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in out])
    assert [r.terminationtype for r in shot.batch.build_result()] == [1] * F and shot.batch.last_build_shared_factor()
    assert not np.array_equal(outs[0][0], P)
    for f in range(F):
        assert np.array_equal(outs[0][f], outs[1][f])
    # the models built meanwhile are those of the other deltas
    tt, _, Wo, _ = _oracle(oracle, rest, other[F - 1], q, lam, term)
    assert np.abs(shot.weights()[F - 1] - Wo).max() <= 1e-8 * np.abs(Wo).max()
    shot.close()
