"""GPU: the multilayer case of fd_batch_set_shared_factor -- a shot of multilayer models built from ONE factorisation per
layer, every frame's right-hand sides through them in one launch (facedeform_amd/csrc/fd_build_ml_shared.hip
k_ml_solve_shared) -- against the numpy oracle (oracle/fd_oracle.py build_multilayer), against the
per-context builds, and the contract of include/facedeform_hip.h: delegation bit for bit, statuses, repeatability.

The bar on weights is the project's bar for builds, 1e-8 of max |W|.  On these rigs every layer matrix
has a condition number of at most 3.3e3 (the worst: M = 1024, R = 1, lambda = 0.1), so eps * cond is about 7e-13 and
the bar leaves four decades."""
import numpy as np
import pytest
import torch

from conftest import parity_ratio
from facedeform_amd import capi, synth
from oracle import fd_oracle as fo
from test_shared_ml_build_abi import NAME, threshold

pytestmark = pytest.mark.gpu

RADIUS2, RATE = 1.0, 1.5
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
DEV = lambda: torch.device("cuda", 0)

#        M    L  F   R    lam   term      why this size
GRID = [(33, 8, 5, 0.7, 0.1, "zero"),        # ragged last 32-block; 15 columns, a partial tile
        (40, 3, 17, 0.5, 0.05, "const"),     # 51 columns: frame 5 straddles tiles 0 / 1; last tile partial
        (100, 4, 32, 0.5, 0.05, "linear"),   # six full tiles; four 32-blocks, the last ragged
        (256, 4, 32, 1.0, 0.1, "linear"),    # the SOP's defaults
        (700, 3, 6, 0.7, 0.1, "linear"),     # many blocks; 90 KB LDS block
        (64, 1, 2, 1.0, 0.1, "const"),       # one layer; the smallest batch
        (1024, 2, 2, 1.0, 0.1, "linear")]    # the LDS limit


def _deltas(rest, F, flip=False):
    """The deltas the device is given are those of the oracle's table: control_table(rest, rest + delta) holds the fp32 sum,
    whose distance from rest is the delta only to fp32 rounding (1e-6 of it) -- so the deformed rig is formed first and the
    deltas are taken from it, as tests/test_gpu_multilayer.py does."""
    d = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    d = np.ascontiguousarray(d[::-1] * np.float32(0.5)) if flip else d
    deform = (rest[None] + d).astype(np.float32)
    return np.ascontiguousarray((deform - rest[None]).astype(np.float32))


_CASES = {}


def _case(oracle, row):
    """Rest rig, deltas and the oracle's model per frame of one grid row: computed once, shared, never changed."""
    if row not in _CASES:
        M, L, F, R, lam, term = row
        rest = synth.control_points(M, "head")
        deltas = _deltas(rest, F)
        refs = []
        for f in range(F):
            tt, table_ml, Wo, radii = oracle.build_multilayer(oracle.control_table(rest, rest + deltas[f]), R, L, lam, TERMS[term])
            assert tt == 1
            for a in (table_ml, Wo, radii):
                a.setflags(write=False)
            refs.append((table_ml, Wo, radii))
        rest.setflags(write=False); deltas.setflags(write=False)
        _CASES[row] = (rest, deltas, refs)
    return _CASES[row]


class Shot:
    """F multilayer contexts in one batch, the device arrays they read in place."""
    def __init__(self, M, L, F, R, lam, term, stream=None):
        self.M, self.F = M, F
        self.engines = []
        for _ in range(F):
            e = capi.Engine()
            if stream is not None:
                e.set_stream(stream)
            e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [R, L, lam]); e.set_term(TERMS[term])
            self.engines.append(e)
        self.batch = capi.Batch(self.engines)
        self.keep = []

    def build(self, rest, deltas, on, stream=None, wait=True):
        """rest, deltas: numpy arrays (uploaded here, then a device synchronisation) or tensors already on the device."""
        fresh = not (isinstance(rest, torch.Tensor) and isinstance(deltas, torch.Tensor))
        d_rest = rest if isinstance(rest, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rest)).to(DEV())
        d_del = deltas if isinstance(deltas, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(deltas)).to(DEV())
        self.keep += [d_rest, d_del]
        if fresh:
            torch.cuda.synchronize()
        self.batch.set_shared_factor(on)
        self.batch.set_points_dev([d_rest.data_ptr()] * self.F, [d_del.data_ptr() + f * self.M * 12 for f in range(self.F)], self.M)
        self.batch.build_async(stream)
        if wait:
            return [r.terminationtype for r in self.batch.build_result(check=False)]

    def weights(self):
        return [e.get_weights()[0] for e in self.engines]

    def close(self):
        self.batch.close()
        for e in self.engines:
            e.set_stream(None); e.close()


# ---- 1. weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", GRID, ids=lambda r: f"M{r[0]}_L{r[1]}_F{r[2]}")
def test_weights_against_the_oracle_with_the_switch_on_and_off(hip_lib, oracle, row):
    """Both paths within 1e-8 of max |W| of the oracle, per frame; the on-to-off distance is printed (DESIGN.md 4.2h
    records it; it has no bar of its own)."""
    M, L, F, R, lam, term = row
    assert capi.fd_shared_ml_build_kernel_name(M, L, F) == NAME
    rest, deltas, refs = _case(oracle, row)
    shot = Shot(*row)
    got = {}
    for on in (True, False):
        tts = shot.build(rest, deltas, on)
        assert shot.batch.last_build_shared_factor() is on
        assert tts == [1] * F
        got[on] = shot.weights()
    worst = {True: 0.0, False: 0.0}
    apart = 0.0
    for f in range(F):
        Wo = refs[f][1]
        scale = np.abs(Wo).max()
        for on in (True, False):
            assert got[on][f].shape == Wo.shape
            worst[on] = max(worst[on], np.abs(got[on][f] - Wo).max() / scale)
        apart = max(apart, np.abs(got[True][f] - got[False][f]).max() / scale)
    print(f"shared ml build M={M} L={L} F={F} {term}: on {worst[True]:.3e}, off {worst[False]:.3e}, on-to-off {apart:.3e} (of max |W|)")
    assert worst[True] <= 1e-8 and worst[False] <= 1e-8
    # the records' radii and the iteration count are those of a per-context build
    for e in shot.engines:
        assert np.array_equal(e.get_weights()[1], np.repeat(R / 2.0 ** np.arange(L), M))
    shot.close()


# ---- 2. lambda = 0 -----------------------------------------------------------------------------------------------------------
def test_lambda_zero_hands_exact_zeros_to_the_next_layer(hip_lib, oracle):
    """R = 0.1 on this rig: the layer matrices are the identity to 1e-16 off the diagonal (cond = 1.00), and with
    lambda = 0 the right-hand sides of layer 1 are 0 * w_0: its weights are exactly zero in both paths."""
    row = (48, 2, 3, 0.1, 0.0, "linear")
    M, L, F, R, lam, term = row
    rest, deltas, refs = _case(oracle, row)
    shot = Shot(*row)
    for on in (True, False):
        assert shot.build(rest, deltas, on) == [1] * F
        assert shot.batch.last_build_shared_factor() is on
        for f, W in enumerate(shot.weights()):
            Wo = refs[f][1]
            assert np.array_equal(W[M:2 * M], np.zeros((M, 3)))                       # layer-major: rows M .. 2M-1 are layer 1
            assert np.abs(W[:M] - Wo[:M]).max() <= 1e-8 * np.abs(Wo).max()
            assert np.abs(W - Wo).max() <= 1e-8 * np.abs(Wo).max()
    shot.close()


# ---- 3. through the evaluation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [GRID[1], GRID[3]], ids=lambda r: f"M{r[0]}_L{r[1]}_F{r[2]}")
def test_models_built_this_way_evaluate_within_the_bar(hip_lib, oracle, row):
    M, L, F, R, lam, term = row
    N = 4099
    P = synth.head_mesh(20_000)[:: 20_000 // N][:N].copy()
    dist2 = np.linspace(0.0, 1.2, N).astype(np.float32)
    rest, deltas, refs = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    d_P = torch.from_numpy(P).to(DEV()); d_d2 = torch.from_numpy(dist2).to(DEV())
    out = [torch.empty_like(d_P) for _ in range(F)]
    fall = [torch.empty(N, device=DEV()) for _ in range(F)]
    shot.batch.deform_shared_ml_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], d_dist2=d_d2.data_ptr(),
                                    d_falloff=[t.data_ptr() for t in fall], radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    for f in range(F):
        table_ml, Wo, radii = refs[f]
        ref, _ = oracle.deform(table_ml, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P, dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
        r = parity_ratio(out[f].cpu().numpy(), ref, P, 1e-5)
        print(f"shared ml build M={M} L={L} F={F} evaluated, frame {f}: {r:.3f} of the bar")
        assert r <= 1.0, (f, r)
    shot.close()


# ---- 4. delegation, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["second_rest_array", "m1025", "one_context", "below_threshold"])
def test_a_batch_that_misses_a_condition_is_built_as_without_the_switch(hip_lib, case):
    t = threshold()
    if case == "below_threshold" and t <= 2:
        # (no frame count between the "at least two contexts" condition and the threshold: "one_context" is that case)
        assert t == 2
        case = "one_context"
    M, L, F = {"second_rest_array": (64, 3, 4), "m1025": (1025, 1, 2), "one_context": (64, 3, 1), "below_threshold": (64, 3, t - 1)}[case]
    rest = synth.control_points(M, "head")
    deltas = _deltas(rest, F)
    shot = Shot(M, L, F, 0.7, 0.1, "linear")
    got = {}
    for on in (True, False):
        if case != "second_rest_array":
            tts = shot.build(rest, deltas, on)
        else:
            shared = torch.from_numpy(rest).to(DEV()); other = torch.from_numpy((rest * np.float32(1.01)).astype(np.float32)).to(DEV())
            d_del = torch.from_numpy(deltas).to(DEV())
            shot.keep += [shared, other, d_del]
            torch.cuda.synchronize()
            shot.batch.set_shared_factor(on)
            shot.batch.set_points_dev([other.data_ptr() if f == 2 else shared.data_ptr() for f in range(F)],
                                      [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
            shot.batch.build_async()
            tts = [r.terminationtype for r in shot.batch.build_result()]
        assert tts == [1] * F
        assert shot.batch.last_build_shared_factor() is False
        got[on] = shot.weights()
    for f in range(F):
        assert np.array_equal(got[True][f], got[False][f])
    shot.close()


def test_with_the_switch_off_the_batch_equals_single_builds_bitwise(hip_lib, oracle):
    row = GRID[2]
    M, L, F, R, lam, term = row
    rest, deltas, _ = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, False) == [1] * F
    Wb = shot.weights()
    for f in (0, 5, F - 1):
        e = capi.Engine()
        e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [R, L, lam]); e.set_term(TERMS[term])
        e.set_points(rest, deltas[f])
        assert e.build().terminationtype == 1
        assert np.array_equal(e.get_weights()[0], Wb[f])
        e.close()
    shot.close()


# ---- 5. status and repeatability -----------------------------------------------------------------------------------------
def test_coincident_centres_reach_every_frame_and_the_batch_recovers(hip_lib, oracle):
    row = (64, 3, 5, 0.7, 0.1, "linear")
    M, L, F, R, lam, term = row
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
    row = GRID[2]
    M, L, F, R, lam, term = row
    rest, deltas, _ = _case(oracle, row)
    shot = Shot(*row)
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    first = shot.weights()
    reps = shot.batch.build_result()
    assert [r.iterationscount for r in reps] == [M + 4] * F and [r.n for r in reps] == [M + 4] * F
    assert shot.build(rest, deltas, True) == [1] * F and shot.batch.last_build_shared_factor()
    for a, b in zip(first, shot.weights()):
        assert np.array_equal(a, b)
    # no single factorisation to reuse: as on a multilayer context built on its own
    with pytest.raises(capi.FdError) as ei:
        shot.engines[0].set_deltas(deltas[0])
    assert ei.value.code == capi.FD_E_NOT_BUILT
    shot.close()


def test_a_build_behind_wait_consumed_leaves_the_running_evaluation_alone(hip_lib, oracle):
    """Evaluate on one stream, fd_batch_wait_consumed on the build stream, a switch-on build with other deltas there while
    the evaluation runs: its outputs equal an undisturbed run's, and the new models are sound."""
    row = (64, 4, 8, 1.0, 0.1, "linear")
    M, L, F, R, lam, term = row
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
        shot.batch.deform_shared_ml_dev(N, d_P.data_ptr(), [t.data_ptr() for t in out], stream_ptr=sA.cuda_stream)
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
    tt, table_ml, Wo, radii = oracle.build_multilayer(oracle.control_table(rest, rest + other[F - 1]), R, L, lam, TERMS[term])
    assert np.abs(shot.weights()[F - 1] - Wo).max() <= 1e-8 * np.abs(Wo).max()
    shot.close()
