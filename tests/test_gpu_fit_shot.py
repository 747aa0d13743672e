"""GPU: fd_fit_deltas_shot -- fd_fit_deltas for the F targets of a shot over one mesh, omega and mu: one Gram launch, one
factorisation, the right-hand sides through fd_deform_adjoint_shot (include/facedeform_hip.h states the contract).

Recipe, restated normal system (NN, b_f) and bars are tests/test_gpu_fit.py's: the system is the same and the yardstick is the
same, and the right-hand side's error enters exactly as in the single fit.  F = 3 targets -- three other poses of the rig
plus noise -- with a delta0 per frame, 33 control points.

The bars:
  optimality   per frame |NN delta_f - b_f|_2 <= KAPPA2[kind] 2^-53 (|NN|_2 |delta_f|_2 + |b_f|_2), that file's KAPPA2.
  energy       per frame E(delta_f) <= E(lstsq_f) (1 + 1e-10); the reported E0 and E_fit within 1e-10 of the restated ones.
  independence frame 1's deltas from F = 1 and from F = 3 are bit-equal.
  planted      three planted poses: after fd_set_deltas(fp32(delta_f)) + build, fd_deform in fp64 lies within
               conftest.l2_parity_ulp <= 1 of frame f's targets."""
import functools

import numpy as np
import pytest

import test_gpu_fit as tf
from conftest import l2_parity_ulp
from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

RADIUS2, RATE = tf.RADIUS2, tf.RATE
M_FIT, F_FIT = 33, 3
CASES = [(k, p) for k in sorted(tf.KINDS) for p in (False, True)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(kind_name, proj):
    kind, params = tf.KINDS[kind_name]
    P, tu, tv, nrm, dist2, omega = tf._inputs()
    M = M_FIT
    rest = synth.control_points(M)
    rng = np.random.default_rng(300 + len(kind_name))
    e = tf._engine(kind, params, rest, synth.rig_deltas(rest, 0))
    T = []
    for _ in range(F_FIT):
        pose = tf._engine(kind, params, rest, (0.05 * rng.standard_normal(rest.shape)).astype(np.float32))
        T.append((pose.deform(P)[0] + 0.01 * rng.standard_normal(P.shape)).astype(np.float32))
        pose.close()
    T = np.stack(T)
    delta0 = (0.01 * rng.standard_normal((F_FIT,) + rest.shape)).astype(np.float32)
    mu = 1e-8 * float(omega.astype(np.float64).sum())
    frames = (tu, tv, nrm) if proj else None
    kw = dict(omega=omega, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE, mu=mu)
    W_before = e.get_weights()[0]
    S = e.solve_operator()
    fit, reps = e.fit_deltas_shot(P, T, S=S, delta0=delta0, **kw)
    fit_own_S, _ = e.fit_deltas_shot(P, T, S=None, delta0=delta0, **kw)
    alone, reps_alone = e.fit_deltas_shot(P, T[1:2], S=S, delta0=delta0[1:2], **kw)
    single, _ = e.fit_deltas(P, T[1], S=S, delta0=delta0[1], **kw)
    W_after = e.get_weights()[0]
    ekind = capi.KERNEL_THIN_PLATE if kind == capi.KERNEL_THIN_PLATE else capi.KERNEL_GAUSSIAN
    systems = [tf._system(e, ekind, rest, S, P, T[f], omega, dist2, frames, mu, delta0[f]) for f in range(F_FIT)]
    # a following fd_set_deltas + build, against a twin that never ran the fit
    twin = tf._engine(kind, params, rest, synth.rig_deltas(rest, 0))
    nxt = (0.03 * rng.standard_normal(rest.shape)).astype(np.float32)
    W_next = []
    for eng in (e, twin):
        if kind != capi.KERNEL_GAUSSIAN_ML:
            eng.set_deltas(nxt)
        else:                                       # the multilayer model keeps no factorisation for fd_set_deltas
            eng.set_points(rest, nxt)
        eng.build()
        W_next.append(eng.get_weights()[0])
        eng.close()
    return dict(fit=fit, fit_own_S=fit_own_S, alone=alone, single=single, reps=reps, reps_alone=reps_alone, W_before=W_before,
                W_after=W_after, W_next=W_next, systems=systems, mu=mu, delta0=delta0, M=M)


@pytest.mark.parametrize("kind_name,proj", CASES)
def test_optimality_and_energy_per_frame(hip_lib, kind_name, proj):
    c = _case(kind_name, proj)
    M = c["M"]
    assert c["fit"].shape == (F_FIT, M, 3) and np.isfinite(c["fit"]).all()
    for f in range(F_FIT):
        A, w, t, NN, b = c["systems"][f]
        fit, rep, d0 = c["fit"][f], c["reps"][f], c["delta0"][f]
        assert rep.order == (3 * M if proj else M)
        assert 0 < rep.pivot_min <= rep.pivot_max
        res = np.linalg.norm(NN @ fit.ravel() - b)
        bar1 = 2.0 ** -53 * (np.linalg.norm(NN, 2) * np.linalg.norm(fit) + np.linalg.norm(b))
        res1 = np.linalg.norm(NN @ c["single"].ravel() - b) / bar1 if f == 1 else float("nan")
        print(f"fit shot {kind_name} proj={proj} frame {f}: |NN d - b| / (2^-53 (|NN| |d| + |b|)) = {res / bar1:.2f}"
              f"  (fd_fit_deltas on frame 1: {res1:.2f})")
        lstsq = np.linalg.solve(NN, b).reshape(M, 3)
        E_fit, E_ls = (tf._energy(A, w, t, c["mu"], d0, d) for d in (fit, lstsq))
        E0 = tf._energy(A, w, t, c["mu"], d0, d0.astype(np.float64))
        print(f"   E0 = {E0:.9e} (reported {rep.E0:.9e}), E(fit) = {E_fit:.12e} (reported {rep.E_fit:.12e}), "
              f"E(fit) / E(numpy) - 1 = {E_fit / E_ls - 1:.2e}")
        assert res <= tf.KAPPA2[kind_name] * bar1
        assert 0 < E_fit <= E_ls * (1 + 1e-10) and E_fit < E0
        assert abs(rep.E_fit - E_fit) <= 1e-10 * E_fit
        assert abs(rep.E0 - E0) <= 1e-10 * E0
    # order, pivots and stage times are the call's own: the same in every entry
    for rep in c["reps"][1:]:
        for name in ("order", "pivot_min", "pivot_max", "ms_gram", "ms_adjoint", "ms_compose", "ms_solve"):
            assert getattr(rep, name) == getattr(c["reps"][0], name)


@pytest.mark.parametrize("kind_name,proj", CASES)
def test_frame_independence_operator_and_state(hip_lib, kind_name, proj):
    c = _case(kind_name, proj)
    assert np.array_equal(_bits(c["alone"][0]), _bits(c["fit"][1]))                       # F = 1 and F = 3: the same bits
    assert c["reps_alone"][0].E0 == c["reps"][1].E0 and c["reps_alone"][0].E_fit == c["reps"][1].E_fit
    assert np.array_equal(_bits(c["fit"]), _bits(c["fit_own_S"]))                         # S given and S = NULL: the same bits
    assert np.array_equal(_bits(c["W_before"]), _bits(c["W_after"]))                      # the context's model is as it was
    assert np.array_equal(_bits(c["W_next"][0]), _bits(c["W_next"][1]))                   # and so is what fd_set_deltas builds on


@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_planted(hip_lib, kind_name):
    """Targets from fd_deform (fp64, positions) of rigs built on three planted fp32 deltas; no gate, no f = 0, no projection,
    delta0 = 0, mu = 0.  Each frame's fitted deltas, rounded to fp32 and built, reproduce that frame's targets."""
    kind, params = tf.KINDS[kind_name]
    P = tf._inputs()[0]
    M = 64
    rest = synth.control_points(M)
    rng = np.random.default_rng(77)
    planted = (0.05 * rng.standard_normal((F_FIT,) + rest.shape)).astype(np.float32)
    T = []
    for f in range(F_FIT):
        pose = tf._engine(kind, params, rest, planted[f])
        pose.set_eval_precision(capi.EVAL_FP64)
        T.append(pose.deform(P)[0])
        pose.close()
    T = np.stack(T)
    e = tf._engine(kind, params, rest, np.zeros_like(rest))
    fit, reps = e.fit_deltas_shot(P, T)
    for f in range(F_FIT):
        e.set_deltas(fit[f].astype(np.float32))
        e.build()
        e.set_eval_precision(capi.EVAL_FP64)
        out = e.deform(P)[0]
        ratio = l2_parity_ulp(out, T[f], P)
        print(f"planted {kind_name} frame {f}: l2_parity_ulp = {ratio:.3f}; max |fit - planted| = {np.abs(fit[f] - planted[f]).max():.3e}; "
              f"E0 = {reps[f].E0:.6e}, E_fit = {reps[f].E_fit:.6e}")
        assert ratio <= 1.0
    e.close()


def test_singular_without_mu(hip_lib):
    """mu = 0 and every vertex gated: the normal matrix is zero, FD_E_SINGULAR, and nothing is written to delta_out; the same
    case with mu > 0 succeeds and returns every frame's delta0."""
    P = tf._inputs()[0][:500]
    M = 33
    rest = synth.control_points(M)
    e = tf._engine(capi.KERNEL_THIN_PLATE, [], rest, synth.rig_deltas(rest, 0))
    dist2 = np.full(P.shape[0], 2 * RADIUS2, np.float32)
    T = np.stack([(P + np.float32(0.01 * (f + 1))).astype(np.float32) for f in range(F_FIT)])
    delta0 = (0.01 * np.random.default_rng(2).standard_normal((F_FIT,) + rest.shape)).astype(np.float32)
    ptr = capi._np_ptr
    out = np.full((F_FIT, M, 3), -7.25, np.float64)
    reps = (capi.FdFitReport * F_FIT)()
    for r in reps:
        r.struct_size = capi.C.sizeof(capi.FdFitReport)
    rc = e.L.fd_fit_deltas_shot(e.ctx, P.shape[0], F_FIT, ptr(P), ptr(T), None, ptr(dist2), None, None, None, RADIUS2, RATE, 0.0,
                                ptr(delta0), None, ptr(out), reps)
    assert rc == capi.FD_E_SINGULAR
    assert (out == -7.25).all()
    assert all(r.order == M and r.E_fit == r.E0 for r in reps)
    fit, reps = e.fit_deltas_shot(P, T, dist2=dist2, radius2=RADIUS2, falloffrate=RATE, mu=1e-3, delta0=delta0)
    assert np.allclose(fit, delta0.astype(np.float64), rtol=1e-14, atol=0)
    assert all(r.pivot_min == r.pivot_max == 1e-3 for r in reps)
    e.close()


def test_limits_and_frame_count_answer_before_device_work(hip_lib):
    """C + 4 > 1028 is FD_E_INVALID on a context without a model, where FD_E_NOT_BUILT would be the answer had the limit not
    come first; F = 0 likewise."""
    arr = np.zeros((2, 1, 3), np.float32)
    out = np.zeros((2, 1100, 3), np.float64)
    ptr = capi._np_ptr
    e = capi.Engine(device=0)
    rest = synth.control_points(300)
    e.set_points(rest, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1]); e.set_term(capi.TERM_LINEAR)
    call = lambda F: e.L.fd_fit_deltas_shot(e.ctx, 1, F, ptr(arr), ptr(arr), None, None, None, None, None, 1.0, 1.0, 0.0, None, None,
                                            ptr(out), None)
    assert call(2) == capi.FD_E_INVALID
    e.set_kernel(capi.KERNEL_GAUSSIAN_ML, [0.7, 2, 0.1])
    assert call(0) == capi.FD_E_INVALID
    assert call(2) == capi.FD_E_NOT_BUILT
    e.close()
