"""GPU: the morph-space factorisation and the per-cook passes (csrc/fd_morph.hip) against the oracle on every path the host
code can take -- the column-by-column factorisation (S > 256), the blocked one at its largest LDS request and at exact
multiples of a workgroup's rows, workgroup counts around the shapes of its reductions, zero / lone / duplicated columns in
every position of a panel, FD_MORPH_MAX_SHAPES blendshapes, one handle re-initialised through every capacity-guarded buffer,
and fd_morph_init's refusals.  tests/morph_cases.py has the cases and says which path each is there for;
tests/test_oracle_morph_paths.py holds the two references to each other on the CPU.

Bars, the existing ones of test_gpu_morph.py: packed QR <= 1e-11 max|QR_ref|, tau <= 1e-12, weights <= 1e-10 max(1, |w|);
displacement np.array_equal with oracle.morph_displace given the device's own weights.  Every case prints its ratios."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import morph_cases as mc
from facedeform_amd import capi

pytestmark = pytest.mark.gpu
CLAMP = (-0.05, 0.08)


def _qr_bars(case, QR, tau, QR_ref, tau_ref, what="oracle"):
    scale = np.abs(QR_ref).max()
    e_qr, e_tau = float(np.abs(QR - QR_ref).max() / scale), float(np.abs(tau - tau_ref).max())
    print(f"{case.name} vs {what}: QR {e_qr:.2e} (1e-11), tau {e_tau:.2e} (1e-12)")
    assert np.isfinite(QR).all() and np.isfinite(tau).all()
    assert e_qr <= 1e-11
    assert e_tau <= 1e-12


def _w_bar(case, w, w_ref, what):
    e = float(np.abs(w - w_ref).max() / max(1.0, np.abs(w_ref).max()))
    print(f"{case.name} weights vs {what}: {e:.2e} (1e-10)")
    assert np.isfinite(w).all()
    assert e <= 1e-10


def _cook(oracle, case, m, r, w_refs):
    """One-frame weights against every (what, w_ref); then the displacement, bit for bit, given the device's weights."""
    w = None
    for clamp, add_delta, fr in ((None, False, 0.0), (CLAMP, True, 0.25)):
        out, w = m.apply(r["P"], clamp, add_delta, fr)
        assert np.array_equal(out, oracle.morph_displace(r["A"], w, r["P"], r["rest"], clamp, add_delta, fr)), (clamp, add_delta)
    for what, w_ref in w_refs:
        _w_bar(case, w, w_ref, what)
    return w


@pytest.mark.parametrize("case", mc.ENTRYWISE, ids=mc.ids(mc.ENTRYWISE))
def test_against_the_oracle(hip_lib, oracle, case):
    r = mc.reference(oracle, case)
    m = capi.Morph()
    m.init(r["rest"], r["shapes"])
    QR, tau = m.qr()
    _qr_bars(case, QR, tau, r["QR"], r["tau"])
    for z in case.zeros:
        assert tau[z] == 0.0 and np.all(QR[:, z] == 0.0), z
    if case.lone:
        assert tau[0] == 0.0 and QR[0, 0] == r["A"][0, 0] and np.all(QR[1:, 0] == 0.0)
    w = _cook(oracle, case, m, r, [("the oracle", r["w"])])
    for z in case.zeros:
        assert w[z] == 0.0, z
    m.close()


@pytest.mark.parametrize("case", mc.MANY, ids=mc.ids(mc.MANY))
def test_many_workgroups_weights_two_ways(hip_lib, oracle, case):
    """Hundreds of row partitions: the weights against the oracle on ITS factors and on the factors downloaded from the
    device -- the second separates a reduction that drops or repeats partitions from a difference of the factorisations."""
    r = mc.reference(oracle, case)
    F = 3
    frames = mc.frames(case, r["rest"], r["shapes"], F)
    m = capi.Morph()
    m.init(r["rest"], r["shapes"])
    QR, tau = m.qr()
    _qr_bars(case, QR, tau, r["QR"], r["tau"])
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(P).to(dev) for P in frames]
    torch.cuda.synchronize()
    m.compute_weights_batch_dev([t.data_ptr() for t in d_frames])
    wb = m.weights_batch()
    for f in range(F):
        w_o, w_d = oracle.morph_weights(r["QR"], frames[f], r["rest"]), oracle.morph_weights(QR, frames[f], r["rest"])
        m.compute_weights_dev(d_frames[f].data_ptr())
        w1 = m.weights()
        for got, name in ((w1, "one-frame"), (wb[f], "batched")):
            _w_bar(case, got, w_o, f"the oracle on its QR, frame {f}, {name}")
            _w_bar(case, got, w_d, f"the oracle on the device's QR, frame {f}, {name}")
    m.close()


@pytest.mark.parametrize("case", mc.DUPLICATE, ids=mc.ids(mc.DUPLICATE))
def test_duplicated_blendshapes(hip_lib, oracle, case):
    """The reflector of a dependent column is rounding noise: no entrywise bar, but everything finite and a backward error
    ||Q R - A||_F / ||A||_F within 10x the larger of the two references' own (the device sums in trees, the oracle in
    sequence: a small constant between them is expected, two orders of magnitude would be a wrong update)."""
    r = mc.reference(oracle, case)
    m = capi.Morph()
    m.init(r["rest"], r["shapes"])
    QR, tau = m.qr()
    assert np.isfinite(QR).all() and np.isfinite(tau).all()
    QL, tl = mc.lapack_raw(r["A"])
    r_dev, r_o, r_l = mc.residual(QR, tau, r["A"]), mc.residual(r["QR"], r["tau"], r["A"]), mc.residual(QL, tl, r["A"])
    print(f"{case.name}: ||QR - A|| / ||A|| device {r_dev:.2e}, oracle {r_o:.2e}, LAPACK {r_l:.2e}")
    assert r_dev <= 10.0 * max(r_o, r_l)
    # up to the duplicate it is the oracle's factorisation, to the entrywise bars
    d = case.dup[0]
    assert np.abs(QR[:, :d] - r["QR"][:, :d]).max() <= 1e-11 * np.abs(r["QR"]).max() and np.abs(tau[:d] - r["tau"][:d]).max() <= 1e-12
    # the weights belong to the factors they are summed over: the oracle's sum over the device's QR
    _cook(oracle, case, m, r, [("the oracle on the device's QR", oracle.morph_weights(QR, r["P"], r["rest"]))])
    m.close()


def test_shape_count_limit(hip_lib, oracle):
    """FD_MORPH_MAX_SHAPES blendshapes: k_morph_weights asks for the whole 64 KB of LDS.  Reference: LAPACK (the oracle takes
    seconds here; the two agree to 8.5e-15 / 5.3e-14 on this case, tests/test_oracle_morph_paths.py)."""
    case = mc.TOP
    assert case.S == mc.MAX_SHAPES and 3 * case.N > case.S
    r = mc.reference(oracle, case)
    m = capi.Morph()
    t0 = time.perf_counter()
    m.init(r["rest"], r["shapes"])
    print(f"{case.name}: init {time.perf_counter() - t0:.2f} s on the host clock, {m.last_init_ms:.0f} ms on the device")
    QR, tau = m.qr()
    _qr_bars(case, QR, tau, r["QR"], r["tau"], "LAPACK")
    _cook(oracle, case, m, r, [("the oracle on LAPACK's QR", r["w"]), ("the oracle on the device's QR", oracle.morph_weights(QR, r["P"], r["rest"]))])
    m.close()


def test_reinitialising_one_handle(hip_lib):
    """(700, 9) -> (86, 257) -> (5, 8) -> (700, 256) -> (175001, 9) -> (700, 9) on one handle: every buffer behind cap_S,
    cap_entries, cap_bpartial and cap_partial grows, is reused larger than needed, and changes between the two
    factorisations.  The device code is deterministic, so each result is a fresh handle's bit for bit."""
    m = capi.Morph()
    for case in mc.REINIT:
        rest, shapes = mc.make(case)
        m.init(rest, shapes)
        QR, tau = m.qr()
        fresh = capi.Morph()
        fresh.init(rest, shapes)
        QR2, tau2 = fresh.qr()
        fresh.close()
        assert QR.shape == (3 * case.N, case.S)
        assert np.array_equal(QR, QR2) and np.array_equal(tau, tau2), case.name
    m.close()


def test_init_refusals_leave_the_factorisation(hip_lib):
    """S above FD_MORPH_MAX_SHAPES, S > 3N, N = 0 and a NULL shape: FD_E_INVALID with the message, before any device work --
    a handle that held a factorisation still returns it unchanged."""
    L = hip_lib
    case = mc.ZERO[1]
    rest, shapes = mc.make(case)
    m = capi.Morph()
    m.init(rest, shapes)
    QR, tau = m.qr()
    big = np.ascontiguousarray(np.zeros((700, 3), np.float32))

    def refused(N, S, table, text):
        rc = L.fd_morph_init(m.h, N, S, C.c_void_p(big.ctypes.data), table)
        msg = L.fd_morph_last_error(m.h).decode()
        assert rc == capi.FD_E_INVALID, (rc, msg)
        assert text in msg, msg
        assert m.initialised and L.fd_morph_shape_count(m.h) == case.S
        QR2, tau2 = m.qr()
        assert np.array_equal(QR, QR2) and np.array_equal(tau, tau2)

    def table(S, null_at=None):
        return (C.c_void_p * S)(*[None if s == null_at else big.ctypes.data for s in range(S)])

    over = mc.MAX_SHAPES + 1
    refused(700, over, table(over), f"at most {mc.MAX_SHAPES} (FD_MORPH_MAX_SHAPES)")
    refused(2, 7, table(7), "more blendshapes (7) than rows (6)")
    refused(0, 3, table(3), "need N > 0")
    refused(700, 5, table(5, null_at=3), "shape 3 is NULL")
    m.init(rest, shapes)                                      # and the handle goes on working
    QR3, _ = m.qr()
    assert np.array_equal(QR, QR3)
    m.close()
