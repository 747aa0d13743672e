"""CPU: the two references of tests/test_gpu_morph_paths.py against each other on every one of its cases -- the oracle's
column-by-column Householder QR (oracle/fd_oracle.c: fdo_morph_qr, the reference's src/dbse.cpp:9-37) and LAPACK's dgeqrf
(morph_cases.lapack_raw), the oracle's weights and a numpy product on LAPACK's factors.

The bars are a tenth of the device's (test_gpu_morph.py): packed QR <= 1e-12 max|QR|, tau <= 1e-13, weights
<= 1e-11 max(1, |w|).  Measured with these generators: QR <= 2.8e-14 up to N = 5462 and <= 1.7e-13 at the two 411/513-workgroup
cases, tau <= 5.3e-14 (the 2048-shape case; <= 2.8e-14 elsewhere), weights <= 1.2e-13.  The test keeps the references inside
their bars when somebody changes a generator.

Duplicated blendshapes: the reflector of a dependent column is made of rounding noise, so the two references differ entry by
entry (1e-2); what both must hold is the backward error ||Q R - A||_F / ||A||_F.  A Householder QR's is a modest multiple of
the unit roundoff growing no faster than the column count (Higham, Accuracy and Stability of Numerical Algorithms, 19.4);
the bar is S * 2^-52, measured <= 1.3e-15."""
import numpy as np
import pytest

import morph_cases as mc


def _pair(oracle, case):
    rest, shapes = mc.make(case)
    A = oracle.morph_shapes_matrix(rest, shapes)
    assert np.array_equal(A, mc.shapes_matrix(rest, shapes)), "the matrix itself: fp32 deltas, exactly"
    QR, tau = oracle.morph_qr(A)
    QL, tl = mc.lapack_raw(A)
    assert np.isfinite(QR).all() and np.isfinite(tau).all() and np.isfinite(QL).all() and np.isfinite(tl).all()
    return rest, shapes, A, QR, tau, QL, tl


@pytest.mark.parametrize("case", mc.ENTRYWISE + [mc.TOP], ids=mc.ids(mc.ENTRYWISE + [mc.TOP]))
def test_oracle_and_lapack_agree(oracle, case):
    rest, shapes, A, QR, tau, QL, tl = _pair(oracle, case)
    scale = np.abs(QL).max()
    e_qr, e_tau = np.abs(QR - QL).max() / scale, np.abs(tau - tl).max()
    P = mc.frames(case, rest, shapes)[0]
    w, wl = oracle.morph_weights(QR, P, rest), mc.weights_numpy(QL, P, rest)
    e_w = np.abs(w - wl).max() / max(1.0, np.abs(wl).max())
    print(f"{case.name}: QR {e_qr:.2e} (1e-12), tau {e_tau:.2e} (1e-13), weights {e_w:.2e} (1e-11)")
    assert e_qr <= 1e-12
    assert e_tau <= 1e-13
    assert e_w <= 1e-11
    for z in case.zeros:
        for q, t in ((QR, tau), (QL, tl)):
            assert t[z] == 0.0 and np.all(q[:, z] == 0.0), z
        assert w[z] == 0.0 and wl[z] == 0.0
    if case.lone:                                             # nothing below the diagonal: the identity, R_00 the entry itself
        for q, t in ((QR, tau), (QL, tl)):
            assert t[0] == 0.0 and q[0, 0] == A[0, 0] and np.all(q[1:, 0] == 0.0)


@pytest.mark.parametrize("case", mc.DUPLICATE, ids=mc.ids(mc.DUPLICATE))
def test_duplicated_blendshapes_reconstruct(oracle, case):
    rest, shapes, A, QR, tau, QL, tl = _pair(oracle, case)
    assert np.array_equal(A[:, case.dup[0]], A[:, case.dup[1]])
    r_o, r_l = mc.residual(QR, tau, A), mc.residual(QL, tl, A)
    bar = case.S * 2.0 ** -52
    print(f"{case.name}: ||QR - A|| / ||A|| oracle {r_o:.2e}, LAPACK {r_l:.2e} (bar {bar:.2e}); entry by entry they differ by "
          f"{np.abs(QR - QL).max() / np.abs(QL).max():.1e}")
    assert r_o <= bar and r_l <= bar
    # up to the duplicate the two are the same factorisation
    d = case.dup[0]
    assert np.abs(QR[:, :d] - QL[:, :d]).max() <= 1e-12 * np.abs(QL).max() and np.abs(tau[:d] - tl[:d]).max() <= 1e-13


def test_reconstruct_is_a_reference_of_its_own(oracle):
    """reconstruct against numpy's own Q R (mode='reduced' forms Q with dorgqr), on a matrix with a zero column."""
    case = mc.ZERO[1]
    rest, shapes = mc.make(case)
    A = mc.shapes_matrix(rest, shapes)
    QL, tl = mc.lapack_raw(A)
    Q, R = np.linalg.qr(A, mode="reduced")
    assert np.abs(mc.reconstruct(QL, tl) - Q @ R).max() <= 1e-14 * np.abs(A).max()
    bad = tl.copy()
    bad[3] *= 1.0 + 1e-9                                       # and it sees a tau that is off in the ninth digit
    assert mc.residual(QL, bad, A) > 1e3 * mc.residual(QL, tl, A)
