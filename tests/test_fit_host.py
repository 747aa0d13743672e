"""CPU: the dense host algebra of the delta fits (facedeform_amd/csrc/fd_fit_host.h) on its own, under the address and
undefined-behaviour sanitizers.  tests/tools/fit_host_check.cpp includes that header alone and runs it on raw float64 arrays
that the tests write; the references are NumPy in longdouble.  The GPU tests of the fits (test_gpu_fit.py, test_gpu_fit_shot.py)
reach the same functions through the library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facedeform_amd", "csrc")
LD = np.longdouble
QMAP = ((0, 1, 2), (1, 3, 4), (2, 4, 5))          # the component of H and G that couples axis b with axis c


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("fit_host") / "fit_host_check")
    # the sanitizers' runtimes are linked statically: the shared ASan runtime refuses to start in an environment that preloads
    # any other library, since it must come first
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "fit_host_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(prog, tmp_path, mode, a, b, arrays):
    """The program's output for `mode a b` on the arrays, as one float64 vector; the sanitizers must have had nothing to say."""
    src, dst = str(tmp_path / "in.f64"), str(tmp_path / "out.f64")
    np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in arrays] + [np.zeros(0)]).tofile(src)
    r = subprocess.run([prog, mode, str(a), str(b), src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return np.fromfile(dst, np.float64)


def spd(rng, n, lam):
    """Q diag(lam) Q^T for a random orthogonal Q, symmetric to the bit"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


def solve_ld(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting in longdouble (np.linalg has no longdouble)"""
    A, B = A.astype(LD), B.astype(LD)
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, p]], B[[j, p]] = A[[p, j]], B[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:] -= f[:, None] * A[j]
        B[j + 1:] -= f[:, None] * B[j]
    for j in range(n - 1, -1, -1):
        B[j] = (B[j] - A[j, j + 1:] @ B[j + 1:]) / A[j, j]
    return B


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 7, 48])
def test_cholesky_solves_to_the_conditioning(prog, tmp_path, n, nrhs):
    """A = Q diag(lam) Q^T with lam log-spaced on [1, 100]; the right-hand sides interleaved as the fit lays them out.  Bound:
    n eps kappa = 48 * 2.2e-16 * 100 is about 1e-12 (5e-13 with the unit roundoff); 1e-10 leaves two orders for its constant."""
    rng = np.random.default_rng(100 * n + nrhs)
    A = spd(rng, n, np.logspace(0, 2, n))
    B = rng.standard_normal((n, nrhs))
    out = run(prog, tmp_path, "chol", n, nrhs, [A, B])
    ok, pmin, pmax, X = out[0], out[1], out[2], out[3:].reshape(n, nrhs)
    ref = solve_ld(A, B)
    err = float(np.abs(X - ref).max() / np.abs(ref).max())
    print("n=%d nrhs=%d relative error %.3e pivots [%.3e, %.3e]" % (n, nrhs, err, pmin, pmax))
    assert ok == 1.0
    assert 0.0 < pmin <= pmax
    assert err <= 1e-10


def test_cholesky_accepts_order_zero_without_touching_memory(prog, tmp_path):
    """the program hands null pointers to both functions for n = 0: a read or write would stop it under the sanitizers"""
    out = run(prog, tmp_path, "chol", 0, 3, [])
    assert out.size == 3 and out[0] == 1.0


@pytest.mark.parametrize("n", [2, 7, 48])
def test_cholesky_refuses_an_indefinite_matrix(prog, tmp_path, n):
    rng = np.random.default_rng(n)
    lam = np.logspace(0, 2, n)
    lam[n // 2] = -1.0
    out = run(prog, tmp_path, "chol", n, 1, [spd(rng, n, lam), np.ones(n)])
    assert out[0] == 0.0
    assert out[1] <= 0.0


@pytest.mark.parametrize("proj", [0, 1])
@pytest.mark.parametrize("M", [1, 4])
def test_normal_system_and_energy(prog, tmp_path, M, proj):
    """G = S^T H_q S, A = G in block form + mu I, b = S^T c + mu delta0, and the energy as the quadratic form
    d^T G d - 2 d^T S^T c + tt + mu |d - delta0|^2.  Sums of at most a few hundred products: 1e-12 of the sum of the absolute
    terms."""
    rng = np.random.default_rng(10 * M + proj)
    n, nq, order = M + 4, 6 if proj else 1, 3 * M if proj else M
    mu, tt = 0.37, 5.25
    S = rng.standard_normal((n, M))
    H = rng.standard_normal((nq, n, n))
    H = H + H.transpose(0, 2, 1)
    c = rng.standard_normal((n, 3))
    delta0 = rng.standard_normal((M, 3)).astype(np.float32)
    d = rng.standard_normal((M, 3))
    out = run(prog, tmp_path, "sys", M, proj, [[mu, tt], S, H, c, delta0, d])
    sizes = [nq * M * M, order * order, M * 3, M * 3, 1, 1]
    G, A, b, Stc, E_d, E_0 = np.split(out, np.cumsum(sizes)[:-1])
    assert out.size == sum(sizes)
    G, A, b, Stc = G.reshape(nq, M, M), A.reshape(order, order), b.reshape(M, 3), Stc.reshape(M, 3)

    Sl, Hl, cl, dl, d0l = (x.astype(LD) for x in (S, H, c, d, delta0))
    G_ref = np.stack([Sl.T @ Hl[q] @ Sl for q in range(nq)])
    G_abs = np.stack([np.abs(Sl).T @ np.abs(Hl[q]) @ np.abs(Sl) for q in range(nq)])
    assert (np.abs(G - G_ref) <= 1e-12 * G_abs).all()
    Stc_ref, Stc_abs = Sl.T @ cl, np.abs(Sl).T @ np.abs(cl)
    assert (np.abs(Stc - Stc_ref) <= 1e-12 * Stc_abs).all()
    assert (np.abs(b - (Stc_ref + LD(mu) * d0l)) <= 1e-12 * (Stc_abs + mu * np.abs(d0l))).all()

    def block(Gq):          # unknown 3 i + b with projection frames, else M unknowns with three right-hand sides
        if not proj:
            return Gq[0]
        return np.array([[Gq[QMAP[bb][cc]][i, k] for k in range(M) for cc in range(3)] for i in range(M) for bb in range(3)])
    assert (A == block(G) + mu * np.eye(order)).all()           # placed, and mu added to the diagonal alone: exact

    def energy(x):
        Gb, Ga = block(G_ref), block(G_abs)
        if proj:
            x1 = x.reshape(-1)
            quad, quad_abs = x1 @ Gb @ x1, np.abs(x1) @ Ga @ np.abs(x1)
        else:
            quad = sum(x[:, a] @ Gb @ x[:, a] for a in range(3))
            quad_abs = sum(np.abs(x[:, a]) @ Ga @ np.abs(x[:, a]) for a in range(3))
        lin, lin_abs = 2 * (x * Stc_ref).sum(), 2 * (np.abs(x) * Stc_abs).sum()
        reg = LD(mu) * ((x - d0l) ** 2).sum()
        return quad - lin + LD(tt) + reg, quad_abs + lin_abs + tt + reg
    for got, x in ((E_d[0], dl), (E_0[0], d0l)):
        ref, scale = energy(x)
        print("M=%d proj=%d energy %.17g reference %.17g" % (M, proj, got, float(ref)))
        assert abs(got - ref) <= 1e-12 * scale


@pytest.mark.parametrize("with_omega", [0, 1])
@pytest.mark.parametrize("N", [1, 3, 1000])
def test_cotangent(prog, tmp_path, N, with_omega):
    """g = omega (T - P) in fp32, bit for bit; sum_v omega_v |T_v - P_v|^2 to 1e-12.  Some omega are 0."""
    rng = np.random.default_rng(N + with_omega)
    P = rng.standard_normal((N, 3)).astype(np.float32)
    T = (P + 0.1 * rng.standard_normal((N, 3))).astype(np.float32)
    omega = rng.random(N).astype(np.float32)
    omega[::3] = 0.0
    out = run(prog, tmp_path, "cot", N, with_omega, [P, T, omega])
    tt, g = out[0], out[1:].astype(np.float32).reshape(N, 3)
    w = omega if with_omega else np.ones(N, np.float32)
    diff = T - P
    assert (g.view(np.uint32) == (w[:, None] * diff).view(np.uint32)).all()
    ref = (w.astype(LD) * (diff.astype(LD) ** 2).sum(axis=1)).sum()
    assert abs(tt - ref) <= 1e-12 * ref
