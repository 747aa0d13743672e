"""GPU: fd_deform_vectors* -- the Jacobian A = I + f Pi J of the deformation and the normals / tangents it carries
(include/facedeform_hip.h states the definition).

The yardstick is an independent fp64 restatement of the field and its derivative in numpy, from the weights the
engine solved (Engine.get_weights) and the rest rig.  It is first held to fd_deform's own fp64 displacement, which pins
the weight conventions, so the Jacobian checks test derivatives and not bookkeeping."""
import json
import os

import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

KINDS = {
    "thin_plate": (capi.KERNEL_THIN_PLATE, []),
    "gaussian": (capi.KERNEL_GAUSSIAN, [0.35]),
    "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0]),
    "multilayer": (capi.KERNEL_GAUSSIAN_ML, [0.7, 4, 0.1]),
    "biharmonic": (capi.KERNEL_BIHARMONIC, []),
    "cubic": (capi.KERNEL_CUBIC, []),
}
TERMS = {"linear": capi.TERM_LINEAR, "const": capi.TERM_CONST, "zero": capi.TERM_ZERO}
# the error bars, fixed in advance: fp32 output rounding of A plus the evaluation's own error against S'
BAR_REL = 2.0 ** -22
BAR_ABS = {capi.EVAL_FP64: 1e-12, capi.EVAL_FP32: 2.0 ** -22}
RADIUS2, RATE = 0.36, 1.7
WORST = {}          # (kind, precision) -> worst observed ratio against the bar; written out if FD_VECTORS_REPORT names a file


def teardown_module(module):
    path = os.environ.get("FD_VECTORS_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({f"{k[0]}/{'fp64' if k[1] == capi.EVAL_FP64 else 'fp32'}": v for k, v in sorted(WORST.items())}, f, indent=1)


def _engine(kind, params, term, rest, delta):
    e = capi.Engine(device=0)
    e.set_points(rest, delta)
    e.set_kernel(kind, params)
    e.set_term(term)
    e.build()
    return e


def _model(e, kind, rest):
    """(centres, per-record weights, affine rows {const, x, y, z} x output, radii) in fp64."""
    W, radii = e.get_weights()
    n = W.shape[0] - 4
    centres = np.tile(rest.astype(np.float64), (n // rest.shape[0], 1))     # multilayer: record l * M + c sits on centre c
    return centres, W[:n], W[n:], radii


def _field(kind, X, centres, Wr, aff, radii, chunk=1024):
    """d(x), J(x) = dd/dx and sum_j |w_j| |grad phi_j| in fp64, raw kernel forms of the header's table."""
    n = X.shape[0]
    d = np.empty((n, 3)); J = np.empty((n, 3, 3)); S = np.empty(n)
    wn = np.linalg.norm(Wr, axis=1)
    L = aff[1:4].T                                  # L[c, k] = d d_c / d x_k
    for a in range(0, n, chunk):
        D = X[a:a + chunk, None, :] - centres[None]
        r2 = np.einsum("bjk,bjk->bj", D, D)
        r = np.sqrt(r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            if kind == capi.KERNEL_THIN_PLATE:
                phi = np.where(r > 0, r2 * np.log(r), 0.0); g = np.where(r > 0, 2 * np.log(r) + 1, 0.0)
            elif kind == capi.KERNEL_BIHARMONIC:
                phi = -r; g = np.where(r > 0, -1.0 / r, 0.0)
            elif kind == capi.KERNEL_CUBIC:
                phi = r2 * r; g = 3 * r
            else:
                phi = np.exp(-r2 / radii[None] ** 2); g = -2.0 / radii[None] ** 2 * phi
        d[a:a + chunk] = phi @ Wr + aff[0] + X[a:a + chunk] @ aff[1:4]
        G = g[:, :, None] * D                                              # grad phi_j, (b, M, 3)
        J[a:a + chunk] = np.tensordot(G, Wr, axes=([1], [0])).transpose(0, 2, 1) + L
        S[a:a + chunk] = np.abs(g) * r @ wn
    return d, J, S + np.linalg.norm(L)


def _normalise(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def _projection(tu, tv, nrm):
    """Pi = a1 a1^T + a2 a2^T as project_to_tangents builds a1, a2 (reference src/SOP_FaceDeform.hpp:28-41), fp64."""
    u, v, n = (_normalise(a.astype(np.float64)) for a in (tu, tv, nrm))
    G = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = _normalise(np.einsum("bi,bij->bj", u, G)); a2 = _normalise(np.einsum("bi,bij->bj", v, G))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def _inputs(P, seed=5):
    """Frames on the head ellipsoid (u, v deliberately not unit length), a transported normal N = u x v, and a dist2 that
    gates about a third of the vertices; a few sit exactly on the radius (f = 0, not gated)."""
    n0 = _normalise(P.astype(np.float64) / np.array([0.75, 1.0, 0.85]) ** 2)
    u = 1.3 * _normalise(np.cross(n0, [0.3, 0.2, 1.0]))
    v = 0.8 * np.cross(n0, _normalise(u))
    tu, tv, nrm = (a.astype(np.float32) for a in (u, v, n0))
    Nv = np.cross(tu.astype(np.float64), tv.astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(seed)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    return tu, tv, nrm, Nv, dist2


def _check_A(A, f, Pi, J, S, precision):
    """Worst ratio of ||A_gpu - (I + f Pi J)||_F against the bar, over the vertices given."""
    fJ = f[:, None, None] * (J if Pi is None else Pi @ J)
    Aref = np.eye(3)[None] + fJ
    err = np.linalg.norm(A.astype(np.float64) - Aref, axis=(1, 2))
    bar = BAR_REL * np.linalg.norm(Aref, axis=(1, 2)) + BAR_ABS[precision] * f * S
    return float((err / bar).max()) if err.size else 0.0


def _run_case(e, P, tu, tv, nrm, Nv, dist2, J64, S64, precisions=(capi.EVAL_FP32, capi.EVAL_FP64), sub=None):
    """fd_deform_vectors in both precisions, projection on and off; returns the worst ratio per precision."""
    worst = {}
    live = ~(dist2 > RADIUS2)
    sel = np.arange(P.shape[0]) if sub is None else sub
    lv = sel[live[sel]]
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv])
    for prec in precisions:
        e.set_eval_precision(prec)
        for proj in (False, True):
            frames = (tu, tv, nrm) if proj else None
            out, fall, No, tuo, tvo, A = e.deform_vectors(P, dist2=dist2, tangents=frames, N=Nv, tu=tu, tv=tv,
                                                          want_jacobian=True, radius2=RADIUS2, falloffrate=RATE)
            ref, rfall = e.deform(P, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
            assert np.array_equal(out, ref) and np.array_equal(fall, rfall)          # fd_deform's bits
            # gated vertices: everything passes through, A = I exactly; f = 0: A = I exactly
            g = ~live
            assert np.array_equal(No[g], Nv[g]) and np.array_equal(tuo[g], tu[g]) and np.array_equal(tvo[g], tv[g])
            assert np.array_equal(A[g], np.broadcast_to(np.eye(3, dtype=np.float32), A[g].shape))
            z = live & (fall == 0)
            assert z.any() and np.array_equal(A[z], np.broadcast_to(np.eye(3, dtype=np.float32), A[z].shape))
            f = fall[lv].astype(np.float64)
            idx = np.searchsorted(sel, lv)
            r = _check_A(A[lv], f, Pi_all if proj else None, J64[idx], S64[idx], prec)
            worst[prec] = max(worst.get(prec, 0.0), r)
            # transport against the A it wrote: t' = A t, n' = cof(A) n = (A u) x (A v) for n = u x v, |n'| = |n|
            A64 = A[lv].astype(np.float64)
            for t, to in ((tu, tuo), (tv, tvo)):
                want = np.einsum("bij,bj->bi", A64, t[lv].astype(np.float64))
                assert np.abs(to[lv] - want).max() <= 1e-6 * np.abs(want).max()
            Au = np.einsum("bij,bj->bi", A64, tu[lv].astype(np.float64))
            Av = np.einsum("bij,bj->bi", A64, tv[lv].astype(np.float64))
            assert np.abs(_normalise(No[lv].astype(np.float64)) - _normalise(np.cross(Au, Av))).max() <= 1e-6
            nN = np.linalg.norm(Nv[lv].astype(np.float64), axis=1)
            assert np.abs(np.linalg.norm(No[lv].astype(np.float64), axis=1) - nN).max() <= 1e-6 * nN.max()
    return worst


def _check_parity(e, P, d64, sub=None):
    """numpy's d reproduces fd_deform's fp64 displacement (no gate, no projection) to 2e-7 of max |d|."""
    e.set_eval_precision(capi.EVAL_FP64)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    out, _ = e.deform(P)
    e.set_output(capi.OUTPUT_POSITION)
    got = out if sub is None else out[sub]
    assert np.abs(got - d64).max() <= 2e-7 * np.abs(d64).max()


def _record(kind_name, worst):
    for prec, r in worst.items():
        WORST[(kind_name, prec)] = max(WORST.get((kind_name, prec), 0.0), r)


@pytest.mark.parametrize("M", [32, 96, 256])
@pytest.mark.parametrize("term", sorted(TERMS))
@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_jacobian_against_fp64_restatement(hip_lib, kind_name, term, M):
    kind, params = KINDS[kind_name]
    P = synth.head_mesh(20_000)
    rest = synth.control_points(M, "head")
    e = _engine(kind, params, TERMS[term], rest, synth.smooth_deltas(rest))
    centres, Wr, aff, radii = _model(e, kind, rest)
    d64, J64, S64 = _field(kind, P.astype(np.float64), centres, Wr, aff, radii)
    _check_parity(e, P, d64)
    worst = _run_case(e, P, *_inputs(P), J64, S64)
    _record(kind_name, worst)
    e.close()
    for prec, r in worst.items():
        assert r <= 1.0, (kind_name, term, M, prec, r)


@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_jacobian_million_vertices(hip_lib, kind_name):
    kind, params = KINDS[kind_name]
    P = synth.head_mesh(1_000_000)
    rest = synth.control_points(256, "head")
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.smooth_deltas(rest))
    centres, Wr, aff, radii = _model(e, kind, rest)
    sub = np.arange(0, P.shape[0], 37)                      # every vertex is evaluated; the restatement checks a sample
    d64, J64, S64 = _field(kind, P[sub].astype(np.float64), centres, Wr, aff, radii)
    _check_parity(e, P, d64, sub)
    worst = _run_case(e, P, *_inputs(P), J64, S64, sub=sub)
    _record(kind_name, worst)
    e.close()
    for prec, r in worst.items():
        assert r <= 1.0, (kind_name, prec, r)


def _rotation(angle, axis):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@pytest.mark.parametrize("precision", [capi.EVAL_FP32, capi.EVAL_FP64])
def test_rigid_motion_is_reproduced_exactly(hip_lib, precision):
    """Thin-plate + linear term on a rig moved rigidly: the polynomial reproduces the motion and the RBF weights vanish
    (up to the fp32 rounding of the deltas), so A = R and N_out = R N; a translation gives A = I."""
    rest = synth.control_points(96, "head")
    P = synth.head_mesh(20_000)
    tu, tv, nrm, Nv, _ = _inputs(P)
    R = _rotation(0.1, [0.3, 1.0, -0.2])
    p0 = np.array([0.4, -0.3, 0.25])
    moved = ((rest.astype(np.float64) - p0) @ R.T + p0).astype(np.float32)
    for delta, want in (((moved - rest).astype(np.float32), R),
                        (np.broadcast_to(np.float32([0.05, -0.02, 0.03]), rest.shape).copy(), np.eye(3))):
        e = _engine(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, rest, delta)
        e.set_eval_precision(precision)
        _, _, No, _, _, A = e.deform_vectors(P, N=Nv, want_jacobian=True)
        assert np.abs(A - want[None]).max() <= 1e-5
        assert np.abs(No - Nv.astype(np.float64) @ want.T).max() <= 1e-5
        e.close()


def test_central_differences_agree(hip_lib):
    """A - I against central differences of fd_deform's fp64 displacement, h = 2^-10 (x +- h exact in fp32)."""
    P = synth.head_mesh(20_000)[::10].copy()
    h = np.float32(2.0 ** -10)
    for kind_name in ("thin_plate", "qnn", "cubic"):
        kind, params = KINDS[kind_name]
        rest = synth.control_points(96, "head")
        e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.smooth_deltas(rest))
        e.set_eval_precision(capi.EVAL_FP64)
        _, _, _, _, _, A = e.deform_vectors(P, want_jacobian=True)
        e.set_output(capi.OUTPUT_DISPLACEMENT)
        fd = np.empty((P.shape[0], 3, 3))
        exact = np.ones(P.shape[0], bool)
        for k in range(3):
            Pp, Pm = P.copy(), P.copy()
            Pp[:, k] += h; Pm[:, k] -= h
            exact &= ((Pp[:, k] - P[:, k]) == h) & ((P[:, k] - Pm[:, k]) == h)
            dp, _ = e.deform(Pp); dm, _ = e.deform(Pm)
            fd[:, :, k] = (dp.astype(np.float64) - dm) / (2.0 * float(h))
        # away from the centres, where the third derivative that h^2 multiplies stays bounded
        far = np.min(np.linalg.norm(P[:, None, :] - rest[None], axis=2), axis=1) > 0.05
        use = exact & far
        assert use.sum() > 0.8 * P.shape[0] * far.mean()
        AmI = A.astype(np.float64) - np.eye(3)
        scale = np.linalg.norm(AmI, axis=(1, 2)).max()
        assert np.linalg.norm(AmI[use] - fd[use], axis=(1, 2)).max() <= 1e-3 * scale, kind_name
        e.close()


def test_dev_path_aliasing_and_untouched_tail(hip_lib):
    """fd_deform_vectors_dev gives the host path's bits; N_out = N in place gives the same bits as separate arrays,
    also when N is the projection's nrm array and P is deformed in place; lanes past N write nothing."""
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(20_000)
    tu, tv, nrm, Nv, dist2 = _inputs(P)
    rest = synth.control_points(96, "head")
    for prec in (capi.EVAL_FP32, capi.EVAL_FP64):
        e = _engine(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, rest, synth.smooth_deltas(rest))
        e.set_eval_precision(prec)
        host = e.deform_vectors(P, dist2=dist2, tangents=(tu, tv, nrm), N=Nv, tu=tu, tv=tv, want_jacobian=True,
                                radius2=RADIUS2, falloffrate=RATE)
        n = P.shape[0] - 123                                  # a tail the call does not own
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_P, d_d2, d_tu, d_tv, d_nrm, d_N = (T(a) for a in (P, dist2, tu, tv, nrm, Nv))
        sentinel = -7.25
        d_out = torch.full_like(d_P, sentinel); d_fall = torch.full_like(d_d2, sentinel)
        d_No, d_tuo, d_tvo = (torch.full_like(d_P, sentinel) for _ in range(3))
        d_A = torch.full((P.shape[0], 9), sentinel, device=dev)
        e.deform_vectors_dev(n, d_P.data_ptr(), d_out.data_ptr(), d_d2.data_ptr(), d_fall.data_ptr(), d_tu.data_ptr(),
                             d_tv.data_ptr(), d_nrm.data_ptr(), d_N.data_ptr(), d_No.data_ptr(), d_tu.data_ptr(),
                             d_tuo.data_ptr(), d_tv.data_ptr(), d_tvo.data_ptr(), d_A.data_ptr(), RADIUS2, RATE)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in (d_out, d_fall, d_No, d_tuo, d_tvo, d_A)]
        want = list(host[:5]) + [host[5].reshape(-1, 9)]
        live = ~(dist2 > RADIUS2)
        for k, (g, w) in enumerate(zip(got, want)):
            if k == 1:      # fall-off: gated vertices keep the caller's entry (here the sentinel)
                assert np.array_equal(g[:n][live[:n]], w[:n][live[:n]])
            else:
                assert np.array_equal(g[:n], w[:n]), k
            assert (g[n:] == sentinel).all(), k
        # in place: N_out = N = nrm (the projection reads the same array the result goes to), P deformed in place
        d_P2, d_nrm2 = T(P), T(nrm)
        d_A2 = torch.empty_like(d_A)
        e.deform_vectors_dev(n, d_P2.data_ptr(), d_P2.data_ptr(), d_d2.data_ptr(), 0, d_tu.data_ptr(), d_tv.data_ptr(),
                             d_nrm2.data_ptr(), d_nrm2.data_ptr(), d_nrm2.data_ptr(), 0, 0, 0, 0, d_A2.data_ptr(),
                             RADIUS2, RATE)
        e.deform_vectors_dev(n, d_P.data_ptr(), d_out.data_ptr(), d_d2.data_ptr(), 0, d_tu.data_ptr(), d_tv.data_ptr(),
                             d_nrm.data_ptr(), d_nrm.data_ptr(), d_No.data_ptr(), 0, 0, 0, 0, d_A.data_ptr(), RADIUS2, RATE)
        torch.cuda.synchronize()
        assert torch.equal(d_P2[:n], d_out[:n]) and torch.equal(d_nrm2[:n], d_No[:n]) and torch.equal(d_A2[:n], d_A[:n])
        e.close()


def test_unbuilt_model_passes_vectors_through(hip_lib):
    """The evaluation enqueued right behind a build whose status cannot be known yet, on a rig the first solver fails
    (two centres one fp32 step apart, cubic): the pass-through case -- every vector bit for bit, A = I; the next call
    repairs the model and transports."""
    dev = torch.device("cuda", 0)
    M, N = 300, 20_000
    rest = synth.control_points(M, "head")
    near = rest.copy(); near[17] = near[200] + np.float32(1e-7) * np.array([1, 0.5, -0.3], np.float32)
    P = synth.head_mesh(N)
    _, _, _, Nv, _ = _inputs(P)
    d_P, d_N = (torch.from_numpy(a).to(dev) for a in (P, Nv))
    d_out, d_No = torch.empty_like(d_P), torch.empty_like(d_P)
    d_A = torch.empty((N, 9), device=dev)
    e = capi.Engine(device=0)
    e.set_points(near, synth.smooth_deltas(rest)); e.set_kernel(capi.KERNEL_CUBIC, []); e.set_term(capi.TERM_LINEAR)
    e.build_async()
    e.deform_vectors_dev(N, d_P.data_ptr(), d_out.data_ptr(), d_N=d_N.data_ptr(), d_N_out=d_No.data_ptr(),
                         d_jacobian=d_A.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_P) and torch.equal(d_No, d_N)
    assert torch.equal(d_A, torch.eye(3, device=dev).reshape(1, 9).expand(N, 9))
    e.deform_vectors_dev(N, d_P.data_ptr(), d_out.data_ptr(), d_N=d_N.data_ptr(), d_N_out=d_No.data_ptr(),
                         d_jacobian=d_A.data_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(d_No, d_N) and not torch.equal(d_out, d_P)
    assert e.build_result().terminationtype == 1
    e.close()


def test_vectors_null_is_fd_deform(hip_lib):
    """vec == NULL or all-NULL members: exactly fd_deform (both precisions, both output modes)."""
    P = synth.head_mesh(20_000)
    tu, tv, nrm, _, dist2 = _inputs(P)
    rest = synth.control_points(64, "head")
    e = _engine(capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0], capi.TERM_LINEAR, rest, synth.smooth_deltas(rest))
    import ctypes as C
    for prec in (capi.EVAL_FP32, capi.EVAL_FP64):
        for mode in (capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT):
            e.set_eval_precision(prec); e.set_output(mode)
            ref, rfall = e.deform(P, dist2=dist2, tangents=(tu, tv, nrm), radius2=RADIUS2, falloffrate=RATE)
            for vec in (None, capi.FdVectors(C.sizeof(capi.FdVectors))):
                out = P.copy(); fall = np.zeros(P.shape[0], np.float32)
                rc = hip_lib.fd_deform_vectors(e.ctx, P.shape[0], out.ctypes.data, out.ctypes.data, dist2.ctypes.data,
                                               fall.ctypes.data, tu.ctypes.data, tv.ctypes.data, nrm.ctypes.data,
                                               RADIUS2, RATE, None if vec is None else C.byref(vec))
                assert rc == capi.FD_OK
                assert np.array_equal(out, ref) and np.array_equal(fall, rfall)
            out2, fall2, _, _, _, _ = e.deform_vectors(P, dist2=dist2, tangents=(tu, tv, nrm), want_jacobian=True,
                                                       radius2=RADIUS2, falloffrate=RATE)
            assert np.array_equal(out2, ref) and np.array_equal(fall2, rfall)
    e.close()
