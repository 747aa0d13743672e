"""GPU: fd_invert* -- the rest-space x with x + f Pi d(x) = y, per vertex, by Newton in one fp64 launch
(include/facedeform_hip.h states the contract).

The yardstick is this file's own fp64 numpy restatement of the field, its Jacobian and the Newton iteration, built from the
weights the engine solved (Engine.get_weights) and the rest rig.  It is first held to fd_deform's own fp64 displacement,
which pins the weight conventions.  f is the fall-off fd_deform reports, Y is fd_deform's own fp64 output.

The bars (fixed in advance, no further margin):
  round trip   |F_ref(X_out)|_2 <= tol_i + |A_ref(X_out)|_F * 1/2 |ulp(X_out)|_2   (the stopping rule + what rounding x to fp32
               adds through A);
  same root    |X_out - x_ref|_2 <= |ulp(x_ref)|_2 (both sides rounded to fp32), iters within +-1 of the reference's count."""
import functools

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
# linear for all kinds, const and zero for thin-plate and QNN
KIND_TERMS = [(k, "linear") for k in sorted(KINDS)] + [(k, t) for k in ("thin_plate", "qnn") for t in ("const", "zero")]
RADIUS2, RATE = 0.36, 1.7
M_RIG = 64


# ---- the restatement ---------------------------------------------------------------------------------------------

def _engine(kind, params, term, rest, delta, check=True):
    e = capi.Engine(device=0)
    e.set_points(rest, delta)
    e.set_kernel(kind, params)
    e.set_term(term)
    e.build(check=check)
    return e


def _model(e, rest):
    """(centres, per-record weights, affine rows {const, x, y, z} x output, radii) in fp64."""
    W, radii = e.get_weights()
    n = W.shape[0] - 4
    centres = np.tile(rest.astype(np.float64), (n // rest.shape[0], 1))     # multilayer: record l * M + c sits on centre c
    return centres, W[:n], W[n:], radii


def _field(kind, X, model, chunk=1024):
    """d(x) and J(x) = dd/dx in fp64, raw kernel forms of the header's table."""
    centres, Wr, aff, radii = model
    n = X.shape[0]
    d = np.empty((n, 3)); J = np.empty((n, 3, 3))
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
    return d, J


def _normalise(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(n > 0, v / np.where(n > 0, n, 1), v)


def _projection(tu, tv, nrm):
    """Pi = a1 a1^T + a2 a2^T as project_to_tangents builds a1, a2, fp64."""
    u, v, n = (_normalise(a.astype(np.float64)) for a in (tu, tv, nrm))
    G = u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :] + n[:, :, None] * n[:, None, :]
    a1 = _normalise(np.einsum("bi,bij->bj", u, G)); a2 = _normalise(np.einsum("bi,bij->bj", v, G))
    return a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :]


def _F_A(kind, model, X, Y, f, Pi):
    """F(x) = x + f Pi d(x) - y and A(x) = I + f Pi J(x)."""
    d, J = _field(kind, X, model)
    if Pi is not None:
        d = np.einsum("bij,bj->bi", Pi, d); J = Pi @ J
    return (X - Y) + f[:, None] * d, np.eye(3)[None] + f[:, None, None] * J


def _scale(rest):
    """The model's normalisation scale: the rest rig's extent rounded to a power of two (fd_pack.h)."""
    c = rest.astype(np.float64)
    cen = c.mean(axis=0)
    rad_c = np.sqrt(((c - cen) ** 2).sum(axis=1).max()); rad_o = np.sqrt((c ** 2).sum(axis=1).max())
    rad = rad_c if np.linalg.norm(cen) > rad_c * 0.0625 else rad_o
    return 2.0 ** int(np.rint(np.log2(rad)))


def _tol(Y, s, tol=0.0):
    if tol > 0:
        return np.full(Y.shape[0], float(tol))
    return 2.0 ** -25 * np.maximum(np.abs(Y.astype(np.float64)).max(axis=1), s)


def _newton(kind, model, Y, f, Pi, tol, max_iter=20):
    """The iteration of the contract on every row: x0 = y; while |F| > tol: x <- x - A^-1 F (cofactors, one division).
    Returns (x written, its residual, status): status >= 0 steps taken, -1 max_iter reached, -2 broke down."""
    Y = Y.astype(np.float64)
    n = Y.shape[0]
    x = Y.copy(); best = Y.copy(); bestres = np.full(n, np.inf); res = np.zeros(n)
    status = np.zeros(n, np.int64); active = np.ones(n, bool)
    for k in range(max_iter + 1):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        with np.errstate(all="ignore"):
            F, A = _F_A(kind, model, x[idx], Y[idx], f[idx], None if Pi is None else Pi[idx])
            rn = np.linalg.norm(F, axis=1)
            c = np.empty_like(A)
            for i in range(3):
                for j in range(3):
                    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                    c[:, i, j] = A[:, i1, j1] * A[:, i2, j2] - A[:, i1, j2] * A[:, i2, j1]
            det = (A[:, 0] * c[:, 0]).sum(axis=1)
            xn = x[idx] - np.einsum("bji,bj->bi", c, F) / det[:, None]          # adj = cof^T
        fin = np.isfinite(rn)
        better = fin & (rn < bestres[idx])
        conv = fin & (rn <= tol[idx])
        spent = fin & ~conv & (k == max_iter)
        broke = ~conv & ~spent & (~fin | (det == 0) | ~np.isfinite(xn).all(axis=1))
        step = ~conv & ~spent & ~broke
        best[idx[better]] = x[idx[better]]; bestres[idx[better]] = rn[better]
        res[idx[conv]] = rn[conv]
        status[idx[conv]] = k; status[idx[broke]] = -2; status[idx[spent]] = -1
        x[idx[step]] = xn[step]
        active[idx] = step
    # left at -1 or -2: the best iterate rounded to fp32 is what is written, and the residual is taken there
    failed = np.nonzero(status < 0)[0]
    if failed.size:
        x[failed] = best[failed].astype(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            F, _ = _F_A(kind, model, x[failed], Y[failed], f[failed], None if Pi is None else Pi[failed])
        res[failed] = np.linalg.norm(F, axis=1)
    return x, res, status


def _ulp(X32):
    return np.linalg.norm(np.spacing(np.abs(X32.astype(np.float32))).astype(np.float64), axis=1)


def _bar_ratio(kind, model, X32, Y, f, Pi, tol):
    """Per row: |F_ref(X_out)|_2 over tol_i + |A_ref(X_out)|_F * 1/2 |ulp(X_out)|_2; also |F_ref(X_out)|_2 itself."""
    F, A = _F_A(kind, model, X32.astype(np.float64), Y.astype(np.float64), f, Pi)
    rn = np.linalg.norm(F, axis=1)
    return rn / (tol + np.linalg.norm(A, axis=(1, 2)) * 0.5 * _ulp(X32)), rn


# ---- inputs --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _inputs():
    """3000 head vertices + the first 8 control points (x on a centre) + 200 mesh points scaled by 1.6 (off the surface);
    frames; a dist2 that gates about a third of the vertices, every 97th exactly on the radius (f = 0, not gated)."""
    rest = synth.control_points(M_RIG)
    mesh = synth.head_mesh(3000)
    P = np.concatenate([mesh, rest[:8], (mesh[:200] * np.float32(1.6))]).astype(np.float32)
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(5)
    dist2 = (rng.random(P.shape[0]) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    for a in (rest, P, tu, tv, nrm, dist2):
        a.setflags(write=False)
    return rest, P, tu, tv, nrm, dist2


def _check_parity(e, kind, model, P):
    """numpy's d reproduces fd_deform's fp64 displacement (no gate, no projection) to 2e-7 of max |d|."""
    d64, _ = _field(kind, P.astype(np.float64), model)
    e.set_eval_precision(capi.EVAL_FP64)
    e.set_output(capi.OUTPUT_DISPLACEMENT)
    out, _ = e.deform(P)
    e.set_output(capi.OUTPUT_POSITION)
    assert np.abs(out - d64).max() <= 2e-7 * np.abs(d64).max()


@functools.lru_cache(maxsize=None)
def _case(kind_name, term, mult, proj):
    """One engine, its forward output Y, the call under test and the reference iteration, computed once and left unchanged."""
    kind, params = KINDS[kind_name]
    rest, P, tu, tv, nrm, dist2 = _inputs()
    delta = (synth.rig_deltas(rest, 0) * np.float32(mult)).astype(np.float32)
    e = _engine(kind, params, TERMS[term], rest, delta)
    model = _model(e, rest)
    _check_parity(e, kind, model, P)
    frames = (tu, tv, nrm) if proj else None
    e.set_eval_precision(capi.EVAL_FP64)
    Y, fall = e.deform(P, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    e.set_eval_precision(capi.EVAL_FP32)            # the inverse is fp64 whatever the context says
    X, res, its = e.invert(Y, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    e.close()
    live = ~(dist2 > RADIUS2)
    lv = np.nonzero(live)[0]
    f = fall[lv].astype(np.float64)
    Pi = _projection(tu[lv], tv[lv], nrm[lv]) if proj else None
    tol = _tol(Y[lv], _scale(rest))
    xr, rr, sr = _newton(kind, model, Y[lv], f, Pi, tol)
    return dict(kind=kind, model=model, Y=Y, X=X, res=res, its=its, live=live, lv=lv, f=f, Pi=Pi, tol=tol, xr=xr, rr=rr, sr=sr)


CASES = [(k, t, m, p) for k, t in KIND_TERMS for m in (1, 3) for p in (False, True)]


# ---- 1-3: round trip, same root, pass-through ------------------------------------------------------------------------

@pytest.mark.parametrize("kind_name,term,mult,proj", CASES)
def test_round_trip(hip_lib, kind_name, term, mult, proj):
    c = _case(kind_name, term, mult, proj)
    lv = c["lv"]
    assert (c["its"][lv] >= 0).all()
    ratio, _ = _bar_ratio(c["kind"], c["model"], c["X"][lv], c["Y"][lv], c["f"], c["Pi"], c["tol"])
    print(f"round trip {kind_name}/{term} x{mult} proj={proj}: worst ratio {ratio.max():.3f}, iters {np.bincount(c['its'][lv])}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("kind_name,term,mult,proj", CASES)
def test_same_root_as_the_reference(hip_lib, kind_name, term, mult, proj):
    c = _case(kind_name, term, mult, proj)
    lv = c["lv"]
    assert (c["sr"] >= 0).all()                                   # the restated iteration converges on these inputs
    xr32 = c["xr"].astype(np.float32)
    err = np.linalg.norm(c["X"][lv].astype(np.float64) - xr32, axis=1)
    step = np.abs(c["its"][lv] - c["sr"])
    print(f"same root {kind_name}/{term} x{mult} proj={proj}: worst |dX| / |ulp| {(err / _ulp(xr32)).max():.3f}, "
          f"reference iters {np.bincount(c['sr'])}, worst |d iters| {step.max()}")
    assert (err <= _ulp(xr32)).all()
    assert step.max() <= 1
    # residual_out is the fp64 residual rounded to fp32; rounding is monotone, so <= tol survives it against tol rounded alike
    assert (c["res"][lv] <= c["tol"].astype(np.float32)).all()


@pytest.mark.parametrize("kind_name,term,mult,proj", CASES[:4])
def test_gated_vertices_pass_through(hip_lib, kind_name, term, mult, proj):
    c = _case(kind_name, term, mult, proj)
    g = ~c["live"]
    assert g.any()
    assert np.array_equal(c["X"][g].view(np.uint32), c["Y"][g].view(np.uint32))
    assert (c["its"][g] == 0).all() and (c["res"][g] == 0).all()
    # f = 0 (dist2 exactly on the radius): step 0 converges, F(y) = 0 exactly
    z = np.nonzero(c["f"] == 0)[0]
    assert z.size > 0
    zi = c["lv"][z]
    assert np.array_equal(c["X"][zi].view(np.uint32), c["Y"][zi].view(np.uint32))
    assert (c["its"][zi] == 0).all() and (c["res"][zi] == 0).all()


def test_failed_build_passes_every_vertex_through(hip_lib):
    """Coincident control points: the build ends with -5 and is not repaired.  Enqueued right behind the build, whose status
    cannot be known yet, the launch passes every vertex through; every call returns what fd_deform_dev returns."""
    dev = torch.device("cuda", 0)
    rest, P, _, _, _, _ = _inputs()
    dup = rest.copy(); dup[17] = dup[40]
    e = capi.Engine(device=0)
    e.set_points(dup, synth.rig_deltas(rest, 0)); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR)
    N = P.shape[0]
    d_Y = torch.from_numpy(P.copy()).to(dev)
    d_X = torch.full_like(d_Y, -7.25); d_res = torch.full((N,), -7.25, device=dev)
    d_its = torch.full((N,), -7, dtype=torch.int32, device=dev)
    d_out = torch.empty_like(d_Y)

    def rc_of(call):
        try:
            call()
            return capi.FD_OK
        except capi.FdError as err:
            return err.code

    e.build_async()
    rc_first = rc_of(lambda: e.invert_dev(N, d_Y.data_ptr(), d_X.data_ptr(), d_residual=d_res.data_ptr(), d_iters=d_its.data_ptr()))
    torch.cuda.synchronize()
    if rc_first == capi.FD_OK:            # the usual course: the call came before the host could know the status
        assert torch.equal(d_X, d_Y)
        assert (d_its == 0).all() and (d_res == 0).all()
    # the status is in by now: both calls report the failed build, the device and the host forms alike
    rc_inv = rc_of(lambda: e.invert_dev(N, d_Y.data_ptr(), d_X.data_ptr()))
    rc_def = rc_of(lambda: e.deform_dev(N, d_Y.data_ptr(), d_out.data_ptr()))
    assert rc_inv == rc_def and rc_def in (capi.FD_E_DUPLICATE, capi.FD_E_SINGULAR)
    assert rc_first in (capi.FD_OK, rc_def)
    assert rc_of(lambda: e.invert(P)) == rc_of(lambda: e.deform(P)) == rc_def
    e.close()


# ---- 4: launch shapes ------------------------------------------------------------------------------------------------

def test_launch_shapes_and_determinism(hip_lib):
    """N around the wave and the 512-vertex workgroup tile; a vertex's bits do not depend on N; two calls agree; X_out may
    alias Y (the host call solves in place on the device; the device call is tried both ways)."""
    dev = torch.device("cuda", 0)
    c = _case("thin_plate", "linear", 1, True)
    rest, P, tu, tv, nrm, dist2 = _inputs()
    kind, params = KINDS["thin_plate"]
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    Y = c["Y"]
    full = (c["X"], c["res"], c["its"])
    for N in (1, 63, 64, 65, 511, 512, 513):
        got = e.invert(Y[:N], dist2=dist2[:N], tangents=(tu[:N], tv[:N], nrm[:N]), radius2=RADIUS2, falloffrate=RATE)
        for g, w in zip(got, full):
            assert np.array_equal(g.view(np.uint32), w[:N].view(np.uint32)), N
    again = e.invert(Y, dist2=dist2, tangents=(tu, tv, nrm), radius2=RADIUS2, falloffrate=RATE)
    for g, w in zip(again, full):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # device pointers: separate output, then in place; a tail the call does not own stays untouched
    N = 513
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_Y, d_d2, d_tu, d_tv, d_nrm = (T(a) for a in (Y, dist2, tu, tv, nrm))
    d_X = torch.full_like(d_Y, -7.25)
    d_res = torch.full((Y.shape[0],), -7.25, device=dev); d_its = torch.full((Y.shape[0],), -7, dtype=torch.int32, device=dev)
    e.invert_dev(N, d_Y.data_ptr(), d_X.data_ptr(), d_d2.data_ptr(), d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr(),
                 RADIUS2, RATE, d_residual=d_res.data_ptr(), d_iters=d_its.data_ptr())
    d_Y2 = d_Y.clone()
    e.invert_dev(N, d_Y2.data_ptr(), d_Y2.data_ptr(), d_d2.data_ptr(), d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr(),
                 RADIUS2, RATE)
    torch.cuda.synchronize()
    assert np.array_equal(d_X[:N].cpu().numpy().view(np.uint32), full[0][:N].view(np.uint32))
    assert np.array_equal(d_res[:N].cpu().numpy(), full[1][:N]) and np.array_equal(d_its[:N].cpu().numpy(), full[2][:N])
    assert torch.equal(d_Y2[:N], d_X[:N]) and torch.equal(d_Y2[N:], d_Y[N:])
    assert (d_X[N:] == -7.25).all() and (d_res[N:] == -7.25).all() and (d_its[N:] == -7).all()
    e.close()


def test_mixed_wave_leaves_iterating_lanes_alone(hip_lib):
    """A wave in which lane 0 is gated, lane 1 has f = 0 and the rest iterate: the iterating lanes' bits are those of the
    all-live run."""
    rest, P, _, _, _, _ = _inputs()
    kind, params = KINDS["qnn"]
    e = _engine(kind, params, capi.TERM_LINEAR, rest, (synth.rig_deltas(rest, 0) * np.float32(3)).astype(np.float32))
    e.set_eval_precision(capi.EVAL_FP64)
    n = 64
    d2_live = np.full(n, np.float32(0.1))
    Y, _ = e.deform(P[:n], dist2=d2_live, radius2=RADIUS2, falloffrate=RATE)
    all_live = e.invert(Y, dist2=d2_live, radius2=RADIUS2, falloffrate=RATE)
    assert (all_live[2] >= 1).all()                               # every lane iterates
    d2_mixed = d2_live.copy(); d2_mixed[0] = np.float32(2 * RADIUS2); d2_mixed[1] = np.float32(RADIUS2)
    mixed = e.invert(Y, dist2=d2_mixed, radius2=RADIUS2, falloffrate=RATE)
    for g, w in zip(mixed, all_live):
        assert np.array_equal(g[2:].view(np.uint32), w[2:].view(np.uint32))
    assert np.array_equal(mixed[0][:2].view(np.uint32), Y[:2].view(np.uint32))
    assert (mixed[2][:2] == 0).all() and (mixed[1][:2] == 0).all()
    e.close()


@pytest.mark.parametrize("M", [33, 49])
@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_padded_record_counts(hip_lib, kind_name, M):
    """M = 33 and 49: the records are padded to a multiple of 16 (Mpad > M); the round trip and the reference's root."""
    kind, params = KINDS[kind_name]
    _, P, tu, tv, nrm, dist2 = _inputs()
    rest = synth.control_points(M)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, synth.rig_deltas(rest, 0))
    model = _model(e, rest)
    _check_parity(e, kind, model, P)
    e.set_eval_precision(capi.EVAL_FP64)
    Y, fall = e.deform(P, dist2=dist2, tangents=(tu, tv, nrm), radius2=RADIUS2, falloffrate=RATE)
    X, res, its = e.invert(Y, dist2=dist2, tangents=(tu, tv, nrm), radius2=RADIUS2, falloffrate=RATE)
    e.close()
    lv = np.nonzero(~(dist2 > RADIUS2))[0]
    f = fall[lv].astype(np.float64); Pi = _projection(tu[lv], tv[lv], nrm[lv]); tol = _tol(Y[lv], _scale(rest))
    assert (its[lv] >= 0).all()
    ratio, _ = _bar_ratio(kind, model, X[lv], Y[lv], f, Pi, tol)
    xr, _, sr = _newton(kind, model, Y[lv], f, Pi, tol)
    xr32 = xr.astype(np.float32)
    err = np.linalg.norm(X[lv].astype(np.float64) - xr32, axis=1)
    print(f"M={M} {kind_name}: worst ratio {ratio.max():.3f}, worst |dX| / |ulp| {(err / _ulp(xr32)).max():.3f}")
    assert ratio.max() <= 1.0
    assert (err <= _ulp(xr32)).all() and np.abs(its[lv] - sr).max() <= 1


# ---- 5: a map that folds must end, and say so -------------------------------------------------------------------------

FOLD_CASES = [(k, p) for k in sorted(KINDS) for p in (False, True)]


@functools.lru_cache(maxsize=None)
def _fold_case(kind_name, proj):
    """noise deltas x 3, max_iter = 30: the call (it raises unless it returns FD_OK) and the reference iteration, once."""
    kind, params = KINDS[kind_name]
    rest, P, tu, tv, nrm, dist2 = _inputs()
    delta = (synth.noise_deltas(M_RIG) * np.float32(3)).astype(np.float32)
    e = _engine(kind, params, capi.TERM_LINEAR, rest, delta)
    model = _model(e, rest)
    _check_parity(e, kind, model, P)
    frames = (tu, tv, nrm) if proj else None
    e.set_eval_precision(capi.EVAL_FP64)
    Y, fall = e.deform(P, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE)
    X, res, its = e.invert(Y, dist2=dist2, tangents=frames, radius2=RADIUS2, falloffrate=RATE, max_iter=30)
    e.close()
    lv = np.nonzero(~(dist2 > RADIUS2))[0]
    f = fall[lv].astype(np.float64); Pi = _projection(tu[lv], tv[lv], nrm[lv]) if proj else None
    tol = _tol(Y[lv], _scale(rest))
    _, A0 = _F_A(kind, model, P[lv].astype(np.float64), Y[lv].astype(np.float64), f, Pi)
    ratio, rn = _bar_ratio(kind, model, X[lv], Y[lv], f, Pi, tol)
    _, _, sr = _newton(kind, model, Y[lv], f, Pi, tol, max_iter=30)
    return dict(X=X, res=res[lv], its=its[lv], det0=np.linalg.det(A0), ratio=ratio, rn=rn, sr=sr)


@pytest.mark.parametrize("kind_name,proj", FOLD_CASES)
def test_folded_map_ends_and_says_so(hip_lib, kind_name, proj):
    """noise deltas x 3: the forward map folds (min det A < 0 over the vertices).  An ordinary bounded loop on finite data:
    the call returns FD_OK, every X_out is finite, every vertex that reports convergence meets the round-trip bar, every
    other one reports -1 or -2, and none of those converges in the reference within 28 steps."""
    c = _fold_case(kind_name, proj)
    assert c["det0"].min() < 0                                  # the premise: the map folds on these inputs
    assert np.isfinite(c["X"]).all()
    ok = c["its"] >= 0
    bad = ~ok
    print(f"fold {kind_name} proj={proj}: {ok.sum()} converged (worst ratio {c['ratio'][ok].max():.3f}, most steps {c['its'].max()}), "
          f"{bad.sum()} not (iters {sorted(set(c['its'][bad].tolist()))}); reference: {(c['sr'] >= 0).sum()} converged")
    assert c["ratio"][ok].max() <= 1.0
    assert np.isin(c["its"][bad], (-1, -2)).all()
    wrongly = bad & (c["sr"] >= 0) & (c["sr"] <= 28)
    assert not wrongly.any()


@pytest.mark.parametrize("kind_name,proj", FOLD_CASES)
def test_folded_map_reports_the_residual_of_what_was_written(hip_lib, kind_name, proj):
    """Every vertex the call leaves at -1 or -2: residual_out against the restated residual at X_out, to 1e-6 relative (the
    call takes that residual at the fp32 value it writes, not at the unrounded iterate)."""
    c = _fold_case(kind_name, proj)
    bad = c["its"] < 0
    if not bad.any():
        return
    rel = np.abs(c["res"][bad].astype(np.float64) - c["rn"][bad]) / c["rn"][bad]
    print(f"fold residual {kind_name} proj={proj}: {bad.sum()} unconverged; residual_out against the restatement at X_out: "
          f"worst relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-6


# ---- 6: opts ---------------------------------------------------------------------------------------------------------

def test_opts(hip_lib):
    c = _case("thin_plate", "linear", 3, False)
    rest, P, tu, tv, nrm, dist2 = _inputs()
    kind, params = KINDS["thin_plate"]
    e = _engine(kind, params, capi.TERM_LINEAR, rest, (synth.rig_deltas(rest, 0) * np.float32(3)).astype(np.float32))
    Y, lv, f, model = c["Y"], c["lv"], c["f"], c["model"]
    kw = dict(dist2=dist2, radius2=RADIUS2, falloffrate=RATE)
    # max_iter = 1: vertices are left at -1 with the best iterate written
    X1, res1, its1 = e.invert(Y, max_iter=1, **kw)
    xr, rr, sr = _newton(kind, model, Y[lv], f, None, c["tol"], max_iter=1)
    assert (its1[lv] == -1).any() and np.array_equal(its1[lv], sr)
    xr32 = xr.astype(np.float32)
    assert (np.linalg.norm(X1[lv].astype(np.float64) - xr32, axis=1) <= _ulp(xr32)).all()
    short = its1[lv] == -1
    _, rn1 = _bar_ratio(kind, model, X1[lv], Y[lv], f, None, c["tol"])
    assert (np.abs(res1[lv][short] - rn1[short]) <= 1e-6 * rn1[short]).all()      # the residual of what was written, as in (5)
    # an explicit tol = 1e-4 stops earlier and still meets the round-trip bar with that tol
    Xt, rest_, itst = e.invert(Y, tol=1e-4, **kw)
    assert (itst[lv] >= 0).all() and (itst[lv] <= c["its"][lv]).all() and itst[lv].sum() < c["its"][lv].sum()
    ratio, _ = _bar_ratio(kind, model, Xt[lv], Y[lv], f, None, _tol(Y[lv], 1.0, 1e-4))
    assert ratio.max() <= 1.0
    assert (rest_[lv] <= np.float32(1e-4)).all()
    # NULL residual_out / iters_out change no bit of X_out
    for wr, wi in ((False, True), (True, False), (False, False)):
        Xn, rn_, in_ = e.invert(Y, want_residual=wr, want_iters=wi, **kw)
        assert np.array_equal(Xn.view(np.uint32), c["X"].view(np.uint32))
        assert (rn_ is None) == (not wr) and (in_ is None) == (not wi)
    e.close()
