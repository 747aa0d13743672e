"""GPU: fd_batch_deform_vectors_shared_dev -- the Jacobian and the vectors it carries for every frame of a shared-rig
batch in one launch (k_vectors32_shared_<kind>), DESIGN.md 4.7b.

The yardstick is test_gpu_vectors.py's independent fp64 restatement of each frame's field and derivative, from the
weights the frame's context solved.  The bar is fixed in advance: per vertex and frame
    ||A_gpu - A_ref||_F <= 2^-22 ||A_ref||_F + 2^-21 f S'
(twice the one-frame fp32 absolute term: the split's dropped lo x lo product and the fp32 accumulation over M)."""
import json
import os

import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_vectors import _field, _inputs, _model, _normalise, _projection, _rotation, KINDS, TERMS, RADIUS2, RATE

pytestmark = pytest.mark.gpu

BAR_REL = 2.0 ** -22
BAR_ABS = 2.0 ** -21
SHARED_KINDS = {k: KINDS[k] for k in ("thin_plate", "gaussian", "qnn")}
WORST = {}          # kind -> worst ratio against the bar; written out if FD_VECTORS_SHARED_REPORT names a file
SENTINEL = np.float32(-7.25)


def teardown_module(module):
    path = os.environ.get("FD_VECTORS_SHARED_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)


def _batch(kind, params, term, M, F, rest, deltas=None, precision=None):
    dev = torch.device("cuda", 0)
    if deltas is None:
        deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    d_rest = torch.from_numpy(rest).to(dev)
    d_del = torch.from_numpy(np.ascontiguousarray(deltas)).to(dev)
    engines = []
    for _ in range(F):
        e = capi.Engine()
        e.set_kernel(kind, list(params)); e.set_term(term)
        if precision is not None:
            e.set_eval_precision(precision)
        engines.append(e)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    return engines, batch, (d_rest, d_del)


def _close(engines, batch):
    batch.close()
    for e in engines:
        e.close()


class Outs:
    """Device outputs of one vectors call (N + 64 entries, the tail a sentinel: entries past N are not touched)."""
    def __init__(self, N, F, jac=True):
        dev = torch.device("cuda", 0)
        full = lambda w: torch.full((N + 64, w), float(SENTINEL), device=dev)
        self.N = N
        self.P = [full(3) for _ in range(F)]
        self.fall = [torch.zeros(N + 64, device=dev) for _ in range(F)]
        self.No = [full(3) for _ in range(F)]
        self.tuo = [full(3) for _ in range(F)]
        self.tvo = [full(3) for _ in range(F)]
        self.A = [full(9) for _ in range(F)] if jac else None
        torch.cuda.synchronize()        # the fills run on torch's stream, the library on the contexts': order them

    def call(self, batch, d, proj, dist2=True, stream_ptr=None):
        ptr = lambda ts: None if ts is None else [t.data_ptr() for t in ts]
        batch.deform_vectors_shared_dev(self.N, d["P"].data_ptr(), ptr(self.P), d_dist2=d["d2"].data_ptr() if dist2 else 0,
                                        d_falloff=ptr(self.fall), d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if proj else None,
                                        d_N=d["Nv"].data_ptr(), d_N_out=ptr(self.No), d_vtu=d["tu"].data_ptr(), d_vtu_out=ptr(self.tuo),
                                        d_vtv=d["tv"].data_ptr(), d_vtv_out=ptr(self.tvo), d_jacobian=ptr(self.A),
                                        radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream_ptr)

    def host(self, f):
        n = self.N
        got = [t[f].cpu().numpy() for t in (self.P, self.No, self.tuo, self.tvo)] + [self.fall[f].cpu().numpy()]
        A = self.A[f].cpu().numpy() if self.A is not None else None
        for t in got[:4] + ([A] if A is not None else []):
            assert (t[n:] == SENTINEL).all()                  # entries past N untouched
        P, No, tuo, tvo, fall = got
        return P[:n], fall[:n], No[:n], tuo[:n], tvo[:n], None if A is None else A[:n].reshape(n, 3, 3)


def _device_inputs(P):
    dev = torch.device("cuda", 0)
    tu, tv, nrm, Nv, dist2 = _inputs(P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (tu, tv, nrm, Nv, dist2), {"P": t(P), "tu": t(tu), "tv": t(tv), "nrm": t(nrm), "Nv": t(Nv), "d2": t(dist2)}


def _check_frame(A, No, tuo, tvo, fall, live, Pi, J, S, tu, tv, Nv):
    """Worst ratio against the bar for A and, carried through, for t' = A t and n' = cof(A) n rescaled to |n|."""
    f = fall.astype(np.float64)
    Aref = np.eye(3)[None] + f[:, None, None] * (J if Pi is None else Pi @ J)
    bar = BAR_REL * np.linalg.norm(Aref, axis=(1, 2)) + BAR_ABS * f * S
    ratio = float((np.linalg.norm(A.astype(np.float64) - Aref, axis=(1, 2)) / bar).max())
    for t, to in ((tu, tuo), (tv, tvo)):
        t64 = t.astype(np.float64)
        want = np.einsum("bij,bj->bi", Aref, t64)
        tb = bar * np.linalg.norm(t64, axis=1) + 2.0 ** -23 * np.linalg.norm(want, axis=1)
        ratio = max(ratio, float((np.linalg.norm(to - want, axis=1) / tb).max()))
    n64 = Nv.astype(np.float64)
    cof = np.stack([np.cross(Aref[:, :, 1], Aref[:, :, 2]), np.cross(Aref[:, :, 2], Aref[:, :, 0]),
                    np.cross(Aref[:, :, 0], Aref[:, :, 1])], axis=2)           # columns: cof(A) = [a1 x a2, a2 x a0, a0 x a1]
    m = np.einsum("bij,bj->bi", cof, n64)
    nn = np.linalg.norm(n64, axis=1)
    want = _normalise(m) * nn[:, None]
    nb = 4.0 * np.linalg.norm(Aref, axis=(1, 2)) * bar * nn ** 2 / np.linalg.norm(m, axis=1) + 2.0 ** -22 * nn
    ratio = max(ratio, float((np.linalg.norm(No - want, axis=1) / nb).max()))
    return ratio


def _run(kind, params, term, M, F, N=3_000, projs=(False, True), sub=None, scale=1.0):
    P = synth.head_mesh(max(N, 20_000))[:: max(N, 20_000) // N][:N].copy() * np.float32(scale)
    rest = synth.control_points(M, "head")
    engines, batch, keep = _batch(kind, params, term, M, F, rest)
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    live = ~(dist2 > RADIUS2)
    sel = np.arange(N) if sub is None else sub
    lv = sel[live[sel]]
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv])
    refs = []
    for f in range(F):
        centres, Wr, aff, radii = _model(engines[f], kind, rest)
        _, J, S = _field(kind, P[lv].astype(np.float64), centres, Wr, aff, radii)
        refs.append((J, S))
    worst = 0.0
    for proj in projs:
        outs = Outs(N, F)
        outs.call(batch, d, proj)
        # the position launch's own bits, same run
        Pref = [torch.empty_like(d["P"]) for _ in range(F)]
        fref = [torch.zeros(N, device=d["P"].device) for _ in range(F)]
        torch.cuda.synchronize()
        batch.deform_shared_dev(N, d["P"].data_ptr(), [t.data_ptr() for t in Pref], d_dist2=d["d2"].data_ptr(),
                                d_falloff=[t.data_ptr() for t in fref],
                                d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if proj else None,
                                radius2=RADIUS2, falloffrate=RATE)
        torch.cuda.synchronize()
        for f in range(F):
            Pg, fall, No, tuo, tvo, A = outs.host(f)
            assert np.array_equal(Pg, Pref[f].cpu().numpy()) and np.array_equal(fall, fref[f].cpu().numpy()), f
            g = ~live
            assert np.array_equal(No[g], Nv[g]) and np.array_equal(tuo[g], tu[g]) and np.array_equal(tvo[g], tv[g])
            assert np.array_equal(A[g], np.broadcast_to(np.eye(3, dtype=np.float32), A[g].shape))
            z = live & (fall == 0)
            assert z.any() and np.array_equal(A[z], np.broadcast_to(np.eye(3, dtype=np.float32), A[z].shape))
            assert np.array_equal(No[z], Nv[z]) and np.array_equal(tuo[z], tu[z]) and np.array_equal(tvo[z], tv[z])
            J, S = refs[f]
            r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], live[lv], Pi_all if proj else None, J, S, tu[lv], tv[lv], Nv[lv])
            worst = max(worst, r)
    _close(engines, batch)
    return worst


@pytest.mark.parametrize("F", [1, 3, 13, 17, 20, 32])
@pytest.mark.parametrize("M", [32, 96, 256])
@pytest.mark.parametrize("term", sorted(TERMS))
@pytest.mark.parametrize("kind_name", sorted(SHARED_KINDS))
def test_jacobian_of_every_frame_against_fp64_restatement(hip_lib, kind_name, term, M, F):
    kind, params = SHARED_KINDS[kind_name]
    assert capi.fd_shared_vectors_kernel_name(M, F, kind).startswith("k_vectors32_shared_")
    r = _run(kind, params, TERMS[term], M, F)
    WORST[kind_name] = max(WORST.get(kind_name, 0.0), r)
    assert r <= 1.0, (kind_name, term, M, F, r)


# (M, F) -> the position launch, hence the pack layout the vector launch reads, and whether it stages the model in chunks:
#   384 / 20: k_deform32_shared_w1 (32-row tiles per lane half), resident;  384 / 32: k_deform32_tps_shared_wide (rows 3 f + c),
#   resident (12 K blocks, 12 fit);  512 / 20: w1, staged in chunks;  512 / 32: tps_shared_wide, staged in chunks.
LARGE = {(384, 20): "k_deform32_shared_w1", (384, 32): "k_deform32_tps_shared_wide",
         (512, 20): "k_deform32_shared_w1", (512, 32): "k_deform32_tps_shared_wide"}


@pytest.mark.parametrize("M,F", sorted(LARGE))
@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_every_pack_layout_and_chunked_staging(hip_lib, kind_name, M, F):
    kind, params = SHARED_KINDS[kind_name]
    assert capi.load().fd_shared_kernel_name(M, F, kind).decode() == LARGE[(M, F)]
    r = _run(kind, params, capi.TERM_LINEAR, M, F, N=2_000)
    WORST[kind_name] = max(WORST.get(kind_name, 0.0), r)
    assert r <= 1.0, (kind_name, M, F, r)


def test_thin_plate_far_from_the_rig(hip_lib):
    """Vertices 21-32 rig radii from the centres (the head scaled by 30): the thin-plate basis grows like |x - c| log |x - c|;
    its pre-scale keeps the fp16 pieces finite there, and the bar holds."""
    r = _run(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, 96, 13, N=2_000, projs=(False,), scale=30.0)
    WORST["thin_plate"] = max(WORST.get("thin_plate", 0.0), r)
    assert r <= 1.0, r


@pytest.mark.parametrize("F", [3, 20])
def test_an_unbuilt_frame_passes_its_vectors_through(hip_lib, F):
    """A frame built on other rest points than frame 0 (the rest array rewritten between two builds, as in
    test_gpu_shared.py) is passed through by the pack kernel's frame record: its vectors come out bit for bit with
    A = I at every vertex, P_out = P_in, and the other frames still meet the bar."""
    M, N = 96, 4_000
    kind = capi.KERNEL_THIN_PLATE
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(100_000)[::16][:N].copy()
    rest = synth.control_points(M, "head")
    other = (rest * np.float32(1.01)).astype(np.float32)
    deltas = np.stack([synth.smooth_deltas(rest, f % 8) for f in range(F)]).astype(np.float32)
    d_rest = torch.from_numpy(rest).to(dev)
    d_del = torch.from_numpy(deltas).to(dev)
    engines = []
    for _ in range(F):
        e = capi.Engine(); e.set_kernel(kind); e.set_term(capi.TERM_LINEAR); engines.append(e)
    head, lone, batch = capi.Batch(engines[:-1]), capi.Batch([engines[-1]]), capi.Batch(engines)
    head.set_points_dev([d_rest.data_ptr()] * (F - 1), [d_del[k].data_ptr() for k in range(F - 1)], M)
    head.build_async(); assert [r.terminationtype for r in head.build_result()] == [1] * (F - 1)
    d_rest.copy_(torch.from_numpy(other).to(dev))            # the same array, another rig
    torch.cuda.synchronize()
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(); assert lone.build_result()[0].terminationtype == 1
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, proj=True)                          # same address everywhere: accepted by the host
    torch.cuda.synchronize()
    Pg, _, No, tuo, tvo, A = outs.host(F - 1)
    assert np.array_equal(Pg, P)
    assert np.array_equal(No, Nv) and np.array_equal(tuo, tu) and np.array_equal(tvo, tv)
    assert np.array_equal(A, np.broadcast_to(np.eye(3, dtype=np.float32), A.shape))
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    Pi = _projection(tu[lv], tv[lv], nrm[lv])
    for f in (0, F - 2):
        centres, Wr, aff, radii = _model(engines[f], kind, rest)
        _, J, S = _field(kind, P[lv].astype(np.float64), centres, Wr, aff, radii)
        _, fall, No, tuo, tvo, A = outs.host(f)
        assert not np.array_equal(A[lv], np.broadcast_to(np.eye(3, dtype=np.float32), A[lv].shape))
        r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], live[lv], Pi, J, S, tu[lv], tv[lv], Nv[lv])
        assert r <= 1.0, (f, r)
    # the next call on the batch reports the mismatch (fd_batch_deform_shared_dev's rule)
    with pytest.raises(capi.FdError) as ei:
        outs.call(batch, d, proj=True)
    assert ei.value.code == capi.FD_E_INVALID
    for b in (head, lone, batch):
        b.close()
    for e in engines:
        e.close()


@pytest.mark.parametrize("kind_name", ["thin_plate", "qnn"])
def test_full_size(hip_lib, kind_name):
    kind, params = SHARED_KINDS[kind_name]
    N = 1_000_000
    r = _run(kind, params, capi.TERM_LINEAR, 256, 32, N=N, projs=(True,), sub=np.arange(0, N, 997))
    WORST[kind_name] = max(WORST.get(kind_name, 0.0), r)
    assert r <= 1.0, (kind_name, r)


@pytest.mark.parametrize("case", ["biharmonic", "cubic", "multilayer", "fp64", "few_centres"])
def test_fallback_is_the_one_frame_launch_bit_for_bit(hip_lib, case):
    M, F, N = (16 if case == "few_centres" else 96), 3, 5_000
    kind, params = KINDS["thin_plate" if case in ("fp64", "few_centres") else case]
    precision = capi.EVAL_FP64 if case == "fp64" else None
    P = synth.head_mesh(20_000)[::4][:N].copy()
    rest = synth.control_points(M, "head")
    engines, batch, keep = _batch(kind, params, capi.TERM_LINEAR, M, F, rest, precision=precision)
    # (the name query sees no context: an fp64 batch falls back whatever it says -- include/facedeform_hip.h)
    assert capi.fd_shared_vectors_kernel_name(M, F, kind) == "" or case == "fp64"
    _, d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, proj=True)
    # the positions as fd_batch_deform_shared_dev writes them with the same arguments
    Pref = [torch.empty_like(d["P"]) for _ in range(F)]
    fref = [torch.zeros(N, device=d["P"].device) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_dev(N, d["P"].data_ptr(), [t.data_ptr() for t in Pref], d_dist2=d["d2"].data_ptr(),
                            d_falloff=[t.data_ptr() for t in fref], d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()),
                            radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    for f in range(F):
        Pg, fall = outs.host(f)[:2]
        assert np.array_equal(Pg, Pref[f].cpu().numpy()) and np.array_equal(fall, fref[f].cpu().numpy()), (case, f)
        ref = Outs(N, 1)
        engines[f].deform_vectors_dev(N, d["P"].data_ptr(), ref.P[0].data_ptr(), d["d2"].data_ptr(), ref.fall[0].data_ptr(),
                                      d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr(), d["Nv"].data_ptr(), ref.No[0].data_ptr(),
                                      d["tu"].data_ptr(), ref.tuo[0].data_ptr(), d["tv"].data_ptr(), ref.tvo[0].data_ptr(), ref.A[0].data_ptr(),
                                      radius2=RADIUS2, falloffrate=RATE)
        torch.cuda.synchronize()
        for a, b in zip(outs.host(f), ref.host(0)):
            assert np.array_equal(a, b), (case, f)
    _close(engines, batch)


def test_rigid_motion_gives_the_rotation(hip_lib):
    """Thin-plate + linear term, every frame a rigidly moved rig: the polynomial reproduces the motion, A = R_f and
    N_out = R_f N for every frame."""
    M, F, N = 96, 4, 20_000
    rest = synth.control_points(M, "head")
    P = synth.head_mesh(N)
    p0 = np.array([0.4, -0.3, 0.25])
    Rs = [_rotation(0.05 + 0.04 * f, [0.3, 1.0 - 0.2 * f, -0.2]) for f in range(F)]
    deltas = np.stack([((rest.astype(np.float64) - p0) @ R.T + p0 - rest).astype(np.float32) for R in Rs])
    engines, batch, keep = _batch(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest, deltas=deltas)
    (tu, tv, nrm, Nv, _), d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, proj=False, dist2=False)
    torch.cuda.synchronize()
    for f in range(F):
        _, _, No, _, _, A = outs.host(f)
        assert np.abs(A - Rs[f][None]).max() <= 1e-5, f
        assert np.abs(No - Nv.astype(np.float64) @ Rs[f].T).max() <= 1e-5, f
    _close(engines, batch)


@pytest.mark.parametrize("F", [16, 32])
def test_contexts_may_be_rebuilt_once_the_launch_has_its_copy(hip_lib, F):
    """fd_batch_wait_consumed covers the vector launch: a lane that waits for it and then builds the NEXT group's models on
    the same contexts leaves the vectors in flight untouched -- each group's Jacobians match that group's models."""
    N, M = 200_000, 256
    kind = capi.KERNEL_THIN_PLATE
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    d_rest = torch.from_numpy(rest).to(dev)
    groups = [np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8) + 0.5 * g) for f in range(F)]) for g in range(2)]
    d_del = [torch.from_numpy(x).to(dev) for x in groups]
    lane, es = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    engines = []
    for _ in range(F):
        e = capi.Engine(); e.set_stream(lane.cuda_stream); e.set_kernel(kind); e.set_term(capi.TERM_LINEAR)
        engines.append(e)
    batch = capi.Batch(engines)
    outs = [Outs(N, F) for _ in range(2)]
    torch.cuda.synchronize()
    built = torch.cuda.Event()
    weights = []
    for g in range(2):
        batch.wait_consumed(lane.cuda_stream)
        batch.set_points_dev([d_rest.data_ptr()] * F, [d_del[g].data_ptr() + f * M * 12 for f in range(F)], M)
        batch.build_async(lane.cuda_stream)
        built.record(lane)
        es.wait_event(built)
        outs[g].call(batch, d, proj=True, stream_ptr=es.cuda_stream)
        if g == 0:
            lane.synchronize()
            weights.append([_model(engines[f], kind, rest) for f in (0, F - 1)])
    torch.cuda.synchronize()
    weights.append([_model(engines[f], kind, rest) for f in (0, F - 1)])
    live = ~(dist2 > RADIUS2)
    sel = np.arange(0, N, 401)
    lv = sel[live[sel]]
    Pi = _projection(tu[lv], tv[lv], nrm[lv])
    for g in range(2):
        for q, f in enumerate((0, F - 1)):
            centres, Wr, aff, radii = weights[g][q]
            _, J, S = _field(kind, P[lv].astype(np.float64), centres, Wr, aff, radii)
            _, fall, No, tuo, tvo, A = outs[g].host(f)
            r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], live[lv], Pi, J, S, tu[lv], tv[lv], Nv[lv])
            assert r <= 1.0, (g, f, r)
    batch.close()
    for e in engines:
        e.set_stream(None); e.close()


def test_prepared_set_then_vectors(hip_lib):
    """fd_batch_prepare_shared, then the vectors call with the same outputs: the same bits as an unprepared call."""
    M, F, N = 256, 20, 30_000
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    engines, batch, keep = _batch(capi.KERNEL_GAUSSIAN_QNN, (1.0, 5.0), capi.TERM_LINEAR, M, F, rest)
    _, d = _device_inputs(P)
    plain, prepped = Outs(N, F), Outs(N, F)
    plain.call(batch, d, proj=True)
    batch.prepare_shared([t.data_ptr() for t in prepped.P], [t.data_ptr() for t in prepped.fall])
    prepped.call(batch, d, proj=True)
    torch.cuda.synchronize()
    for f in range(F):
        for a, b in zip(plain.host(f), prepped.host(f)):
            assert np.array_equal(a, b), f
    _close(engines, batch)
