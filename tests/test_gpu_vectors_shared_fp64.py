"""GPU: fd_batch_deform_vectors_shared_fp64_dev -- the Jacobian and the vectors it carries for every frame of a shot in
fp64, one matrix-pipe launch (k_vectors64_shared).

Yardsticks, fixed in advance:
  * test_gpu_vectors.py's fp64 restatement in numpy, at its fp64 bar: per vertex and frame
        ||A - A_ref||_F <= 2^-22 ||A_ref||_F + 1e-12 f S'
    (the fp32 rounding of A's entries plus the evaluation's own fp64 error against S' = sum |w_j| |grad phi_j| + |L|);
    t' and n' at test_gpu_vectors_shared._check_frame's bars with that absolute term;
  * the per-frame fp64 launches (fd_batch_deform_vectors_shared_dev on FD_EVAL_FP64 contexts):
        ||A - A_frame||_F <= 2^-23 ||A_frame||_F + 1e-12 f S'
    -- one fp32 rounding step: both sides round an fp64 value that differs only by summation order;
  * P_out and fd_falloff bit-identical to fd_batch_deform_shared_fp64_dev in the same run."""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_vectors import _field, _inputs, _model, _normalise, _projection, _rotation, KINDS, TERMS, RADIUS2, RATE
from test_gpu_vectors_shared import Outs as Outs32, SENTINEL, _batch, _close, _device_inputs

pytestmark = pytest.mark.gpu

NAME = "k_vectors64_shared"
BAR_REL, BAR_FRAME, BAR_ABS = 2.0 ** -22, 2.0 ** -23, 1e-12
FAST_KINDS = ("thin_plate", "gaussian", "qnn", "biharmonic", "cubic")
EYE = np.eye(3, dtype=np.float32)
# the fewest frames at which the one launch is taken (include/facedeform_hip.h)
MIN_FRAMES = {capi.KERNEL_THIN_PLATE: 2, capi.KERNEL_GAUSSIAN: 3, capi.KERNEL_GAUSSIAN_QNN: 3, capi.KERNEL_BIHARMONIC: 2, capi.KERNEL_CUBIC: 3}


class Outs(Outs32):
    """test_gpu_vectors_shared's outputs (N + 64 entries, a sentinel tail), filled by the fp64 call."""
    def call(self, batch, d, proj, dist2=True, stream_ptr=None, N=None, off=0, fp64=True):
        o = lambda t, w: t.data_ptr() + 4 * w * off
        ptr = lambda ts, w: [o(t, w) for t in ts]
        f = batch.deform_vectors_shared_fp64_dev if fp64 else batch.deform_vectors_shared_dev
        f(self.N if N is None else N, o(d["P"], 3), ptr(self.P, 3), d_dist2=o(d["d2"], 1) if dist2 else 0, d_falloff=ptr(self.fall, 1),
          d_tangents=(o(d["tu"], 3), o(d["tv"], 3), o(d["nrm"], 3)) if proj else None,
          d_N=o(d["Nv"], 3), d_N_out=ptr(self.No, 3), d_vtu=o(d["tu"], 3), d_vtu_out=ptr(self.tuo, 3),
          d_vtv=o(d["tv"], 3), d_vtv_out=ptr(self.tvo, 3), d_jacobian=ptr(self.A, 9),
          radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream_ptr)

    def host(self, f):
        tail = self.fall[f][self.N:].cpu().numpy()
        assert (tail == tail[0]).all() and tail[0] in (0.0, SENTINEL)          # fd_falloff past N untouched as well
        return super().host(f)


def _mesh(N, scale=1.0, offset=0.0):
    big = max(N, 20_000)
    return (synth.head_mesh(big)[:: big // N][:N] * np.float32(scale) + np.float32(offset)).astype(np.float32)


def _check_frame(A, No, tuo, tvo, fall, Pi, J, S, tu, tv, Nv):
    """Worst ratio against the fp64 bar for A and, carried through, for t' = A t and n' = cof(A) n rescaled to |n|
    (test_gpu_vectors_shared._check_frame's bars with the absolute term 1e-12)."""
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
                    np.cross(Aref[:, :, 0], Aref[:, :, 1])], axis=2)
    m = np.einsum("bij,bj->bi", cof, n64)
    nn = np.linalg.norm(n64, axis=1)
    want = _normalise(m) * nn[:, None]
    nb = 4.0 * np.linalg.norm(Aref, axis=(1, 2)) * bar * nn ** 2 / np.linalg.norm(m, axis=1) + 2.0 ** -22 * nn
    return max(ratio, float((np.linalg.norm(No - want, axis=1) / nb).max()))


def _assert_passed_through(outs, f, sel, tu, tv, Nv):
    _, _, No, tuo, tvo, A = outs.host(f)
    assert np.array_equal(No[sel], Nv[sel]) and np.array_equal(tuo[sel], tu[sel]) and np.array_equal(tvo[sel], tv[sel])
    assert np.array_equal(A[sel], np.broadcast_to(EYE, A[sel].shape))


def _positions(batch, d, N, F, proj):
    """fd_batch_deform_shared_fp64_dev with the same arguments: the bits P_out and fd_falloff must have."""
    Pref = [torch.full((N, 3), float(SENTINEL), device=d["P"].device) for _ in range(F)]
    fref = [torch.zeros(N, device=d["P"].device) for _ in range(F)]
    torch.cuda.synchronize()
    batch.deform_shared_fp64_dev(N, d["P"].data_ptr(), [t.data_ptr() for t in Pref], d_dist2=d["d2"].data_ptr(),
                                 d_falloff=[t.data_ptr() for t in fref],
                                 d_tangents=(d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr()) if proj else None,
                                 radius2=RADIUS2, falloffrate=RATE)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in Pref], [t.cpu().numpy() for t in fref]


def _run(kind, params, term, M, F, N=2_000, projs=(False, True), scale=1.0, offset=0.0, per_frame=True, deltas=None):
    """The new call against the restatement (and, per_frame, against the per-frame fp64 launches and the position call's
    bits in both fd_set_output modes); returns the worst ratios (restatement, per-frame)."""
    # (the grid follows the name function: below the kind's frame threshold the call runs the per-context fp64 launches, held to
    #  the same bars)
    assert capi.fd_shared_vectors_fp64_kernel_name(M, F, kind) == (NAME if F >= MIN_FRAMES[kind] else "")
    P = _mesh(N, scale, offset)
    rest = (synth.control_points(M, "head") * np.float32(scale) + np.float32(offset)).astype(np.float32)
    if deltas is None and scale != 1.0:
        base = synth.control_points(M, "head")
        deltas = np.stack([synth.smooth_deltas(base, f % 8) * np.float32(scale * (1.0 + 0.25 * (f // 8))) for f in range(F)]).astype(np.float32)
    engines, batch, keep = _batch(kind, params, term, M, F, rest, deltas=deltas, precision=capi.EVAL_FP64)
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    live = ~(dist2 > RADIUS2)
    lv = np.arange(N)[live]
    Pi_all = _projection(tu[lv], tv[lv], nrm[lv]) if lv.size else None
    refs = []
    for f in range(F):
        centres, Wr, aff, radii = _model(engines[f], kind, rest)
        _, J, S = _field(kind, P[lv].astype(np.float64), centres, Wr, aff, radii)
        refs.append((J, S))
    worst = worst_frame = 0.0
    for proj in projs:
        outs = Outs(N, F)
        outs.call(batch, d, proj)
        Pref, fref = _positions(batch, d, N, F, proj)
        per = None
        if per_frame:
            per = Outs(N, F)
            per.call(batch, d, proj, fp64=False)          # FD_EVAL_FP64 contexts: the per-context k_vectors64_<kind> launches
            torch.cuda.synchronize()
        for f in range(F):
            Pg, fall, No, tuo, tvo, A = outs.host(f)
            assert np.array_equal(Pg, Pref[f]) and np.array_equal(fall, fref[f]), f
            g = ~live
            _assert_passed_through(outs, f, g, tu, tv, Nv)
            z = live & (fall == 0)
            if N >= 97:
                assert z.any()
            _assert_passed_through(outs, f, z, tu, tv, Nv)
            if not lv.size:
                continue
            J, S = refs[f]
            assert np.isfinite(A).all()
            r = _check_frame(A[lv], No[lv], tuo[lv], tvo[lv], fall[lv], Pi_all if proj else None, J, S, tu[lv], tv[lv], Nv[lv])
            worst = max(worst, r)
            if per is not None:
                Af = per.host(f)[5][lv].astype(np.float64)
                bar = BAR_FRAME * np.linalg.norm(Af, axis=(1, 2)) + BAR_ABS * fall[lv].astype(np.float64) * S
                worst_frame = max(worst_frame, float((np.linalg.norm(A[lv].astype(np.float64) - Af, axis=(1, 2)) / bar).max()))
    if per_frame:
        # the position call's bits in the other fd_set_output mode as well
        for e in engines:
            e.set_output(capi.OUTPUT_DISPLACEMENT)
        outs = Outs(N, F)
        outs.call(batch, d, True)
        Pref, fref = _positions(batch, d, N, F, True)
        for f in range(F):
            Pg, fall = outs.host(f)[:2]
            assert np.array_equal(Pg, Pref[f]) and np.array_equal(fall, fref[f]), f
    _close(engines, batch)
    print(f"\nM = {M}, F = {F}, N = {N}: worst ratio against the restatement {worst:.3f}, against the per-frame launches {worst_frame:.3f}")
    return worst, worst_frame


# ---- against the numpy restatement and the per-frame launches ---------------------------------------------------------
@pytest.mark.parametrize("F", [1, 4, 5, 12, 13, 16, 17, 32])
@pytest.mark.parametrize("M", [32, 50, 256])
def test_thin_plate_at_the_edges_of_both_row_layouts(hip_lib, M, F):
    r, rf = _run(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F)
    assert r <= 1.0 and rf <= 1.0, (M, F, r, rf)


@pytest.mark.parametrize("F", [3, 13])
@pytest.mark.parametrize("term", sorted(TERMS))
@pytest.mark.parametrize("kind_name", FAST_KINDS)
def test_every_kind_and_term(hip_lib, kind_name, term, F):
    kind, params = KINDS[kind_name]
    r, rf = _run(kind, params, TERMS[term], 96, F)
    assert r <= 1.0 and rf <= 1.0, (kind_name, term, F, r, rf)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 33, 255, 257])
def test_vertex_edges(hip_lib, N):
    r, rf = _run(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, 32, 13, N=N)
    assert r <= 1.0 and rf <= 1.0, (N, r, rf)


def test_large_coordinates(hip_lib):
    """Mesh and rig at scale 100, offset 500: raw coordinates in fp64 on both sides, the same bar."""
    r, _ = _run(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, 96, 13, scale=100.0, offset=500.0, per_frame=False)
    assert r <= 1.0, r


# ---- models staged in chunks --------------------------------------------------------------------------------------------
def _chunks(M, F):
    """The launcher's arithmetic (fd_vectors_shared64.hip): K steps of four centres, staged in even chunks under 158 KiB of LDS."""
    NT = 3 * ((F + 15) // 16) if F > 12 else (F + 3) // 4
    nks = (M + 15) // 16 * 16 // 4
    fixed = 8 * (80 + NT * 64) + 8 * 4 * 32              # head + affine tiles, output pointers
    per_ks = 8 * (16 + NT * 64)
    kmax = (158 * 1024 - fixed) // per_ks
    return (nks + kmax - 1) // kmax


@pytest.mark.parametrize("M,F", [(256, 32), (240, 29)])
def test_chunked_models(hip_lib, M, F):
    assert _chunks(M, F) > 1 and _chunks(96, 32) == 1
    N, cut = 1_000, 389
    r, rf = _run(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, N=N)
    assert r <= 1.0 and rf <= 1.0, (M, F, r, rf)
    # [0, N) in one call equals two calls over two ranges, and two identical calls give identical bits
    P = _mesh(N); rest = synth.control_points(M, "head")
    engines, batch, keep = _batch(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest)
    _, d = _device_inputs(P)
    one, again, two = Outs(N, F), Outs(N, F), Outs(N, F)
    one.call(batch, d, True)
    again.call(batch, d, True)
    two.call(batch, d, True, N=cut)
    two.call(batch, d, True, N=N - cut, off=cut)
    torch.cuda.synchronize()
    for f in range(F):
        for a, b, c in zip(one.host(f), again.host(f), two.host(f)):
            assert np.array_equal(a, b) and np.array_equal(a, c), f
    _close(engines, batch)


# ---- pass-through ---------------------------------------------------------------------------------------------------------
def test_gated_vertices_zero_falloff_and_a_failed_build_pass_through(hip_lib):
    """A third of the vertices gated, some exactly on the radius (f = 0), and the last frame's build failed on coincident
    centres -- produced as in test_gpu_shared_fp64.py: the failure is still unknown to the host when the call is made, so
    the device decides.  Vectors bit for bit, A = I exactly, sentinel tails untouched in every output."""
    N, M, F, big = 2_000, 96, 5, 1_000_000
    dev = torch.device("cuda", 0)
    P = _mesh(N); rest = synth.control_points(M, "head")
    (tu, tv, nrm, Nv, dist2), d = _device_inputs(P)
    S = torch.cuda.Stream(device=dev)
    deltas = np.stack([synth.smooth_deltas(rest, f) for f in range(F)]).astype(np.float32)
    d_rest = torch.from_numpy(rest).to(dev); d_del = torch.from_numpy(deltas).to(dev)
    engines = []
    for _ in range(F):
        e = capi.Engine(); e.set_stream(S.cuda_stream); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR); engines.append(e)
    head, lone, batch = capi.Batch(engines[:-1]), capi.Batch([engines[-1]]), capi.Batch(engines)
    head.set_points_dev([d_rest.data_ptr()] * (F - 1), [d_del[k].data_ptr() for k in range(F - 1)], M)
    head.build_async(S.cuda_stream); assert [r.terminationtype for r in head.build_result()] == [1] * (F - 1)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream); assert lone.build_result()[0].terminationtype == 1
    dup = rest.copy(); dup[1] = dup[0]
    d_rest.copy_(torch.from_numpy(dup).to(dev))                 # the same array, now with two coincident control points
    d_big = torch.from_numpy(synth.head_mesh(big)).to(dev)
    scratch = [torch.empty_like(d_big) for _ in range(F - 1)]
    outs = Outs(N, F)
    torch.cuda.synchronize()
    for _ in range(60):          # keeps the stream busy for several milliseconds
        head.deform_shared_fp64_dev(big, d_big.data_ptr(), [t.data_ptr() for t in scratch], stream_ptr=S.cuda_stream)
    lone.set_points_dev([d_rest.data_ptr()], [d_del[F - 1].data_ptr()], M)
    lone.build_async(S.cuda_stream)
    outs.call(batch, d, True, stream_ptr=S.cuda_stream)
    torch.cuda.synchronize()
    assert lone.build_result(check=False)[0].terminationtype == -5
    gated = dist2 > np.float32(RADIUS2)
    assert gated.sum() > N // 4
    for f in range(F - 1):
        Pg, fall, _, _, _, A = outs.host(f)                     # (host() checks the sentinel tails of every output)
        _assert_passed_through(outs, f, gated, tu, tv, Nv)
        z = ~gated & (fall == 0)
        assert z.any()
        _assert_passed_through(outs, f, z, tu, tv, Nv)
        moving = ~gated & (fall != 0)
        assert not np.array_equal(A[moving], np.broadcast_to(EYE, A[moving].shape))
    Pg = outs.host(F - 1)[0]
    assert np.array_equal(Pg, P)
    _assert_passed_through(outs, F - 1, np.ones(N, bool), tu, tv, Nv)          # the failed frame: every vertex
    for b in (head, lone, batch):
        b.close()
    for e in engines:
        e.set_stream(None); e.close()


# ---- rigid motion -----------------------------------------------------------------------------------------------------------
def test_rigid_motion_gives_the_rotation(hip_lib):
    M, F, N = 96, 5, 2_000
    rest = synth.control_points(M, "head")
    P = _mesh(N)
    p0 = np.array([0.4, -0.3, 0.25])
    Rs = [_rotation(0.05 + 0.04 * f, [0.3, 1.0 - 0.2 * f, -0.2]) for f in range(F)]
    deltas = np.stack([((rest.astype(np.float64) - p0) @ R.T + p0 - rest).astype(np.float32) for R in Rs])
    engines, batch, keep = _batch(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest, deltas=deltas)
    (tu, tv, nrm, Nv, _), d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, proj=False, dist2=False)
    torch.cuda.synchronize()
    # "to the fp32 rounding of its entries": A's entries (of size <= 1) are rounded to fp32, 2^-24; and the model interpolates
    # deltas that are themselves the motion rounded to fp32 -- eta = 2^-24 max |coordinate| on each control point -- so its
    # derivative is R only to 2 eta / h, h the smallest distance between two control points (two neighbours pushed opposite ways)
    D = np.linalg.norm(rest[:, None, :].astype(np.float64) - rest[None], axis=2)
    h = D[D > 0].min()
    moved = np.abs(rest.astype(np.float64)).max() + np.abs(deltas.astype(np.float64)).max()
    bound = 2.0 ** -24 + 2.0 * 2.0 ** -24 * moved / h
    for f in range(F):
        _, _, No, _, _, A = outs.host(f)
        print(f"rigid motion frame {f}: max |A - R| = {np.abs(A - Rs[f][None]).max():.3e} (bound {bound:.3e})")
        assert np.abs(A - Rs[f][None]).max() <= bound, (f, np.abs(A - Rs[f][None]).max(), bound)
        assert np.abs(No - Nv.astype(np.float64) @ Rs[f].T).max() <= 1e-6, f
    _close(engines, batch)


# ---- rebuild while the launch runs ------------------------------------------------------------------------------------------
def test_contexts_may_be_rebuilt_once_the_launch_has_its_copy(hip_lib):
    N, M, F = 50_000, 256, 16
    dev = torch.device("cuda", 0)
    P = _mesh(N); rest = synth.control_points(M, "head")
    sA, sB = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    engines, batch, keep = _batch(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest)
    _, d = _device_inputs(P)
    quiet, raced = Outs(N, F), Outs(N, F)
    quiet.call(batch, d, True, stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    other = torch.from_numpy(np.stack([synth.smooth_deltas(rest, (f + 3) % 8) * np.float32(0.5) for f in range(F)]).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    raced.call(batch, d, True, stream_ptr=sA.cuda_stream)
    batch.wait_consumed(sB.cuda_stream)
    batch.set_points_dev([keep[0].data_ptr()] * F, [other.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(sB.cuda_stream)
    torch.cuda.synchronize()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    for f in range(F):
        for a, b in zip(quiet.host(f), raced.host(f)):
            assert np.array_equal(a, b), f                    # the first models' outputs
    after = Outs(N, F)
    after.call(batch, d, True, stream_ptr=sA.cuda_stream)
    torch.cuda.synchronize()
    assert not np.array_equal(after.host(0)[5], quiet.host(0)[5])          # and now the second models'
    _close(engines, batch)


# ---- fallback ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["multilayer", "eval_variant"])
def test_fallback_is_the_per_context_fp64_launch_bit_for_bit(hip_lib, case):
    M, F, N = 64, 3, 2_000
    kind, params = KINDS["multilayer" if case == "multilayer" else "thin_plate"]
    if case == "multilayer":
        assert capi.fd_shared_vectors_fp64_kernel_name(M, F, kind) == ""
    dev = torch.device("cuda", 0)
    P = _mesh(N); rest = synth.control_points(M, "head")
    deltas = np.stack([synth.smooth_deltas(rest, f) for f in range(F)]).astype(np.float32)
    d_rest = torch.from_numpy(rest).to(dev); d_del = torch.from_numpy(deltas).to(dev)
    engines = []
    for _ in range(F):
        e = capi.Engine(variant=2 if case == "eval_variant" else 0)          # contexts left at fp32: the call evaluates in fp64
        e.set_kernel(kind, list(params)); e.set_term(capi.TERM_LINEAR); engines.append(e)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    _, d = _device_inputs(P)
    outs = Outs(N, F)
    outs.call(batch, d, True)
    torch.cuda.synchronize()
    for f, e in enumerate(engines):
        e.set_eval_precision(capi.EVAL_FP64)
        ref = Outs(N, 1)
        e.deform_vectors_dev(N, d["P"].data_ptr(), ref.P[0].data_ptr(), d["d2"].data_ptr(), ref.fall[0].data_ptr(),
                             d["tu"].data_ptr(), d["tv"].data_ptr(), d["nrm"].data_ptr(), d["Nv"].data_ptr(), ref.No[0].data_ptr(),
                             d["tu"].data_ptr(), ref.tuo[0].data_ptr(), d["tv"].data_ptr(), ref.tvo[0].data_ptr(), ref.A[0].data_ptr(),
                             radius2=RADIUS2, falloffrate=RATE)
        torch.cuda.synchronize()
        for a, b in zip(outs.host(f), ref.host(0)):
            assert np.array_equal(a, b), (case, f)
        assert not np.array_equal(outs.host(f)[5], np.broadcast_to(EYE, (N, 3, 3)))
    _close(engines, batch)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(hip_lib):
    import ctypes as C
    N, M, F = 500, 64, 3
    dev = torch.device("cuda", 0)
    P = _mesh(N); rest = synth.control_points(M, "head")
    engines, batch, keep = _batch(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, M, F, rest)
    one = capi.Batch(engines[:1])
    _, d = _device_inputs(P)
    outs, outs1 = Outs(N, F), Outs(N, 1)
    for t in outs.fall + outs1.fall:
        t.fill_(float(SENTINEL))
    torch.cuda.synchronize()
    vp = C.c_void_p
    L = capi.load()

    def call(b, o, **over):
        n = len(o.P)
        tab = lambda ts: (vp * n)(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])
        a = dict(P_in=d["P"].data_ptr(), P_out=tab(o.P), d2=d["d2"].data_ptr(), fall=tab(o.fall), tu=d["tu"].data_ptr(), tv=d["tv"].data_ptr(),
                 nrm=d["nrm"].data_ptr(), size=C.sizeof(capi.FdBatchVectors), vN=d["Nv"].data_ptr(), No=tab(o.No), vtu=d["tu"].data_ptr(),
                 tuo=tab(o.tuo), vtv=d["tv"].data_ptr(), tvo=tab(o.tvo), jac=tab(o.A), N=N)
        a.update({k: (tab(v) if isinstance(v, list) else v) for k, v in over.items()})
        vec = capi.FdBatchVectors(a["size"], vp(a["vN"]), a["No"], vp(a["vtu"]), a["tuo"], vp(a["vtv"]), a["tvo"], a["jac"])
        return L.fd_batch_deform_vectors_shared_fp64_dev(b.h, None, a["N"], vp(a["P_in"]), a["P_out"], vp(a["d2"]), a["fall"], vp(a["tu"]),
                                                         vp(a["tv"]), vp(a["nrm"]), RADIUS2, RATE, C.byref(vec))

    shared = [d[k].data_ptr() for k in ("P", "d2", "tu", "tv", "nrm", "Nv")]
    for table, ts in (("P_out", outs.P), ("fall", outs.fall), ("No", outs.No), ("tuo", outs.tuo), ("tvo", outs.tvo), ("jac", outs.A)):
        for s in shared:                                                    # every aliasing pair
            assert call(batch, outs, **{table: [ts[0], s, ts[2]]}) == capi.FD_E_INVALID, (table, s)
        assert call(batch, outs, **{table: [ts[0], None, ts[2]]}) == capi.FD_E_INVALID, table          # a NULL table entry
    for s in shared:
        assert call(one, outs1, P_out=[s]) == capi.FD_E_INVALID            # a batch of one in place, and over any other input
    assert call(batch, outs, size=C.sizeof(capi.FdBatchVectors) - 8) == capi.FD_E_INVALID          # a short struct_size
    assert call(batch, outs, No=None) == capi.FD_E_INVALID                 # an input without its output table
    assert call(batch, outs, vtu=None) == capi.FD_E_INVALID                # an output table without its input
    assert call(batch, outs, N=0) == capi.FD_OK
    for e, mode in zip(engines, (capi.OUTPUT_POSITION, capi.OUTPUT_DISPLACEMENT, capi.OUTPUT_POSITION)):
        e.set_output(mode)
    assert call(batch, outs) == capi.FD_E_INVALID                          # differing fd_set_output settings
    for e in engines:
        e.set_output(capi.OUTPUT_POSITION)
    # contexts with different rest arrays
    d_rest = [torch.from_numpy(rest).to(dev) for _ in range(F)]
    batch.set_points_dev([t.data_ptr() for t in d_rest], [keep[1].data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    assert call(batch, outs) == capi.FD_E_INVALID
    torch.cuda.synchronize()
    for o in (outs, outs1):
        for ts in (o.P, o.fall, o.No, o.tuo, o.tvo, o.A):
            for t in ts:
                assert bool((t == float(SENTINEL)).all())                   # nothing was written
    one.close()
    _close(engines, batch)
