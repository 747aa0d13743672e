"""GPU: the morph-space reprojection of all frames of a shot in one pass over each matrix
(fd_morph_compute_weights_batch_dev, fd_morph_displace_batch_dev, fd_morph_get_weights_batch) against the oracle
(reference src/dbse.cpp:39-77, SOP_FaceDeform.cpp:444-473) and against the one-frame calls, which are unchanged.

Bars, the existing ones of test_gpu_morph.py: weights <= 1e-10 * max(1, max|w_ref|) per frame (fp64 on both sides,
another summation order); displacement: the fp32 loop is the reference's own operation order, so GIVEN THE SAME
WEIGHTS the positions are bit-identical to oracle.morph_displace -- asserted with np.array_equal for the batched
call on its weights and for the one-frame call on its own."""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu
W_TOL = 1e-10
CLAMP = (-0.05, 0.08)


def _setup(N, S, F, seed, own_rest=False):
    """A rest pose, S sparse blendshapes, F frames: mixtures of a few shapes plus noise; frames 1, 4, 7, .. (F > 1) ARE
    the rest the passes measure against (weights exactly 0).  own_rest: the object gets a `rest` attribute of its own."""
    rng = np.random.default_rng(seed)
    rest = synth.head_mesh(N) if N >= 1000 else rng.normal(size=(N, 3)).astype(np.float32)
    shapes = [(rest + (0.05 * rng.normal(size=(N, 3)) * (rng.random((N, 1)) < 0.4)).astype(np.float32)).astype(np.float32)
              for _ in range(S)]
    if S > 6:
        shapes[5] = rest.copy()                                # a zero column
    attr = (rest + np.float32(0.001) * rng.normal(size=(N, 3)).astype(np.float32)).astype(np.float32) if own_rest else rest
    frames = []
    for f in range(F):
        if F > 1 and f % 3 == 1:
            frames.append(attr.copy())
            continue
        P = rest.astype(np.float32).copy()
        for _ in range(min(S, 3)):
            s = int(rng.integers(S))
            P = (P + np.float32(rng.uniform(-0.6, 0.9)) * (shapes[s] - rest)).astype(np.float32)
        frames.append((P + (0.002 * rng.normal(size=(N, 3))).astype(np.float32)).astype(np.float32))
    return rest, shapes, attr, frames


def _w_bar(w, w_ref, what):
    err, bar = float(np.abs(w - w_ref).max()) if w.size else 0.0, W_TOL * max(1.0, float(np.abs(w_ref).max()) if w_ref.size else 0.0)
    print(f"{what}: max|w - w_ref| = {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (what, err, bar)


CASES = [  # N, S, F, own rest attribute
    (1, 1, 1, False), (1, 3, 2, False), (63, 5, 7, False), (63, 16, 16, True), (1000, 1, 32, False), (1000, 50, 17, False),
    (1000, 100, 20, True), (1000, 130, 32, False), (20_011, 5, 1, False), (20_011, 16, 2, True), (20_011, 50, 32, False),
    (20_011, 130, 20, False), (20_011, 100, 7, False),
    # the edges of the 64-column groups and of the 8 / 16 / 32-frame tiles, the column-by-column factorisation (S > 256),
    # rows an exact multiple of the one-frame weights' 2048; all of them exercise the clamp (checked with the oracle's weights)
    (1000, 64, 8, False), (1000, 65, 9, False), (1000, 128, 8, False), (1000, 129, 9, False), (1000, 257, 16, False),
    (1000, 300, 32, False), (2048, 16, 1, False),
]


@pytest.mark.parametrize("N,S,F,own_rest", CASES)
def test_weights_and_displacement_against_the_oracle(hip_lib, oracle, N, S, F, own_rest):
    rest, shapes, attr, frames = _setup(N, S, F, 1000 * S + F + N, own_rest)
    A = oracle.morph_shapes_matrix(rest, shapes)
    QR_ref, _ = oracle.morph_qr(A)
    w_ref = np.stack([oracle.morph_weights(QR_ref, P, attr) for P in frames])
    dev = torch.device("cuda", 0)
    m = capi.Morph()
    m.init(rest, shapes)
    if own_rest:
        m.set_rest(attr)
    d_frames = [torch.from_numpy(P).to(dev) for P in frames]
    torch.cuda.synchronize()
    # ---- weights: the oracle per frame, and the one-frame call frame by frame
    m.compute_weights_batch_dev([t.data_ptr() for t in d_frames])
    wb = m.weights_batch()
    assert wb.shape == (F, S) and np.isfinite(wb).all()
    assert not m.computed                                     # the one-frame state is another one
    w_one = np.empty_like(wb)
    for f in range(F):
        m.compute_weights_dev(d_frames[f].data_ptr())
        w_one[f] = m.weights()
    for f in range(F):
        _w_bar(wb[f], w_ref[f], f"N={N} S={S} F={F} frame {f} vs oracle")
        _w_bar(wb[f], w_one[f], f"N={N} S={S} F={F} frame {f} vs one-frame call")
        if F > 1 and f % 3 == 1:
            assert np.all(wb[f] == 0.0)                       # P = rest: every product is zero
    # the read-only call takes a table whose entries repeat
    m.compute_weights_batch_dev([d_frames[0].data_ptr()] * F)
    wrep = m.weights_batch()
    assert all(np.array_equal(wrep[f], wrep[0]) for f in range(F))
    _w_bar(wrep[0], w_ref[0], "repeated entries")
    m.compute_weights_batch_dev([t.data_ptr() for t in d_frames])
    assert np.array_equal(m.weights_batch(), wb)
    # ---- displacement, clamp off/on, add_delta off/on
    if S >= 16 and N >= 1000:
        assert (3 * wb > CLAMP[1]).any() and (3 * wb < CLAMP[0]).any(), "the clamp must be exercised"
    stream = torch.cuda.Stream(device=dev)
    for clamp, add_delta, fr in ((None, False, 0.0), (CLAMP, False, 0.0), (None, True, 0.5), (CLAMP, True, 0.25)):
        guard = np.float32(-7.5)
        work = [torch.full((N + 5, 3), float(guard), device=dev) for _ in range(F)]      # five guard vertices past N
        for f in range(F):
            work[f][:N] = d_frames[f]
        torch.cuda.synchronize()
        m.compute_weights_batch_dev([t.data_ptr() for t in work], stream.cuda_stream)
        m.displace_batch_dev([t.data_ptr() for t in work], clamp, add_delta, fr, stream.cuda_stream)   # weights in stream order
        stream.synchronize()
        assert np.array_equal(m.weights_batch(), wb)
        for f in range(F):
            out = work[f].cpu().numpy()
            assert np.all(out[N:] == guard), "entries past N were touched"
            ref = oracle.morph_displace(A, wb[f], frames[f], attr, clamp, add_delta, fr)
            assert np.array_equal(out[:N], ref), (f, clamp, add_delta)
            # the one-frame pair on a copy of the same frame: the same arithmetic on ITS weights
            d_copy = d_frames[f].clone()
            torch.cuda.synchronize()
            m.compute_weights_dev(d_copy.data_ptr())
            m.displace_dev(d_copy.data_ptr(), clamp, add_delta, fr)
            w1 = m.weights()
            assert np.array_equal(w1, w_one[f])
            assert np.array_equal(d_copy.cpu().numpy(), oracle.morph_displace(A, w1, frames[f], attr, clamp, add_delta, fr))
    m.close()


def test_no_shapes(hip_lib):
    """S = 0 as the one-frame calls: no weights, P = rest [+ (P - rest) * falloffradius]."""
    rng = np.random.default_rng(5)
    N, F = 777, 3
    rest = rng.normal(size=(N, 3)).astype(np.float32)
    frames = [(rest + 0.1 * rng.normal(size=(N, 3))).astype(np.float32) for _ in range(F)]
    dev = torch.device("cuda", 0)
    m = capi.Morph()
    m.init(rest, [])
    for add_delta in (False, True):
        work = [torch.from_numpy(P).to(dev) for P in frames]
        one = [t.clone() for t in work]
        torch.cuda.synchronize()
        m.compute_weights_batch_dev([t.data_ptr() for t in work])
        assert m.weights_batch().shape == (F, 0)
        m.displace_batch_dev([t.data_ptr() for t in work], None, add_delta, 0.5)
        for f in range(F):
            m.compute_weights_dev(one[f].data_ptr())
            m.displace_dev(one[f].data_ptr(), None, add_delta, 0.5)
        m.weights_batch()                                     # drains the object's stream
        for f in range(F):
            assert np.array_equal(work[f].cpu().numpy(), one[f].cpu().numpy())
            if not add_delta:
                assert np.array_equal(work[f].cpu().numpy(), rest)
    m.close()


def test_the_two_states_are_independent(hip_lib):
    rng = np.random.default_rng(21)
    N, S, F = 5_003, 23, 5
    rest, shapes, _, frames = _setup(N, S, F, 77)
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(P).to(dev) for P in frames]
    other = torch.from_numpy((rest + 0.3 * (shapes[2] - rest)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d_frames]
    L = hip_lib
    m = capi.Morph()
    w = np.zeros(F * S)
    wp = w.ctypes.data_as(capi._f64p)
    import ctypes as C
    tab = (C.c_void_p * F)(*ptrs)
    # before fd_morph_init, and after it before a batched compute: not built
    assert L.fd_morph_compute_weights_batch_dev(m.h, F, tab, None) == capi.FD_E_NOT_BUILT
    m.init(rest, shapes)
    assert L.fd_morph_displace_batch_dev(m.h, F, tab, None, 0, 0.0, None) == capi.FD_E_NOT_BUILT
    assert L.fd_morph_get_weights_batch(m.h, F, wp) == capi.FD_E_NOT_BUILT
    with pytest.raises(capi.FdError):
        m.weights_batch()
    # one-frame compute, batched compute, one-frame weights: unchanged bit for bit
    m.compute_weights_dev(other.data_ptr())
    w_one = m.weights().copy()
    assert m.computed
    m.compute_weights_batch_dev(ptrs)
    wb = m.weights_batch().copy()
    assert np.array_equal(m.weights(), w_one) and m.computed
    # the converse: a one-frame compute leaves the batched weights alone
    m.compute_weights_dev(d_frames[0].data_ptr())
    assert np.array_equal(m.weights_batch(), wb)
    assert not np.array_equal(m.weights(), w_one)
    # another F than the last batched compute's: invalid, for the displacement and the read-back; so are the argument errors
    for Fbad in (F - 1, F + 1):
        assert L.fd_morph_displace_batch_dev(m.h, Fbad, (C.c_void_p * (F + 1))(*ptrs, other.data_ptr()), None, 0, 0.0, None) == capi.FD_E_INVALID
        assert L.fd_morph_get_weights_batch(m.h, Fbad, np.zeros((F + 1) * S).ctypes.data_as(capi._f64p)) == capi.FD_E_INVALID
    assert "hold" in m.L.fd_morph_last_error(m.h).decode()
    assert L.fd_morph_compute_weights_batch_dev(m.h, 0, tab, None) == capi.FD_E_INVALID
    assert L.fd_morph_compute_weights_batch_dev(m.h, 33, tab, None) == capi.FD_E_INVALID
    assert L.fd_morph_compute_weights_batch_dev(m.h, F, None, None) == capi.FD_E_INVALID
    assert L.fd_morph_compute_weights_batch_dev(m.h, 2, (C.c_void_p * 2)(ptrs[0], None), None) == capi.FD_E_INVALID
    assert L.fd_morph_displace_batch_dev(m.h, F, (C.c_void_p * F)(*(ptrs[:F - 1] + [ptrs[0]])), None, 0, 0.0, None) == capi.FD_E_INVALID
    assert "same array" in m.L.fd_morph_last_error(m.h).decode()
    assert np.array_equal(m.weights_batch(), wb)              # none of them disturbed the state
    # fd_morph_init clears the batched state (and, as before, the one-frame state)
    m.init(rest, shapes)
    assert not m.computed
    assert L.fd_morph_displace_batch_dev(m.h, F, tab, None, 0, 0.0, None) == capi.FD_E_NOT_BUILT
    assert L.fd_morph_get_weights_batch(m.h, F, wp) == capi.FD_E_NOT_BUILT
    m.compute_weights_batch_dev(ptrs)
    assert np.array_equal(m.weights_batch(), wb)
    assert not m.computed
    m.close()


def test_behind_the_shot_path(hip_lib, oracle):
    """fd_batch_deform_shared_dev writes d_P_out for 20 thin-plate frames; the batched morph pair runs on that table as it
    stands and equals the per-frame morph calls on copies of the same arrays."""
    rng = np.random.default_rng(31)
    N, M, F, S = 20_000, 64, 20, 12
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(N)
    rig = synth.control_points(M, "head")
    deltas = np.stack([synth.smooth_deltas(rig, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(F)]).astype(np.float32)
    shapes = [(P + (0.08 * rng.normal(size=(N, 3)) * (rng.random((N, 1)) < 0.5)).astype(np.float32)).astype(np.float32) for _ in range(S)]
    d_P, d_rig, d_del = (torch.from_numpy(a).to(dev) for a in (P, rig, deltas))
    engines = []
    for _ in range(F):
        e = capi.Engine(device=0); e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR); engines.append(e)
    batch = capi.Batch(engines)
    batch.set_points_dev([d_rig.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async()
    assert [r.terminationtype for r in batch.build_result()] == [1] * F
    guard = np.float32(123.25)
    pad = 7
    outs = [torch.full((N + pad, 3), float(guard), device=dev) for _ in range(F + 1)]    # one array more: no frame's
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    table = [o.data_ptr() for o in outs[:F]]
    batch.deform_shared_dev(N, d_P.data_ptr(), table, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    rbf = [o[:N].clone() for o in outs[:F]]                    # copies of the RBF results, for the per-frame calls
    rbf_host = [t.cpu().numpy() for t in rbf]
    m = capi.Morph()
    m.init(P, shapes)                                          # rest = the incoming mesh, as the cook has it
    m.compute_weights_batch_dev(table, stream.cuda_stream)
    m.displace_batch_dev(table, (-0.01, 0.02), True, 0.25, stream.cuda_stream)
    stream.synchronize()
    wb = m.weights_batch()
    A = oracle.morph_shapes_matrix(P, shapes)
    QR_ref, _ = oracle.morph_qr(A)
    assert (np.abs(3 * wb) > 0.02).any(), "the clamp must be exercised"
    for f in range(F):
        _w_bar(wb[f], oracle.morph_weights(QR_ref, rbf_host[f], P), f"shot frame {f} vs oracle")
        m.compute_weights_dev(rbf[f].data_ptr())
        m.displace_dev(rbf[f].data_ptr(), (-0.01, 0.02), True, 0.25)
        w1 = m.weights()
        _w_bar(wb[f], w1, f"shot frame {f} vs one-frame call")
        out = outs[f].cpu().numpy()
        assert np.all(out[N:] == guard)
        assert np.array_equal(out[:N], oracle.morph_displace(A, wb[f], rbf_host[f], P, (-0.01, 0.02), True, 0.25))
        one = rbf[f].cpu().numpy()
        assert np.array_equal(one, oracle.morph_displace(A, w1, rbf_host[f], P, (-0.01, 0.02), True, 0.25))
        same = np.array_equal(np.float32(3 * wb[f]), np.float32(3 * w1))
        assert not same or np.array_equal(out[:N], one)        # equal float(3 w): the two paths agree bit for bit
    assert np.all(outs[F].cpu().numpy() == guard)              # an array of no frame
    # a shorter table: the frames left out stay as they are
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()
    m.compute_weights_batch_dev(table[:3])
    m.displace_batch_dev(table[:3], None, False, 0.0)
    m.weights_batch()
    for f in range(3, F + 1):
        assert torch.equal(outs[f], before[f])
    m.close(); batch.close()
    for e in engines:
        e.close()


def _full_size(rng, N, S):
    rest = synth.head_mesh(N)
    bumps = rng.normal(size=(S, 3)).astype(np.float32)
    shapes = []
    for s in range(S):
        centre = rest[rng.integers(N)]
        wgt = np.exp(-np.sum((rest - centre) ** 2, axis=1) / 0.05).astype(np.float32)
        shapes.append((rest + wgt[:, None] * bumps[s] * np.float32(0.1)).astype(np.float32))
    return rest, shapes


def test_full_size_properties_and_repeatability(hip_lib, oracle):
    """N = 1M, S = 50, F = 32: what test_full_size_properties holds for one frame.  (a) frames equal to the rest pose give
    zero weights and come back bit-identical; (b) the weights are linear in the deformation; (c) a 4k-vertex sample of the
    displacement equals the oracle's on the batch's weights; (d) three batched computes on the same inputs give the same
    bits; (e) per frame the weights hold the 1e-10 bar against the one-frame call."""
    rng = np.random.default_rng(2)
    N, S, F = 1_000_000, 50, 32
    rest, shapes = _full_size(rng, N, S)
    dev = torch.device("cuda", 0)
    m = capi.Morph()
    m.init(rest, shapes)
    QR, _ = m.qr()
    d1 = (np.float32(0.5) * (shapes[3] - rest)).astype(np.float32)
    d2 = (np.float32(0.25) * (shapes[9] - rest)).astype(np.float32)
    host = {0: rest, 1: (rest + d1).astype(np.float32), 2: (rest + d2).astype(np.float32), 3: (rest + (d1 + d2)).astype(np.float32), 31: rest}
    frames = []
    for f in range(F):
        if f in host:
            frames.append(torch.from_numpy(host[f]).to(dev))
        else:   # a mixture of two shapes, formed on the device
            a, b = int(rng.integers(S)), int(rng.integers(S))
            t = torch.from_numpy(rest).to(dev)
            t = t + float(rng.uniform(-0.6, 0.9)) * (torch.from_numpy(shapes[a]).to(dev) - t) + float(rng.uniform(-0.6, 0.9)) * (torch.from_numpy(shapes[b]).to(dev) - t)
            frames.append(t.contiguous())
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in frames]
    runs = []
    for _ in range(3):
        m.compute_weights_batch_dev(ptrs)
        runs.append(m.weights_batch().copy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    wb = runs[0]
    assert np.all(wb[0] == 0.0) and np.all(wb[31] == 0.0)
    # linear in the fp32 delta actually formed: compare with the weights of d1 + d2 as rounded
    dd = [(host[k] - rest).astype(np.float32) for k in (1, 2, 3)]
    resid = (dd[2].astype(np.float64) - dd[0] - dd[1]).reshape(-1)
    lin = np.abs(wb[3] - (wb[1] + wb[2]) - resid @ QR).max()
    print(f"linearity residual {lin:.3e}")
    assert lin <= 1e-9 * max(1.0, np.abs(wb[3]).max())
    del QR
    for f in range(F):
        m.compute_weights_dev(ptrs[f])
        _w_bar(wb[f], m.weights(), f"1M frame {f} vs one-frame call")
    before = {f: frames[f].cpu().numpy() for f in (5, 17, 30)}
    m.displace_batch_dev(ptrs, (-0.3, 0.4), True, 0.25)
    assert np.array_equal(m.weights_batch(), wb)
    assert (np.abs(3 * wb) > 0.4).any(), "the clamp must be exercised"
    assert np.array_equal(frames[0].cpu().numpy(), rest) and np.array_equal(frames[31].cpu().numpy(), rest)
    idx = np.unique(np.concatenate([rng.integers(N, size=4000), [0, 63, 64, 255, 256, N - 1]]))
    A = oracle.morph_shapes_matrix(rest[idx], [s[idx] for s in shapes])
    for f, P_before in before.items():
        ref = oracle.morph_displace(A, wb[f], P_before[idx], rest[idx], (-0.3, 0.4), True, 0.25)
        assert np.array_equal(frames[f].cpu().numpy()[idx], ref), f
    m.close()
