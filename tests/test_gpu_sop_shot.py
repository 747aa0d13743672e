"""GPU: fdsop_cook_shot / FaceDeformSOP.cook_shot -- all frames of a shot through the node in one call
(include/facedeform_hip.h, facedeform_amd/csrc/fd_sop_host.cpp, the device side in fd_capi.hip behind fd_shot_dev.h).

Frame k of a shot is the k-th of F consecutive cooks: every frame is held to the oracle with the bars fdsop_cook's own tests
use -- parity_ratio(1e-5) <= 1 and l2_parity_ulp <= 1 for fp32 frames, the raw l2_parity <= 1e-5 for frames evaluated in
fp64, fd_falloff with rtol 2e-6 / atol 1e-7 -- and fdsop_shot_paths says which build and launches a group took."""
import numpy as np
import pytest

from conftest import l2_parity, l2_parity_ulp, parity_ratio
from facedeform_amd import capi, synth
from facedeform_amd.sop import FaceDeformSOP
from oracle import fd_oracle as fo
from test_gpu_fp32_contract import _mesh, _rig

pytestmark = pytest.mark.gpu

TOL = 1e-5
N_SPHERE = 10_007                    # not a multiple of 32
TERMINATION = "Termination type: 1, Iterations: "


@pytest.fixture(scope="module")
def sphere():
    P = synth.sphere_mesh(N_SPHERE)
    dist2 = (0.6 * np.abs(P[:, 0])).astype(np.float32)
    return P, dist2


def _frames(rest, F, first=0):
    return [synth.deformed_rig(rest, first + k) for k in range(F)]


def _oracle_frame(oracle, okind, params, rest, deform, P, **kw):
    table = oracle.control_table(rest, deform)
    rc, tt, W, radii = oracle.build(table, okind, params, fo.TERM_LINEAR)
    assert rc == 0 and tt == 1
    return oracle.deform(table, okind, radii, W, P, **kw)


def _hold_fp32(out, ref, P):
    assert parity_ratio(out, ref, P, TOL) <= 1.0, parity_ratio(out, ref, P, TOL)
    assert l2_parity_ulp(out, ref, P, TOL) <= 1.0, l2_parity_ulp(out, ref, P, TOL)


def test_defaults_qnn_linear_term_with_gate_and_falloff(hip_lib, oracle, sphere):
    P, dist2 = sphere
    M, F = 32, 5
    rest = synth.control_points(M, "sphere")
    frames = _frames(rest, F)
    node = FaceDeformSOP()
    node.set("radius", 0.7); node.set("falloffrate", 1.5)
    res = node.cook_shot(P, rest, frames, dist2=dist2)
    assert res.severity == capi.FDSOP_MESSAGE, (res.messages, [f.messages for f in res.frames])
    assert res.messages == [] and len(res.frames) == F
    r2 = np.float32(0.7) * np.float32(0.7)
    gated = dist2 > r2
    assert gated.any() and not gated.all()
    for k, fr in enumerate(res.frames):
        ref, ref_fall = _oracle_frame(oracle, fo.KERNEL_GAUSSIAN_QNN, [1.0, 5.0, 0.0], rest, frames[k], P, dist2=dist2, radius2=r2,
                                      falloffrate=1.5)
        _hold_fp32(fr.P, ref, P)
        assert np.allclose(fr.fd_falloff, ref_fall, rtol=2e-6, atol=1e-7)
        assert np.array_equal(fr.P[gated], P[gated]) and np.all(fr.fd_falloff[gated] == 0.0)
        assert fr.severity == capi.FDSOP_MESSAGE
        assert len(fr.infos) == 1 and fr.infos[0].startswith(TERMINATION), fr.messages
    assert np.array_equal(res.frames[0].Cd, np.ones_like(P))
    assert res.paths == [(0, F, "", capi.fd_shared_kernel_name(M, F, capi.KERNEL_GAUSSIAN_QNN), F, "", 0)]
    assert res.paths[0][3] != ""
    # the raw message lines carry the frame prefix
    text = node.L.fdsop_messages(node.node).decode()
    assert text.count("message\tframe ") == F and "message\tframe 4: Termination type: 1" in text
    node.close()


@pytest.fixture(scope="module")
def tps64(oracle, sphere):
    """33 frames of a thin-plate rig with 64 points, their oracle results on the sphere (shared, never written)."""
    P, _ = sphere
    rest = synth.control_points(64, "sphere")
    frames = _frames(rest, 33)
    refs = [_oracle_frame(oracle, fo.KERNEL_THIN_PLATE, [0.0], rest, d, P)[0] for d in frames]
    for r in refs:
        r.setflags(write=False)
    return rest, frames, refs


@pytest.mark.parametrize("F", [2, 17, 33])
def test_group_edges_thin_plate(hip_lib, sphere, tps64, F):
    P, _ = sphere
    rest, frames, refs = tps64
    node = FaceDeformSOP()
    node.set("kernel", 1)
    res = node.cook_shot(P, rest, frames[:F])
    assert res.severity == capi.FDSOP_WARNING            # no dist2: the reference's warning, once
    assert res.warnings == ["Can't find distance capture attribute. Won't apply radius nor falloff."]
    for k in range(F):
        _hold_fp32(res.frames[k].P, refs[k], P)
        assert np.array_equal(res.frames[k].fd_falloff, np.ones(P.shape[0], np.float32))
        assert res.frames[k].severity == capi.FDSOP_WARNING
    name = lambda n: capi.fd_shared_kernel_name(64, n, capi.KERNEL_THIN_PLATE)
    if F == 33:
        assert [(p[0], p[1]) for p in res.paths] == [(0, 32), (32, 1)]
        assert res.paths[0][3] == name(32) != "" and res.paths[0][4] == 32 and res.paths[1][4] == 1
    else:
        assert res.paths == [(0, F, "", name(F), F, "", 0)]
    node.close()


def test_sixteen_centres_take_the_batch_calls_own_fall_back(hip_lib, oracle, sphere):
    P, _ = sphere
    rest = synth.control_points(16, "sphere")
    frames = _frames(rest, 4)
    node = FaceDeformSOP()
    node.set("kernel", 1)
    res = node.cook_shot(P, rest, frames)
    assert not res.errors and res.paths == [(0, 4, "", "", 4, "", 0)]
    for k in range(4):
        ref, _ = _oracle_frame(oracle, fo.KERNEL_THIN_PLATE, [0.0], rest, frames[k], P)
        _hold_fp32(res.frames[k].P, ref, P)
    node.close()


def test_multilayer(hip_lib, oracle, sphere):
    P, _ = sphere
    M, L = 48, 4
    rest = synth.control_points(M, "sphere")
    frames = _frames(rest, 4)
    node = FaceDeformSOP()
    node.set("model", 1)
    res = node.cook_shot(P, rest, frames)
    assert not res.errors, (res.messages, [f.messages for f in res.frames])
    assert res.paths == [(0, 4, "", capi.fd_shared_ml_kernel_name(M, L, 4), 4, "", 0)] and res.paths[0][3] != ""
    for k in range(4):
        table = oracle.control_table(rest, frames[k])
        tt, table_ml, Wo, radii = oracle.build_multilayer(table, 1.0, L, 0.1, fo.TERM_LINEAR)
        assert tt == 1
        ref, _ = oracle.deform(table_ml, fo.KERNEL_GAUSSIAN_QNN, radii, Wo, P)
        _hold_fp32(res.frames[k].P, ref, P)
    # one frame is the cook, bit for bit
    one = node.cook_shot(P, rest, frames[:1])
    other = FaceDeformSOP()
    other.set("model", 1)
    ref1 = other.cook(P, rest, frames[0])
    assert np.array_equal(one.frames[0].P, ref1.P) and np.array_equal(one.frames[0].fd_falloff, ref1.fd_falloff)
    node.close(); other.close()


@pytest.mark.parametrize("kernel", [0, 1])
def test_one_frame_is_the_cook(hip_lib, sphere, kernel):
    P, dist2 = sphere
    rest = synth.control_points(32, "sphere")
    deform = synth.deformed_rig(rest)
    a, b = FaceDeformSOP(), FaceDeformSOP()
    for n in (a, b):
        n.set("kernel", kernel); n.set("radius", 0.7); n.set("falloffrate", 1.5)
    shot = a.cook_shot(P, rest, [deform], dist2=dist2)
    cook = b.cook(P, rest, deform, dist2=dist2)
    assert np.array_equal(shot.frames[0].P, cook.P) and np.array_equal(shot.frames[0].fd_falloff, cook.fd_falloff)
    assert shot.severity == cook.severity == shot.frames[0].severity
    assert shot.messages + shot.frames[0].messages == cook.messages
    assert np.array_equal(shot.frames[0].Cd, cook.Cd)
    assert shot.paths == [(0, 1, "", "", 1, "", 0)]
    a.close(); b.close()


@pytest.fixture(scope="module")
def mixed(oracle):
    """Four frames on ONE rest rig of which two need fp64 (tests/test_gpu_fp32_contract.py), and their oracle results."""
    rigs = [_rig(5, 100.0), _rig(19, 8.0), _rig(0, 1.0), _rig(19, 32.0)]
    rest = rigs[0][0]
    assert all(np.array_equal(r[0], rest) for r in rigs)
    P = _mesh()
    frames = [r[2] for r in rigs]
    refs = [_oracle_frame(oracle, fo.KERNEL_THIN_PLATE, [], rest, d, P)[0] for d in frames]
    holds = []
    for r in rigs:
        e = capi.Engine()
        e.set_kernel(capi.KERNEL_THIN_PLATE); e.set_term(capi.TERM_LINEAR); e.set_points(rest, r[1])
        holds.append(e.fp32_holds(e.build(), 1e-5))
        e.close()
    assert holds == [True, False, True, False]
    return P, rest, frames, refs, holds


def test_mixed_precision_is_decided_per_frame(hip_lib, mixed):
    P, rest, frames, refs, holds = mixed
    node = FaceDeformSOP()
    node.set("kernel", 1)
    res = node.cook_shot(P, rest, frames)
    assert not res.errors, res.messages
    for k in range(4):
        if holds[k]:
            assert l2_parity_ulp(res.frames[k].P, refs[k], P, TOL) <= 1.0
        else:
            assert l2_parity(res.frames[k].P, refs[k], P) <= TOL
    warned = [(k, w) for k, fr in enumerate(res.frames) for w in fr.warnings if "evaluating in fp64" in w]
    assert len(warned) == 1 and warned[0][0] == 1, warned
    assert not [w for w in res.warnings if "fp64" in w]
    assert len(res.paths) == 1 and res.paths[0][4] == 2 and res.paths[0][6] == 2
    fp32_frames = [res.frames[k].P.copy() for k in (0, 2)]
    # precision = 2: fp32 whatever the estimate says
    node.set("precision", 2)
    res2 = node.cook_shot(P, rest, frames)
    assert not [w for fr in res2.frames for w in fr.warnings if "fp64" in w] and res2.paths[0][6] == 0 and res2.paths[0][4] == 4
    # an fp32 frame's bits do not depend on which of its neighbours needed fp64
    assert np.array_equal(res2.frames[0].P, fp32_frames[0]) and np.array_equal(res2.frames[2].P, fp32_frames[1])
    assert l2_parity(res2.frames[1].P, refs[1], P) > TOL          # (what the default protects against)
    # precision = 1: every frame in fp64, one launch
    node.set("precision", 1)
    res3 = node.cook_shot(P, rest, frames)
    assert res3.paths[0][4] == 0 and res3.paths[0][6] == 4
    assert res3.paths[0][5] == capi.fd_shared_fp64_kernel_name(256, 4, capi.KERNEL_THIN_PLATE) != ""
    for k in range(4):
        assert l2_parity(res3.frames[k].P, refs[k], P) <= TOL
    node.close()


def test_tangent_projection_and_device_capture(hip_lib, oracle):
    from test_gpu_capture import _knn_adjacency, _rig_triangles
    N, M, K, F = 30_000, 40, 6, 3
    P = synth.head_mesh(N)
    rest = synth.control_points(M, "head")
    frames = _frames(rest, F, first=1)
    offsets, nb = _knn_adjacency(P)
    tris = _rig_triangles(rest)
    tu, tv, nn = synth.tangent_frames(P)
    kw = dict(edge_offsets=offsets, edge_neighbours=nb, rig_tris=tris, want_dist2=True, tangentu=tu, tangentv=tv, N=nn)

    def make():
        node = FaceDeformSOP()
        node.set("kernel", 1); node.set("tangent", 1)
        node.set("radius", 0.2); node.set("maxedges", K); node.set("dofalloff", 1); node.set("falloffrate", 1.5)
        return node

    node, single = make(), make()
    res = node.cook_shot(P, rest, frames, **kw)
    assert res.severity == capi.FDSOP_MESSAGE, (res.messages, [f.messages for f in res.frames])
    cooked = single.cook(P, rest, frames[0], **kw)
    got = res.frames[0].dist2
    assert np.array_equal(got, cooked.dist2)                      # produced once, the cook's
    assert all(fr.dist2 is None for fr in res.frames[1:])
    r2 = np.float32(0.2) * np.float32(0.2)
    for k in range(F):
        table = oracle.control_table(rest, frames[k])
        rc, tt, W, radii = oracle.build(table, fo.KERNEL_THIN_PLATE, [0.0], 0)
        ref, ref_fall = oracle.deform(table, fo.KERNEL_THIN_PLATE, radii, W, P, dist2=got, tangents=(tu, tv, nn), radius2=r2, falloffrate=1.5)
        plain, _ = oracle.deform(table, fo.KERNEL_THIN_PLATE, radii, W, P, dist2=got, radius2=r2, falloffrate=1.5)
        # with the projection on, the bar stays relative to the unprojected RBF displacement
        assert parity_ratio(res.frames[k].P, ref, P, TOL, scale_out=plain) <= 1.0
        assert np.allclose(res.frames[k].fd_falloff, ref_fall, rtol=2e-6, atol=1e-7)
    node.close(); single.close()


def test_morph_space_applies_to_frame_zero_only(hip_lib, oracle):
    from test_gpu_morph import _disp_ratio
    rng = np.random.default_rng(9)
    N, M, S, F = 20_011, 48, 9, 3
    P = synth.head_mesh(N)
    rig_rest = synth.control_points(M, "head")
    frames = _frames(rig_rest, F, first=1)
    shapes = [(P + (0.08 * rng.normal(size=(N, 3)) * (rng.random((N, 1)) < 0.5)).astype(np.float32)).astype(np.float32)
              for _ in range(S)]
    node = FaceDeformSOP()
    node.set("kernel", 1); node.set("morphspace", 1); node.set("doclampweight", 1)
    node.set("weightrange", -0.01, 0); node.set("weightrange", 0.02, 1)
    node.set("dofalloff", 1); node.set("falloffradius", 0.25)
    res = node.cook_shot(P, rig_rest, frames, shapes=shapes, blends_changed=True)
    assert not res.errors, res.messages
    morph_warning = "Can't compute weights for morphspace deformation. Ingoring it."
    assert morph_warning not in res.warnings and morph_warning not in res.frames[0].warnings
    assert res.frames[0].weights.shape == (S,)
    # frame 0: the reference's sequence -- RBF deform, then DirectBSEdit on the deformed mesh with rest = incoming P
    plain = []
    for k in range(F):
        table = oracle.control_table(rig_rest, frames[k])
        rc, tt, W, radii = oracle.build(table, fo.KERNEL_THIN_PLATE, [0.0], 0)
        assert rc == 0 and tt == 1
        plain.append(oracle.deform(table, fo.KERNEL_THIN_PLATE, radii, W, P)[0])
    A = oracle.morph_shapes_matrix(P, shapes)
    QR, _ = oracle.morph_qr(A)
    w_ref = oracle.morph_weights(QR, plain[0], P)
    assert np.abs(res.frames[0].weights - w_ref).max() <= 2e-5 * max(1.0, np.abs(w_ref).max())
    ref0 = oracle.morph_displace(A, w_ref, plain[0], P, (-0.01, 0.02), True, 0.25)
    assert _disp_ratio(res.frames[0].P, ref0, P, 2e-5) <= 1.0
    # frames >= 1: the warning, and the plain RBF result
    for k in range(1, F):
        assert res.frames[k].warnings.count(morph_warning) == 1, res.frames[k].messages
        _hold_fp32(res.frames[k].P, plain[k], P)
    node.close()


def test_transport_of_normals_and_tangents(hip_lib, sphere):
    from test_gpu_vectors import _field, _inputs, _model, _normalise
    from test_gpu_vectors_shared import BAR_ABS, BAR_REL
    N, M, F = 3_001, 64, 3
    P = synth.head_mesh(20_000)[:: 20_000 // N][:N].copy()
    rest = synth.control_points(M, "head")
    frames = _frames(rest, F)
    tu, tv, nrm, Nv, dist2 = _inputs(P)
    radius = np.float32(0.6)
    r2 = radius * radius
    node = FaceDeformSOP()
    node.set("kernel", 1); node.set("radius", float(radius)); node.set("falloffrate", 1.7)
    res = node.cook_shot(P, rest, frames, dist2=dist2, N=Nv, tangentu=tu, tangentv=tv, transport=True)
    assert not res.errors, (res.messages, [f.messages for f in res.frames])
    live = ~(dist2 > r2)

    def hold(fr, k):
        g = ~live
        assert np.array_equal(fr.N[g], Nv[g]) and np.array_equal(fr.tangentu[g], tu[g]) and np.array_equal(fr.tangentv[g], tv[g])
        e = capi.Engine()
        e.set_points(rest, (frames[k] - rest).astype(np.float32)); e.set_kernel(capi.KERNEL_THIN_PLATE, []); e.set_term(capi.TERM_LINEAR)
        e.build()
        centres, Wr, aff, radii = _model(e, capi.KERNEL_THIN_PLATE, rest)
        e.close()
        _, J, S = _field(capi.KERNEL_THIN_PLATE, P[live].astype(np.float64), centres, Wr, aff, radii)
        f = fr.fd_falloff[live].astype(np.float64)
        Aref = np.eye(3)[None] + f[:, None, None] * J
        bar = BAR_REL * np.linalg.norm(Aref, axis=(1, 2)) + BAR_ABS * f * S
        for t, to in ((tu[live], fr.tangentu[live]), (tv[live], fr.tangentv[live])):
            t64 = t.astype(np.float64)
            want = np.einsum("bij,bj->bi", Aref, t64)
            tb = bar * np.linalg.norm(t64, axis=1) + 2.0 ** -23 * np.linalg.norm(want, axis=1)
            assert (np.linalg.norm(to - want, axis=1) / tb).max() <= 1.0
        n64 = Nv[live].astype(np.float64)
        cof = np.stack([np.cross(Aref[:, :, 1], Aref[:, :, 2]), np.cross(Aref[:, :, 2], Aref[:, :, 0]),
                        np.cross(Aref[:, :, 0], Aref[:, :, 1])], axis=2)
        m = np.einsum("bij,bj->bi", cof, n64)
        nn = np.linalg.norm(n64, axis=1)
        want = _normalise(m) * nn[:, None]
        nb = 4.0 * np.linalg.norm(Aref, axis=(1, 2)) * bar * nn ** 2 / np.linalg.norm(m, axis=1) + 2.0 ** -22 * nn
        assert (np.linalg.norm(fr.N[live] - want, axis=1) / nb).max() <= 1.0

    for k in range(F):
        hold(res.frames[k], k)
    # one frame with transport: the cook's positions bit for bit, the vectors from the engine's own model
    one = node.cook_shot(P, rest, frames[:1], dist2=dist2, N=Nv, tangentu=tu, tangentv=tv, transport=True)
    other = FaceDeformSOP()
    other.set("kernel", 1); other.set("radius", float(radius)); other.set("falloffrate", 1.7)
    cooked = other.cook(P, rest, frames[0], dist2=dist2)
    assert np.array_equal(one.frames[0].P, cooked.P) and np.array_equal(one.frames[0].fd_falloff, cooked.fd_falloff)
    hold(one.frames[0], 0)
    other.close()
    # the positions are those of the shot without transport
    res_plain = node.cook_shot(P, rest, frames, dist2=dist2, N=Nv, tangentu=tu, tangentv=tv)
    for k in range(F):
        assert np.array_equal(res_plain.frames[k].P, res.frames[k].P)
        assert res_plain.frames[k].N is None and res_plain.frames[k].tangentu is None    # NULL tables: nothing is written
    node.close()


def test_errors_and_node_state(hip_lib, oracle, sphere):
    P, _ = sphere
    rest = synth.control_points(32, "sphere")
    frames = _frames(rest, 3)
    node = FaceDeformSOP()
    # a rest rig with a duplicated point: every frame reports as its own cook does
    bad = rest.copy(); bad[4] = bad[0]
    res = node.cook_shot(P, bad, frames)
    assert res.severity == capi.FDSOP_ERROR
    for fr in res.frames:
        assert fr.errors == ["Can't solve the problem."] and np.array_equal(fr.P, P) and fr.severity == capi.FDSOP_ERROR
    # a good shot, page-locked and pageable outputs: equal bits
    pinned = [capi.host_array((P.shape[0], 3)) for _ in range(3)]
    pinned_fall = [capi.host_array((P.shape[0],)) for _ in range(3)]
    good = node.cook_shot(P, rest, frames, out_P=pinned, out_falloff=pinned_fall)
    assert not good.errors, good.messages
    pageable = node.cook_shot(P, rest, frames, rig_rest_unchanged=True, mesh_unchanged=True)
    for k in range(3):
        assert good.frames[k].P is pinned[k]
        assert np.array_equal(pageable.frames[k].P, pinned[k]) and np.array_equal(pageable.frames[k].fd_falloff, pinned_fall[k])
        ref, _ = _oracle_frame(oracle, fo.KERNEL_GAUSSIAN_QNN, [1.0, 5.0, 0.0], rest, frames[k], P)
        _hold_fp32(pinned[k], ref, P)
    # the node afterwards: a cook that vouches for rig and mesh holds the oracle
    nxt = synth.deformed_rig(rest, 7)
    after = node.cook(P, rest, nxt, rig_rest_unchanged=True, mesh_unchanged=True)
    assert not after.errors, after.messages
    ref, _ = _oracle_frame(oracle, fo.KERNEL_GAUSSIAN_QNN, [1.0, 5.0, 0.0], rest, nxt, P)
    _hold_fp32(after.P, ref, P)
    node.close()
