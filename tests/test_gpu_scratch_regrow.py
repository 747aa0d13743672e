"""GPU: every device buffer of the host layer that grows by need (facedeform_amd/csrc/fd_owned.h: DevBuf::grow, and the buffers
that one capacity governs), through every grow path the C ABI can reach.  Each case makes calls on ONE handle -- a small call, a
larger one, which makes the scratch grow, and the small one again, which reuses the larger buffer -- and compares every result
bit for bit with what a fresh handle gives for the same call.  Equality only: there is no tolerance here, and no allocation is
made to fail.

Sizes: rigs of 32 and 96 points; meshes of 64 and 4160 vertices (one past a 64-vertex group); batches of as few frames as the
launch in question accepts, which the fd_shared_*_kernel_name queries say."""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from facedeform_amd.sop import FaceDeformSOP
from test_gpu_shared_ml import DEV, RADIUS2, RATE, Outs, _close, _deltas, _dist2, _engines, _mesh

pytestmark = pytest.mark.gpu

MS, NS = (32, 96), (64, 4160)
STEPS = (0, 1, 0)                       # small, larger, small again
LAYERS = 3
TPS, QNN, ML = capi.KERNEL_THIN_PLATE, capi.KERNEL_GAUSSIAN_QNN, capi.KERNEL_GAUSSIAN_ML
ML_PARAMS = [0.7, LAYERS, 0.1]


def _unit(rng, n):
    v = rng.standard_normal((n, 3)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def data():
    """Per size index: the rig (rest, 32 frames of deltas) and the mesh with its attributes.  Shared, never written."""
    rng = np.random.default_rng(11)
    rigs, meshes = [], []
    for M in MS:
        rest = synth.control_points(M, "head")
        rigs.append((rest, _deltas(rest, 32)))
    for N in NS:
        m = {"P": _mesh(N), "d2": _dist2(N), "frames": (_unit(rng, N), _unit(rng, N), _unit(rng, N)), "Nv": _unit(rng, N),
             "G": rng.standard_normal((3, N, 3)).astype(np.float32), "omega": rng.random(N).astype(np.float32)}
        meshes.append(m)
    for a in [x for r in rigs for x in r] + [v for m in meshes for v in m.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return rigs, meshes


def _flat(x):
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _flat(y)]
    return [] if x is None else [np.asarray(x)]


def _same(got, want, where):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want) and len(got) > 0, where
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (where, k)


def _walk(make, run, shut, steps=STEPS):
    """run(handle, i) on one handle for every size index i of `steps`, each result against a fresh handle's for that index."""
    want = {}
    for i in sorted(set(steps)):
        h = make()
        want[i] = run(h, i)
        shut(h)
    assert _flat(want[0])[0].tobytes() != _flat(want[1])[0].tobytes()       # the two calls do differ
    h = make()
    for n, i in enumerate(steps):
        _same(run(h, i), want[i], (n, i))
    shut(h)


def _frames_min(*names):
    """The fewest frames at which every name query gives a kernel at both rig sizes: names are functions of (M, F)."""
    return next(F for F in range(1, 33) if all(name(M, F) != "" for name in names for M in MS))


# ---- one context ----------------------------------------------------------------------------------------------------------------
def _built_engine(data, i=0, kind=TPS, params=()):
    rest, deltas = data[0][i]
    e = capi.Engine()
    e.set_kernel(kind, params)
    e.set_points(rest, deltas[0])
    assert e.build().terminationtype == 1
    return e


@pytest.mark.parametrize("kind", [TPS, QNN])
def test_model_records_and_solver_capacity(hip_lib, data, kind):
    """fd_set_points, then fd_build: cap_M, cap_records and cap_npad at 32, 96 and 32 points"""
    mesh = data[1][0]

    def make():
        e = capi.Engine()
        e.set_kernel(kind)
        return e

    def run(e, i):
        rest, deltas = data[0][i]
        e.set_points(rest, deltas[1])
        assert e.build().terminationtype == 1
        return e.get_weights(), e.deform(mesh["P"], dist2=mesh["d2"], radius2=RADIUS2, falloffrate=RATE)
    _walk(make, run, lambda e: e.close())


def test_host_staging_releases_the_frames_and_allocates_them_again(hip_lib, data):
    """ensure_staging: with tangent frames at the small mesh, without them at the larger one (the capacity grows and the three
    frame buffers go), then with them again (allocated at the capacity that governs)"""
    def run(e, i):
        m = data[1][i]
        return e.deform(m["P"], dist2=m["d2"], tangents=m["frames"] if i == 0 else None, radius2=RADIUS2, falloffrate=RATE)
    _walk(lambda: _built_engine(data), run, lambda e: e.close())
    # and the larger mesh with frames on a context that has staged it without them
    e, fresh = _built_engine(data), _built_engine(data)
    m = data[1][1]
    e.deform(m["P"], dist2=m["d2"])
    kw = dict(dist2=m["d2"], tangents=m["frames"], radius2=RADIUS2, falloffrate=RATE)
    _same(e.deform(m["P"], **kw), fresh.deform(m["P"], **kw), "frames at the larger mesh")
    e.close(); fresh.close()


OPS = {
    "vectors": lambda e, m: e.deform_vectors(m["P"], dist2=m["d2"], tangents=m["frames"], N=m["Nv"], tu=m["frames"][0],
                                             want_jacobian=True, radius2=RADIUS2, falloffrate=RATE),             # d_vec
    "vectors_in_place": lambda e, m: e.deform_vectors(m["P"], dist2=m["d2"], N=m["Nv"], radius2=RADIUS2, falloffrate=RATE),
    "invert": lambda e, m: e.invert(m["P"], dist2=m["d2"], radius2=RADIUS2, falloffrate=RATE),                 # d_iters
    "adjoint": lambda e, m: e.deform_adjoint(m["P"], m["G"][0], dist2=m["d2"], radius2=RADIUS2, falloffrate=RATE),
    "adjoint_points": lambda e, m: e.deform_adjoint_points(m["P"], m["G"][0], dist2=m["d2"], tangents=m["frames"], radius2=RADIUS2,
                                                           falloffrate=RATE, want_grad_f=True),
    "gram": lambda e, m: e.deform_gram(m["P"], omega=m["omega"], dist2=m["d2"], radius2=RADIUS2, falloffrate=RATE),
    "gram_frames": lambda e, m: e.deform_gram(m["P"], dist2=m["d2"], tangents=m["frames"], radius2=RADIUS2, falloffrate=RATE),
    "adjoint_shot": lambda e, m: e.deform_adjoint_shot(m["P"], m["G"], dist2=m["d2"], radius2=RADIUS2, falloffrate=RATE),
}


@pytest.mark.parametrize("op", sorted(OPS))
def test_host_call_scratch(hip_lib, data, op):
    """the host calls' staging and scratch (d_vec, d_vecP, d_iters, d_adj, d_adjp, d_gram, d_adjs, d_gshot) at 64, 4160 and 64
    vertices"""
    _walk(lambda: _built_engine(data), lambda e, i: OPS[op](e, data[1][i]), lambda e: e.close())


# ---- the shot calls --------------------------------------------------------------------------------------------------------------
# family: kernel, parameters, position call, vector call, the name queries of both as functions of (M, F), the steps
SHOTS = {
    "fp32": (TPS, [], "deform_shared_dev", "deform_vectors_shared_dev",
             (lambda M, F: capi.fd_shared_kernel_name(M, F, TPS), lambda M, F: capi.fd_shared_vectors_kernel_name(M, F, TPS)),
             (0, 1, 1, 0, 0)),           # two sets that take turns: each grows once, each is reused once
    "fp64": (TPS, [], "deform_shared_fp64_dev", "deform_vectors_shared_fp64_dev",
             (lambda M, F: capi.fd_shared_fp64_kernel_name(M, F, TPS), lambda M, F: capi.fd_shared_vectors_fp64_kernel_name(M, F, TPS)),
             STEPS),
    "ml": (ML, ML_PARAMS, "deform_shared_ml_dev", "deform_vectors_shared_ml_dev",
           (lambda M, F: capi.fd_shared_ml_kernel_name(M, LAYERS, F), lambda M, F: capi.fd_shared_vectors_ml_kernel_name(M, LAYERS, F)),
           STEPS),
    "ml_fp64": (ML, ML_PARAMS, "deform_shared_ml_fp64_dev", "deform_vectors_shared_ml_fp64_dev",
                (lambda M, F: capi.fd_shared_ml_fp64_kernel_name(M, LAYERS, F),
                 lambda M, F: capi.fd_shared_vectors_ml_fp64_kernel_name(M, LAYERS, F)), STEPS),
}


class _Shot:
    """A batch of F contexts on a stream of its own, rebuilt at another rig size behind fd_batch_wait_consumed"""
    def __init__(self, data, kind, params, F):
        self.data, self.F, self.keep, self.M = data, F, {}, None
        self.S = torch.cuda.Stream(device=DEV())
        rest, deltas = data[0][0]
        self.engines, self.batch, _ = _engines(MS[0], LAYERS, F, np.array(rest), np.array(deltas[:F]), kind=kind, params=params, stream=self.S.cuda_stream,
                                               build=False)
        self.dev = [{k: torch.from_numpy(np.array(m[k])).to(DEV()) for k in ("P", "d2", "Nv")} for m in data[1]]

    def build(self, i, before=None):
        M, F = MS[i], self.F
        if i not in self.keep:
            rest, deltas = self.data[0][i]
            self.keep[i] = (torch.from_numpy(np.array(rest)).to(DEV()), torch.from_numpy(np.array(deltas[:F])).to(DEV()))
        if self.M is not None:
            self.batch.wait_consumed(self.S.cuda_stream)
        d_rest, d_del = self.keep[i]
        self.batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
        if before:
            before(self.batch)
        self.batch.build_async(self.S.cuda_stream)
        assert [r.terminationtype for r in self.batch.build_result()] == [1] * F
        self.M = M

    def call(self, which, i, vectors):
        N, d, F = NS[i], self.dev[i], self.F
        outs = Outs(N, F)
        po, fo_ = outs.ptrs()
        kw = dict(d_dist2=d["d2"].data_ptr(), d_falloff=fo_, radius2=RADIUS2, falloffrate=RATE, stream_ptr=self.S.cuda_stream)
        extra = []
        if vectors:
            No = [torch.zeros((N, 3), device=DEV()) for _ in range(F)]
            A = [torch.zeros((N, 9), device=DEV()) for _ in range(F)]
            torch.cuda.synchronize()
            kw.update(d_N=d["Nv"].data_ptr(), d_N_out=[t.data_ptr() for t in No], d_jacobian=[t.data_ptr() for t in A])
            extra = No + A
        getattr(self.batch, which)(N, d["P"].data_ptr(), po, **kw)
        torch.cuda.synchronize()
        return outs.host(), [t.cpu().numpy() for t in extra]

    def close(self):
        _close(self.engines, self.batch)


@pytest.mark.parametrize("vectors", [False, True], ids=["positions", "vectors"])
@pytest.mark.parametrize("family", sorted(SHOTS))
def test_shot_call_scratch(hip_lib, data, family, vectors):
    """the four shot position calls and their vector calls: the two SharedSets, s64, sml and sml64 under rigs of 32, 96 and 32
    points, the one-launch path at every step"""
    kind, params, pos, vec, names, steps = SHOTS[family]
    F = _frames_min(*names)

    def run(h, i):
        h.build(i)
        return h.call(vec if vectors else pos, i, vectors)
    _walk(lambda: _Shot(data, kind, params, F), run, lambda h: h.close(), steps)


BUILDS = {
    "multilayer": (ML, ML_PARAMS, "set_shared_factor", lambda M, F: capi.fd_shared_ml_build_kernel_name(M, LAYERS, F), STEPS),
    # the second small build finds the scratch slot ready; the growth resets it, and the small build behind it fills it again
    "qnn": (QNN, [], "set_shared_lu", lambda M, F: capi.fd_shared_qnn_build_kernel_name(M, F), (0, 0, 1, 0, 0)),
}


@pytest.mark.parametrize("model", sorted(BUILDS))
def test_shared_build_scratch(hip_lib, data, model):
    """a batched multilayer build with the shared factor on (d_mlfac) and a batched QNN build with the shared LU on (d_qnnfac and
    the qnn_slot_ready reset on growth)"""
    kind, params, switch, name, steps = BUILDS[model]
    F = _frames_min(name)

    def run(h, i):
        h.build(i, before=lambda b: getattr(b, switch)(True))
        assert h.batch.last_build_shared_factor()
        return [e.get_weights() for e in h.engines]
    _walk(lambda: _Shot(data, kind, params, F), run, lambda h: h.close(), steps)


# ---- the node's shot cook, the morph space ---------------------------------------------------------------------------------------
def test_cook_shot_staging(hip_lib, data):
    """fd_shot_dev_set_rig, _set_vectors and _reserve through fdsop_cook_shot: rig, mesh and frame count grow together"""
    F = max(2, _frames_min(lambda M, F: capi.fd_shared_kernel_name(M, F, TPS)))
    counts = (F, F + 2)

    def make():
        node = FaceDeformSOP()
        node.set("kernel", 1)
        return node

    def run(node, i):
        (rest, deltas), m = data[0][i], data[1][i]
        res = node.cook_shot(m["P"], rest, [rest + deltas[k] for k in range(counts[i])], dist2=m["d2"], N=m["Nv"], transport=True)
        assert not res.errors, (res.messages, [f.messages for f in res.frames])
        assert [p[3] != "" for p in res.paths] == [True], res.paths          # one group, the one-launch path
        return [(f.P, f.fd_falloff, f.N) for f in res.frames]
    _walk(make, run, lambda node: node.close())


def test_morph_space(hip_lib, data):
    """one fd_morph set up at two sizes: fd_morph_init's buffers, and the batched weights' (d_bw, d_bwpartial)"""
    rng = np.random.default_rng(5)
    shapes = [[(m["P"] + 0.05 * rng.standard_normal(m["P"].shape)).astype(np.float32) for _ in range(S)] for m, S in zip(data[1], (3, 9))]
    poses = [np.stack([(m["P"] + 0.02 * rng.standard_normal(m["P"].shape)).astype(np.float32) for _ in range(2)]) for m in data[1]]

    def run(mo, i):
        mo.init(data[1][i]["P"], shapes[i])
        single = mo.apply(poses[i][0], clamp=(-1.0, 1.0))
        d = [torch.from_numpy(p).to(DEV()) for p in poses[i]]
        ptrs = [t.data_ptr() for t in d]
        mo.compute_weights_batch_dev(ptrs)
        w = mo.weights_batch()
        mo.displace_batch_dev(ptrs, clamp=(-1.0, 1.0))
        torch.cuda.synchronize()
        return single, w, [t.cpu().numpy() for t in d], mo.qr()
    _walk(capi.Morph, run, lambda mo: mo.close())
