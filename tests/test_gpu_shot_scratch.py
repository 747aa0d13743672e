"""GPU: the scratch a batch keeps for its one-launch shot calls (fd_batch_deform_vectors_shared_fp64_dev, _ml_dev and
_ml_fp64_dev, each with a scratch of its own) when the rig changes size under it: the same batch, stream and output tensors
at M = 33, then at M = 96 (the scratch is freed and allocated again), then at M = 33 again behind fd_batch_wait_consumed (the
scratch is larger than needed; the pack kernel waits for the evaluation that last read it).  After every call positions,
fall-off, normals and Jacobian are, bit for bit, those of a fresh batch built directly at that size -- the bar that
test_same_bits_on_every_call_* sets for these launches."""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_shared_ml import DEV, RADIUS2, RATE, SENTINEL, Outs, _close, _deltas, _dist2, _engines, _mesh

pytestmark = pytest.mark.gpu

N, F, LAYERS = 1025, 3, 3
SIZES = (33, 96, 33)
ML = capi.KERNEL_GAUSSIAN_ML
# family: kernel, its parameters, the vector call, the names of the position and of the vector launch at (M, F)
FAMILIES = {
    "fp64": (capi.KERNEL_THIN_PLATE, [], "deform_vectors_shared_fp64_dev",
             lambda M: (capi.fd_shared_fp64_kernel_name(M, F, capi.KERNEL_THIN_PLATE),
                        capi.fd_shared_vectors_fp64_kernel_name(M, F, capi.KERNEL_THIN_PLATE))),
    "ml": (ML, [0.7, LAYERS, 0.1], "deform_vectors_shared_ml_dev",
           lambda M: (capi.fd_shared_ml_kernel_name(M, LAYERS, F), capi.fd_shared_vectors_ml_kernel_name(M, LAYERS, F))),
    "ml_fp64": (ML, [0.7, LAYERS, 0.1], "deform_vectors_shared_ml_fp64_dev",
                lambda M: (capi.fd_shared_ml_fp64_kernel_name(M, LAYERS, F), capi.fd_shared_vectors_ml_fp64_kernel_name(M, LAYERS, F))),
}


class VecOuts(Outs):
    """test_gpu_shared_ml's outputs plus the transported normals and the Jacobian, with the same canary tail."""
    def __init__(self, N, F):
        super().__init__(N, F)
        self.No = [torch.full((N + 64, 3), SENTINEL, device=DEV()) for _ in range(F)]
        self.A = [torch.full((N + 64, 9), SENTINEL, device=DEV()) for _ in range(F)]
        torch.cuda.synchronize()

    def host(self):
        P, fall = super().host()
        No = [t.cpu().numpy() for t in self.No]; A = [t.cpu().numpy() for t in self.A]
        for n, a in zip(No, A):
            assert (n[self.N:] == np.float32(SENTINEL)).all() and (a[self.N:] == np.float32(SENTINEL)).all()
        return P, fall, [n[:self.N] for n in No], [a[:self.N] for a in A]


def _vectors(batch, which, d, outs, stream):
    po, fo_ = outs.ptrs()
    getattr(batch, which)(N, d["P"].data_ptr(), po, d_dist2=d["d2"].data_ptr(), d_falloff=fo_, d_N=d["Nv"].data_ptr(),
                          d_N_out=[t.data_ptr() for t in outs.No], d_jacobian=[t.data_ptr() for t in outs.A],
                          radius2=RADIUS2, falloffrate=RATE, stream_ptr=stream)
    torch.cuda.synchronize()
    return outs.host()


def _rebuild(batch, keep, M, stream):
    d_rest, d_del = keep
    batch.set_points_dev([d_rest.data_ptr()] * F, [d_del.data_ptr() + f * M * 12 for f in range(F)], M)
    batch.build_async(stream)
    assert [r.terminationtype for r in batch.build_result()] == [1] * F


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_scratch_grows_and_is_reused_under_one_batch(hip_lib, family):
    kind, params, which, names = FAMILIES[family]
    for M in set(SIZES):
        assert all(names(M)), (family, M)                      # the one-launch path of both launches, at both sizes
    rng = np.random.default_rng(7)
    Nv = rng.standard_normal((N, 3)).astype(np.float32)
    Nv /= np.linalg.norm(Nv, axis=1, keepdims=True)
    d = {"P": torch.from_numpy(_mesh(N)).to(DEV()), "d2": torch.from_numpy(_dist2(N)).to(DEV()), "Nv": torch.from_numpy(Nv).to(DEV())}
    rigs = {M: synth.control_points(M, "head") for M in set(SIZES)}
    rigs = {M: (rest, _deltas(rest, F)) for M, rest in rigs.items()}
    S = torch.cuda.Stream(device=DEV())
    stream = S.cuda_stream

    # a fresh batch at each size: the bits every call of the one batch below must reproduce
    want = {}
    for M, (rest, deltas) in rigs.items():
        engines, batch, keep = _engines(M, LAYERS, F, rest, deltas, kind=kind, params=params, stream=stream)
        want[M] = _vectors(batch, which, d, VecOuts(N, F), stream)
        _close(engines, batch)
    assert not np.array_equal(want[33][0][0], want[96][0][0])   # the two rigs do move the mesh differently
    assert not np.array_equal(want[33][3][0], want[96][3][0])

    rest, deltas = rigs[SIZES[0]]
    engines, batch, keep0 = _engines(SIZES[0], LAYERS, F, rest, deltas, kind=kind, params=params, stream=stream)
    keeps = {SIZES[0]: keep0}
    outs = VecOuts(N, F)
    for step, M in enumerate(SIZES):
        if step:
            if M not in keeps:
                keeps[M] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV()) for a in rigs[M])
            else:
                batch.wait_consumed(stream)                     # back to a smaller rig: rebuilt behind the last evaluation's copy
            _rebuild(batch, keeps[M], M, stream)
        got = _vectors(batch, which, d, outs, stream)
        for what, g, w in zip(("P", "falloff", "N", "jacobian"), got, want[M]):
            for f in range(F):
                assert np.array_equal(g[f], w[f]), (family, step, M, what, f)
    _close(engines, batch)
