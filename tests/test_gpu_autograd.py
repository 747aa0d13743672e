"""GPU: facedeform_amd.autograd.deform -- the deformation as a torch.autograd.Function over the device-pointer calls.

513 vertices, 33 control points, thin-plate and QNN, projection and gate on; the engine evaluates in fp64.

The bars:
  deltas     the map is linear in the deltas, so no step size: |<grad_delta, d'> - sum_v g . (D(d + d') - D(d))| <=
             2e-7 sum_v |g_v|_2 |D_v(d + d')|_2, the project's bar for an fp64 displacement stored as fp32
             (tests/test_gpu_adjoint.py).  d and d' are multiples of 2^-12, so d + d' is exact in fp32.
  positions  tests/test_gpu_adjoint_points.py's dual identity through the Function:
             |sum_v P.grad . t - sum_v g . tu_out| <= 2e-7 sum_v |g_v|_2 |tu_out_v|_2, tu_out fd_deform_vectors' transport of t."""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
N, M = 513, 33
RADIUS2, RATE = 0.36, 1.7
KINDS = {"thin_plate": (capi.KERNEL_THIN_PLATE, []), "qnn": (capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])}


def _grid(a):
    """Rounded to multiples of 2^-12: sums of two such arrays of this size are exact in fp32."""
    return (np.round(np.asarray(a, np.float64) * 4096) / 4096).astype(np.float32)


def _setup(kind_name):
    from facedeform_amd import autograd
    dev = torch.device("cuda", 0)
    P = synth.head_mesh(3000)[::5][:N].copy()
    assert P.shape[0] == N
    tu, tv, nrm = synth.tangent_frames(P)
    rng = np.random.default_rng(7)
    dist2 = (rng.random(N) * 1.5 * RADIUS2).astype(np.float32)
    dist2[::97] = np.float32(RADIUS2)
    G = rng.standard_normal((N, 3)).astype(np.float32)
    t = rng.standard_normal((N, 3)).astype(np.float32)
    rest = synth.control_points(M)
    delta = _grid(synth.rig_deltas(rest, 0))
    delta2 = _grid(0.05 * rng.standard_normal((M, 3)))
    kind, params = KINDS[kind_name]
    e = capi.Engine(device=0)
    e.set_points(rest, delta); e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
    e.build()
    e.set_eval_precision(capi.EVAL_FP64)
    host = dict(P=P, tu=tu, tv=tv, nrm=nrm, dist2=dist2, G=G, t=t, delta=delta, delta2=delta2)
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    kw = dict(dist2=d["dist2"], tangents=(d["tu"], d["tv"], d["nrm"]), radius2=RADIUS2, falloffrate=RATE)
    return autograd, e, host, d, kw


@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_gradient_for_the_deltas(hip_lib, kind_name):
    autograd, e, host, d, kw = _setup(kind_name)
    S = autograd.solve_operator_tensor(e)
    assert S.dtype == torch.float64 and S.is_cuda and S.shape[1] == M
    delta = d["delta"].clone().requires_grad_(True)
    out = autograd.deform(e, d["P"], delta, S=S, displacement=True, **kw)
    (out * d["G"]).sum().backward()
    assert delta.grad is not None and delta.grad.dtype == torch.float32 and delta.grad.shape == (M, 3)
    D0 = out.detach().cpu().numpy().astype(np.float64)
    with torch.no_grad():
        D1 = autograd.deform(e, d["P"], d["delta"] + d["delta2"], displacement=True, **kw).cpu().numpy().astype(np.float64)
    e.close()
    assert np.array_equal((d["delta"] + d["delta2"]).cpu().numpy().astype(np.float64),
                          host["delta"].astype(np.float64) + host["delta2"].astype(np.float64))
    G = host["G"].astype(np.float64)
    lhs = float((delta.grad.cpu().numpy().astype(LD) * host["delta2"].astype(LD)).sum())
    rhs = float((G.astype(LD) * (D1.astype(LD) - D0.astype(LD))).sum())
    bar = 2e-7 * float((np.linalg.norm(G, axis=1) * np.linalg.norm(D1, axis=1)).sum())
    print(f"deltas {kind_name}: <grad_delta, d'> = {lhs:.12e}, sum g.(D(d + d') - D(d)) = {rhs:.12e}, |diff| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert bar > 0 and abs(rhs) > 100 * bar and abs(lhs - rhs) <= bar


@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_gradient_for_the_positions(hip_lib, kind_name):
    autograd, e, host, d, kw = _setup(kind_name)
    P = d["P"].clone().requires_grad_(True)
    out = autograd.deform(e, P, **kw)
    (out * d["G"]).sum().backward()
    assert P.grad is not None and P.grad.dtype == torch.float32 and P.grad.shape == (N, 3)
    grad_pos = P.grad.clone()
    # the forward is fd_deform
    ref_out, _ = e.deform(host["P"], dist2=host["dist2"], tangents=(host["tu"], host["tv"], host["nrm"]), radius2=RADIUS2, falloffrate=RATE)
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), ref_out.view(np.uint32))
    res = e.deform_vectors(host["P"], dist2=host["dist2"], tangents=(host["tu"], host["tv"], host["nrm"]), tu=host["t"],
                           radius2=RADIUS2, falloffrate=RATE)
    tu_out = res[3].astype(np.float64)
    G = host["G"].astype(np.float64)
    lhs = float((grad_pos.cpu().numpy().astype(LD) * host["t"].astype(LD)).sum())
    rhs = float((G.astype(LD) * tu_out.astype(LD)).sum())
    bar = 2e-7 * float((np.linalg.norm(G, axis=1) * np.linalg.norm(tu_out, axis=1)).sum())
    print(f"positions {kind_name}: sum P.grad . t = {lhs:.12e}, sum g.(A t) = {rhs:.12e}, |diff| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert bar > 0 and abs(lhs - rhs) <= bar

    # displacement=True: the position gradient minus g, formed in fp64 before the cast
    P2 = d["P"].clone().requires_grad_(True)
    out2 = autograd.deform(e, P2, displacement=True, **kw)
    (out2 * d["G"]).sum().backward()
    gp = torch.empty((N, 3), dtype=torch.float64, device=P2.device)
    torch.cuda.synchronize()
    e.deform_adjoint_points_dev(N, d["P"].data_ptr(), d["G"].data_ptr(), gp.data_ptr(), d_dist2=d["dist2"].data_ptr(),
                                d_tu=d["tu"].data_ptr(), d_tv=d["tv"].data_ptr(), d_nrm=d["nrm"].data_ptr(), radius2=RADIUS2,
                                falloffrate=RATE)
    e.synchronize()
    assert torch.equal(grad_pos, gp.to(torch.float32))
    assert torch.equal(P2.grad, (gp - d["G"].to(torch.float64)).to(torch.float32))
    # ... which differs from the rounded position gradient minus g by that rounding alone
    assert (P2.grad - (grad_pos - d["G"])).abs().max().item() <= 2.0 ** -23 * (grad_pos.abs().max().item() + d["G"].abs().max().item())
    e.close()


def test_errors(hip_lib):
    autograd, e, host, d, kw = _setup("thin_plate")
    # a delta that requires grad needs S
    delta = d["delta"].clone().requires_grad_(True)
    with pytest.raises(ValueError):
        autograd.deform(e, d["P"], delta, **kw)
    # inputs must be contiguous float32 CUDA tensors
    with pytest.raises(ValueError):
        autograd.deform(e, d["P"].cpu(), **kw)
    with pytest.raises(ValueError):
        autograd.deform(e, d["P"].double(), **kw)
    # a backward whose model a later forward has replaced
    P1 = d["P"].clone().requires_grad_(True)
    out1 = autograd.deform(e, P1, **kw)
    P2 = d["P"].clone().requires_grad_(True)
    out2 = autograd.deform(e, P2, **kw)
    with pytest.raises(RuntimeError, match="replaced"):
        out1.sum().backward()
    out2.sum().backward()                      # the latest forward's backward goes through
    assert P2.grad is not None and P1.grad is None
    e.close()
