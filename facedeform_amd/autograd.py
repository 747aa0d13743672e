"""The deformation as a differentiable torch operation: a thin torch.autograd.Function over the device-pointer calls of
capi.Engine.  No kernel of its own: the forward is fd_deform_dev, the backward fd_deform_adjoint_points_dev (the gradient for
the vertex positions) and fd_deform_adjoint_dev followed by grad_delta = S^T grad_W (the gradient for the rig's deltas).
deform_shot is the same for the F frames of a shot -- one mesh, one rest rig, F sets of deltas on a capi.Batch: the forward is
fd_batch_set_points_dev + fd_batch_build_async + fd_batch_deform_shared_fp64_dev (the fp64 launch, whatever the contexts'
precision setting says; its outputs are fp32), the backward fd_batch_deform_adjoint_points_shared_dev (grad_P = sum_f A_f^T
g_f) and fd_deform_adjoint_shot_dev on one of the batch's contexts followed by grad_delta[f] = S^T grad_W[f].

    S = solve_operator_tensor(engine)                      # once per rest rig
    out = deform(engine, P, delta, S=S, dist2=d2, tangents=(tu, tv, nrm), radius2=0.36, falloffrate=1.7)
    loss(out).backward()                                   # P.grad, delta.grad

    S = solve_operator_tensor(batch.engines[0])            # once per rest rig, after a first build
    out = deform_shot(batch, P, rest, deltas, S=S, ...)    # (F, N, 3); P.grad, deltas.grad

One model per engine.  The engine holds ONE solved model, and the backward reads it.  Every forward stamps a counter on the
engine; a backward whose stamp is no longer the engine's raises RuntimeError: another forward has replaced the model (or may
have) since, and its gradients would belong to the wrong deltas.  Run backward before the next forward on the same engine, or
use one engine per live graph.  deform_shot keeps the same stamp on the batch, whose contexts hold the F models.

Not differentiated: dist2 and the projection frames (per-point attributes, constants of the map) -- and through them radius2
and falloffrate; Engine.deform_adjoint_points(..., want_grad_f=True) returns the sensitivity for each vertex's fall-off value,
from which a caller forms those.  Nor the rest control points (deform_shot's `rest` included).
"""
from __future__ import annotations

import torch

from . import capi

__all__ = ["deform", "deform_shot", "solve_operator_tensor"]


def solve_operator_tensor(engine: capi.Engine, device=None) -> torch.Tensor:
    """fd_solve_operator's S, (C + 4, M), as a float64 CUDA tensor: W[:, a] = S @ delta[:, a] for the engine's rest rig."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return torch.from_numpy(engine.solve_operator()).to(device)


class _EngineStream:
    """The engine's calls ordered on torch's current stream.  A torch stream with a handle of its own is handed to
    fd_set_stream as it is.  Torch's default stream has the handle 0, which fd_set_stream reads as "the context's own stream",
    and that stream is not ordered with the default one: the engine then runs on a side stream that waits for torch's stream
    on entry and that torch's stream waits for on exit."""

    def __init__(self, engine, device):
        self.engine, self.cur = engine, torch.cuda.current_stream(device)
        self.side = None
        if self.cur.cuda_stream == 0:
            self.side = getattr(engine, "_autograd_stream", None)
            if self.side is None or self.side.device != self.cur.device:
                self.side = engine._autograd_stream = torch.cuda.Stream(device=device)

    def __enter__(self):
        if self.side is not None:
            self.side.wait_stream(self.cur)
        self.engine.set_stream((self.cur if self.side is None else self.side).cuda_stream)
        return self

    def __exit__(self, *exc):
        if self.side is not None:
            self.cur.wait_stream(self.side)
        return False


def _checked(name, t, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    return t


class _Deform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, delta, S, engine, dist2, frames, radius2, falloffrate, displacement):
        n = P.shape[0]
        out = torch.empty_like(P)
        ptrs = dict(d_dist2=dist2.data_ptr() if dist2 is not None else 0)
        if frames is not None:
            ptrs.update(d_tu=frames[0].data_ptr(), d_tv=frames[1].data_ptr(), d_nrm=frames[2].data_ptr())
        with _EngineStream(engine, P.device):
            engine.set_output(capi.OUTPUT_DISPLACEMENT if displacement else capi.OUTPUT_POSITION)
            if delta is not None:
                engine.set_deltas_dev(delta.data_ptr(), delta.shape[0])
                engine.build_async()
            engine.deform_dev(n, P.data_ptr(), out.data_ptr(), radius2=radius2, falloffrate=falloffrate, **ptrs)
        engine._autograd_stamp = getattr(engine, "_autograd_stamp", 0) + 1
        ctx.engine, ctx.stamp, ctx.ptrs = engine, engine._autograd_stamp, ptrs
        ctx.gate = (radius2, falloffrate)
        ctx.displacement = displacement
        ctx.has_delta = delta is not None
        ctx.keep = (dist2, frames)                      # the attribute arrays stay alive until backward has read them
        ctx.save_for_backward(P, S)
        return out

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        if getattr(engine, "_autograd_stamp", None) != ctx.stamp:
            raise RuntimeError("facedeform_amd.autograd.deform: the engine's model has been replaced by a later forward; "
                               "run backward before the next forward on the same engine")
        P, S = ctx.saved_tensors
        n = P.shape[0]
        g = g.to(torch.float32).contiguous()
        radius2, falloffrate = ctx.gate
        want_P, want_delta = ctx.needs_input_grad[0], ctx.has_delta and ctx.needs_input_grad[1]
        gp = torch.empty((n, 3), dtype=torch.float64, device=P.device) if want_P else None
        gw = torch.empty((S.shape[0], 3), dtype=torch.float64, device=P.device) if want_delta else None
        with _EngineStream(engine, P.device):
            if want_P:
                engine.deform_adjoint_points_dev(n, P.data_ptr(), g.data_ptr(), gp.data_ptr(), radius2=radius2,
                                                 falloffrate=falloffrate, **ctx.ptrs)
            if want_delta:
                engine.deform_adjoint_dev(n, P.data_ptr(), g.data_ptr(), gw.data_ptr(), radius2=radius2,
                                          falloffrate=falloffrate, **ctx.ptrs)
        grad_P = grad_delta = None
        if want_P:
            if ctx.displacement:
                gp = gp - g                              # the cotangent of the POSITION output minus the identity's share
            grad_P = gp.to(P.dtype)
        if want_delta:
            grad_delta = torch.matmul(S.t(), gw).to(torch.float32)
        return grad_P, grad_delta, None, None, None, None, None, None, None


def deform(engine: capi.Engine, P: torch.Tensor, delta: torch.Tensor | None = None, *, S: torch.Tensor | None = None, dist2=None,
           tangents=None, radius2=1.0, falloffrate=1.0, displacement=False) -> torch.Tensor:
    """P' = x + f Pi d(x) (displacement=True: f Pi d(x) alone) for the (N, 3) points P, differentiable in P and in delta.

    engine: a capi.Engine whose rest rig is set and built (set_points + build); the call is ordered on torch's current stream.
    P, delta, dist2, tangents = (tu, tv, nrm): contiguous float32 CUDA tensors.  delta (M, 3): new deltas for the rest rig
    (fd_set_deltas_dev + fd_build_async); None evaluates the model the engine holds.  S: solve_operator_tensor(engine), needed
    when delta requires grad (ValueError without it).  See the module's docstring for the one-model-per-engine rule and for
    what is not differentiated."""
    _checked("P", P)
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError("P must be (N, 3)")
    n = P.shape[0]
    if delta is not None:
        _checked("delta", delta, (engine.M, 3))
        if delta.requires_grad and S is None:
            raise ValueError("delta requires grad: pass S = solve_operator_tensor(engine)")
    if S is not None:
        if not (S.is_cuda and S.dtype == torch.float64 and S.dim() == 2 and S.shape[1] == engine.M):
            raise ValueError("S must be solve_operator_tensor(engine)'s float64 CUDA tensor")
        S = S.contiguous()
    if dist2 is not None:
        _checked("dist2", dist2, (n,))
    frames = None
    if tangents is not None:
        frames = tuple(_checked(name, t, (n, 3)) for name, t in zip(("tu", "tv", "nrm"), tangents))
        if len(frames) != 3:
            raise ValueError("tangents must be (tu, tv, nrm)")
    return _Deform.apply(P, delta, S, engine, dist2, frames, float(radius2), float(falloffrate), bool(displacement))


class _DeformShot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, deltas, S, batch, rest, dist2, frames, radius2, falloffrate, displacement):
        n, F, M = P.shape[0], deltas.shape[0], deltas.shape[1]
        out = torch.empty((F, n, 3), dtype=P.dtype, device=P.device)
        kw = dict(d_dist2=dist2.data_ptr() if dist2 is not None else 0,
                  d_tangents=tuple(t.data_ptr() for t in frames) if frames is not None else None)
        # every batch call below goes to context 0's stream, which _EngineStream sets
        with _EngineStream(batch.engines[0], P.device):
            for e in batch.engines:
                e.set_output(capi.OUTPUT_DISPLACEMENT if displacement else capi.OUTPUT_POSITION)
            batch.set_points_dev([rest.data_ptr()] * F, [deltas.data_ptr() + 12 * M * f for f in range(F)], M)
            batch.build_async()
            batch.deform_shared_fp64_dev(n, P.data_ptr(), [out[f].data_ptr() for f in range(F)], radius2=radius2,
                                         falloffrate=falloffrate, **kw)
        batch._autograd_stamp = getattr(batch, "_autograd_stamp", 0) + 1
        ctx.batch, ctx.stamp, ctx.kw = batch, batch._autograd_stamp, kw
        ctx.gate = (radius2, falloffrate)
        ctx.displacement = displacement
        ctx.keep = (rest, deltas, dist2, frames)        # the arrays the contexts read in place stay alive until backward
        ctx.save_for_backward(P, S)
        return out

    @staticmethod
    def backward(ctx, g):
        batch = ctx.batch
        if getattr(batch, "_autograd_stamp", None) != ctx.stamp:
            raise RuntimeError("facedeform_amd.autograd.deform_shot: the batch's models have been replaced by a later forward; "
                               "run backward before the next forward on the same batch")
        P, S = ctx.saved_tensors
        F, n = g.shape[0], P.shape[0]
        g = g.to(torch.float32).contiguous()
        radius2, falloffrate = ctx.gate
        want_P, want_delta = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gp = torch.empty((n, 3), dtype=torch.float64, device=P.device) if want_P else None
        gw = torch.empty((F, S.shape[0], 3), dtype=torch.float64, device=P.device) if want_delta else None
        e0 = batch.engines[0]
        with _EngineStream(e0, P.device):
            if want_P:
                batch.deform_adjoint_points_shared_dev(n, P.data_ptr(), g.data_ptr(), gp.data_ptr(), radius2=radius2,
                                                       falloffrate=falloffrate, **ctx.kw)
            if want_delta:
                # Psi does not depend on the weights: any built context of the batch gives every frame's grad_W
                tu, tv, nr = ctx.kw["d_tangents"] if ctx.kw["d_tangents"] is not None else (0, 0, 0)
                e0.deform_adjoint_shot_dev(n, F, P.data_ptr(), g.data_ptr(), gw.data_ptr(), ctx.kw["d_dist2"], tu, tv, nr, radius2,
                                           falloffrate)
        grad_P = grad_delta = None
        if want_P:
            if ctx.displacement:
                gp = gp - g.to(torch.float64).sum(dim=0)    # the cotangents of the POSITION outputs minus the identities' share
            grad_P = gp.to(P.dtype)
        if want_delta:
            grad_delta = torch.matmul(S.t(), gw).to(torch.float32)
        return grad_P, grad_delta, None, None, None, None, None, None, None, None


def deform_shot(batch: capi.Batch, P: torch.Tensor, rest: torch.Tensor, deltas: torch.Tensor, *, S: torch.Tensor | None = None,
                dist2=None, tangents=None, radius2=1.0, falloffrate=1.0, displacement=False) -> torch.Tensor:
    """P'_f = x + f Pi d_f(x) (displacement=True: f Pi d_f(x) alone) for the (N, 3) points P and the F frames of a shot: (F, N, 3),
    differentiable in P and in deltas.

    batch: a capi.Batch of F engines with kernel and term set; the call is ordered on torch's current stream.  rest (M, 3): the
    ONE rest rig, read in place by every context; deltas (F, M, 3): the frames' deltas.  P, rest, deltas, dist2, tangents =
    (tu, tv, nrm): contiguous float32 CUDA tensors.  S: solve_operator_tensor of one of the batch's engines for this rest rig,
    needed when deltas requires grad (ValueError without it).  Every call builds the F models anew; the backward reads them,
    so it must run before the next forward on the same batch (RuntimeError otherwise).  See the module's docstring for what is
    not differentiated."""
    _checked("P", P)
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError("P must be (N, 3)")
    n, F = P.shape[0], len(batch.engines)
    _checked("rest", rest)
    if rest.dim() != 2 or rest.shape[1] != 3:
        raise ValueError("rest must be (M, 3)")
    M = rest.shape[0]
    _checked("deltas", deltas, (F, M, 3))
    if deltas.requires_grad and S is None:
        raise ValueError("deltas requires grad: pass S = solve_operator_tensor(batch.engines[0])")
    if S is not None:
        if not (S.is_cuda and S.dtype == torch.float64 and S.dim() == 2 and S.shape[1] == M):
            raise ValueError("S must be solve_operator_tensor's float64 CUDA tensor for this rest rig")
        S = S.contiguous()
    if dist2 is not None:
        _checked("dist2", dist2, (n,))
    frames = None
    if tangents is not None:
        frames = tuple(_checked(name, t, (n, 3)) for name, t in zip(("tu", "tv", "nrm"), tangents))
        if len(frames) != 3:
            raise ValueError("tangents must be (tu, tv, nrm)")
    return _DeformShot.apply(P, deltas, S, batch, rest, dist2, frames, float(radius2), float(falloffrate), bool(displacement))
