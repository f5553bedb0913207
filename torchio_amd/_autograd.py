"""How an engine result gets its place in the autograd graph (shared by ``ops.Engine`` and ``noise_stream``)."""
from __future__ import annotations

import torch
from torch import Tensor


class _AttachBackward(torch.autograd.Function):
    """Give an engine result its place in the autograd graph: ``result`` was computed by a kernel from
    ``source.detach()``; ``backward_fn(grad)`` returns dL/d(source) (another kernel, or tensor algebra)."""

    @staticmethod
    def forward(ctx, source, result, backward_fn):
        ctx.backward_fn = backward_fn
        return result.view_as(result)

    @staticmethod
    def backward(ctx, grad):
        return ctx.backward_fn(grad.contiguous()), None, None


class _AttachBackwardMany(torch.autograd.Function):
    """``_AttachBackward`` for a kernel with several data inputs (Motion's k-space composite): ``result`` was computed from the
    detached ``sources``; ``backward_fn(grad, needs)`` returns one gradient (or ``None``) per source, ``needs[n]`` telling which
    are wanted."""

    @staticmethod
    def forward(ctx, backward_fn, result, *sources):
        ctx.backward_fn = backward_fn
        return result.view_as(result)

    @staticmethod
    def backward(ctx, grad):
        return (None, None, *ctx.backward_fn(grad.contiguous(), ctx.needs_input_grad[2:]))


class _AttachGeometryBackward(torch.autograd.Function):
    """Give the results of one resampling call their dependence on its geometry: ``results`` were computed by a kernel from the
    detached ``mapping`` / ``control_points`` (the leaves, or what leads to them); ``backward_fn(grads, want_mapping,
    want_control_points)`` returns ``(dL/d mapping | None, dL/d control_points | None)`` as float32 device tensors, which are cast to
    the dtype and moved to the device of the tensor they belong to.  The gradients of the results pass through unchanged (an image
    that requires a gradient had its own backward attached before)."""

    @staticmethod
    def forward(ctx, backward_fn, mapping, control_points, *results):
        ctx.backward_fn = backward_fn
        ctx.like = [None if t is None else (t.shape, t.dtype, t.device) for t in (mapping, control_points)]
        return tuple(result.view_as(result) for result in results)

    @staticmethod
    def backward(ctx, *grads):
        from ._lib import EngineError  # noqa: PLC0415

        wants = ctx.needs_input_grad[1:3]
        if torch.is_grad_enabled() and any(wants):
            raise EngineError("resample3d: the gradient with respect to the mapping / control points cannot be differentiated again"
                              " (no double backward through tio_resample3d_geometry_grad)")
        geometry = [None, None]
        if any(wants):
            computed = ctx.backward_fn([None if grad is None else grad.contiguous() for grad in grads], wants[0], wants[1])
            for slot, (value, like) in enumerate(zip(computed, ctx.like, strict=True)):
                if wants[slot] and like is not None:
                    shape, dtype, device = like
                    geometry[slot] = torch.zeros(shape, dtype=dtype, device=device) if value is None else value.reshape(shape).to(device=device, dtype=dtype)
        return (None, *geometry, *grads)


class _AttachParameterBackward(torch.autograd.Function):
    """Give the result of an intensity op its dependence on the op's parameters (the coarse bias grid, the blur taps, the noise
    mean / deviation, the gamma exponent): ``result`` was computed by a kernel from the detached ``parameters`` (the leaves, or
    what leads to them; ``None`` for one that is a plain number).  ``backward_fn(grad, wants)`` returns one float32 device tensor
    (or ``None``) per parameter, which is cast to the dtype and moved to the device of the tensor it belongs to.  The gradient of
    the result passes through unchanged (data that requires a gradient had its own backward attached before)."""

    @staticmethod
    def forward(ctx, what, backward_fn, result, *parameters):
        ctx.what, ctx.backward_fn = what, backward_fn
        ctx.like = [None if t is None else (t.shape, t.dtype, t.device) for t in parameters]
        return result.view_as(result)

    @staticmethod
    def backward(ctx, grad):
        from ._lib import EngineError  # noqa: PLC0415

        wants = ctx.needs_input_grad[3:]
        if torch.is_grad_enabled() and any(wants):
            raise EngineError(f"{ctx.what}: the gradient with respect to the parameters cannot be differentiated again"
                              " (no double backward through the parameter-gradient kernels)")
        out = [None] * len(wants)
        if any(wants):
            computed = ctx.backward_fn(grad.contiguous(), wants)
            for slot, (value, like) in enumerate(zip(computed, ctx.like, strict=True)):
                if wants[slot] and like is not None:
                    shape, dtype, device = like
                    out[slot] = torch.zeros(shape, dtype=dtype, device=device) if value is None else value.reshape(shape).to(device=device, dtype=dtype)
        return (None, None, grad, *out)


def _wants_grad(tensor: Tensor | None) -> bool:
    return tensor is not None and torch.is_grad_enabled() and tensor.requires_grad
