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


def _wants_grad(tensor: Tensor | None) -> bool:
    return tensor is not None and torch.is_grad_enabled() and tensor.requires_grad
