"""Test-only helpers of tests/test_gpu_interpolate_adjoint.py and its guarded twin: references and per-voxel bounds for the three
gather adjoints of ``interpolate_adjoint.hip`` (``Engine.interpolate3d_adjoint``, ``axis_gather_lerp_adjoint``, ``pad3d_adjoint``).
Nothing here is imported by the product.

Two references, as for the resampler's adjoint (``adjoint_reference``):

* ``dense_matrix``: at small shapes the FORWARD of the one-hot volumes, riding as channels, is the matrix ``A`` of the op in the
  forward's own float32 weights.  ``A^T g`` in float64 is then the exact answer.  ``check_against_dense`` holds every voxel to
  ``(N_v + slack) u S_v``, ``S = |A|^T |g|``, ``N_v`` the non-zeros of column ``v``.  The slack is derived, not measured:
    - a product of three weights carries two roundings in the forward (the entry of ``A``) and two in the adjoint, which may
      associate differently: 4; the product with ``g``: 1; the ``N_v - 1`` additions: within ``N_v``; one spare for the
      second-order terms and the merged taps of a last index (``l0 + l1`` rounded once more): ``N_v + 6`` for the two
      interpolating ops;
    - padding moves values, its weights are exactly 1: only the additions remain, ``N_v + 1`` (``adjoint_reference``'s bound).
* float64 autograd through ``F.interpolate`` / ``F.pad`` on the device at launch sizes, with the bounds of ``linear_bound`` /
  ``exact_weight_bound``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24  # unit roundoff of float32


def randn(shape, seed: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
def dense_matrix(forward, in_shape, batch: int = 1, device="cpu") -> torch.Tensor:
    """``A`` as ``(batch, n_in, n_out)`` float32: ``A[b, v, o]`` is what output voxel ``o`` of element ``b`` takes from input
    voxel ``v``.  *forward* maps a ``(batch, n_in, *in_shape)`` tensor of one-hot volumes (the channels) to its result."""
    i, j, k = in_shape
    n = i * j * k
    one_hots = torch.eye(n, dtype=torch.float32, device=device).reshape(1, n, i, j, k).repeat(batch, 1, 1, 1, 1)
    return forward(one_hots).reshape(batch, n, -1)


def check_against_dense(matrix: torch.Tensor, grad: torch.Tensor, result: torch.Tensor, slack: int, what: str) -> float:
    """``|result_v - (A^T g)_v| <= (N_v + slack) u S_v`` at EVERY input voxel; prints and returns the worst error / bound."""
    batch, channels = grad.shape[:2]
    a64 = matrix.double().cpu().expand(batch, -1, -1)
    g64 = grad.double().cpu().reshape(batch, channels, -1)
    reference = torch.einsum("bvo,bco->bcv", a64, g64)
    magnitude = torch.einsum("bvo,bco->bcv", a64.abs(), g64.abs())
    counts = (a64 != 0).sum(dim=2).double()[:, None, :]
    bound = (counts + slack) * U * magnitude
    error = (result.double().cpu().reshape(batch, channels, -1) - reference).abs()
    worst = torch.where(bound > 0, error / bound, torch.where(error > 0, torch.full_like(error, math.inf), torch.zeros_like(error)))
    print(f"[dense] {what}: worst error / bound = {float(worst.max()):.3g}, N_v up to {int(counts.max())}, "
          f"{int((counts == 0).sum())} empty columns")
    bad = int((error > bound).sum())
    assert bad == 0, f"{what}: {bad} voxels beyond (N_v + {slack}) u S_v; worst error / bound = {float(worst.max()):.3g}"
    return float(worst.max())


# ---------------------------------------------------------------------------------------------------------------------
# 2. float64 autograd at launch sizes
# ---------------------------------------------------------------------------------------------------------------------
def _autograd64(op, in_shape, grad: torch.Tensor) -> torch.Tensor:
    with torch.enable_grad():
        leaf = torch.zeros((*grad.shape[:2], *in_shape), dtype=torch.float64, device=grad.device).requires_grad_(True)
        (result,) = torch.autograd.grad(op(leaf), leaf, grad.double())
    return result


def interpolate_reference(grad: torch.Tensor, in_shape, mode: str) -> torch.Tensor:
    """``d <F.interpolate(x), grad> / dx`` in float64 on the gradient's device (*mode*: ``"linear"`` or ``"nearest"``)."""
    size = tuple(grad.shape[2:])
    if mode == "linear":
        return _autograd64(lambda x: F.interpolate(x, size=size, mode="trilinear", align_corners=True), in_shape, grad)
    return _autograd64(lambda x: F.interpolate(x, size=size, mode="nearest"), in_shape, grad)


def pad_reference(grad: torch.Tensor, in_shape, padding, mode: str) -> torch.Tensor:
    i0, i1, j0, j1, k0, k1 = padding
    return _autograd64(lambda x: F.pad(x, (k0, k1, j0, j1, i0, i1), mode=mode), in_shape, grad)


def nearest_tables(n_in: int, n_out: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The legacy-nearest source index of every output along one axis, in the forward's float32 expression and in float64."""
    o = torch.arange(n_out)
    scale32 = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    index32 = torch.floor(o.to(torch.float32) * scale32).to(torch.int64).clamp(max=n_in - 1)
    index64 = torch.floor(o.to(torch.float64) * (n_in / n_out)).to(torch.int64).clamp(max=n_in - 1)
    return index32, index64


def _linear_reach(n_in: int, n_out: int) -> torch.Tensor:
    """``(n_out, n_in)`` float64 0/1: input ``v`` is a tap of output ``o`` along one axis, in the float32 OR the float64 chain."""
    reach = torch.zeros(n_out, n_in, dtype=torch.float64)
    o = torch.arange(n_out)
    if n_in == n_out:
        reach[o, o] = 1.0
        return reach
    scale32 = (torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32)) if n_out > 1 else torch.tensor(0.0)
    scale64 = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for real in (o.to(torch.float32) * scale32, o.to(torch.float64) * scale64):
        lower = torch.floor(real).to(torch.int64).clamp(max=n_in - 1)
        reach[o, lower] = 1.0
        reach[o, (lower + 1).clamp(max=n_in - 1)] = 1.0
    return reach


def linear_reach_sums(per_output: torch.Tensor, in_shape) -> torch.Tensor:
    """``(B, C, *in_shape)`` float64: per input voxel the sum of *per_output* over the outputs that can reach it."""
    out_shape = per_output.shape[2:]
    ri, rj, rk = (_linear_reach(n_in, n_out).to(per_output.device) for n_in, n_out in zip(in_shape, out_shape, strict=True))
    return torch.einsum("bcxyz,xi,yj,zk->bcijk", per_output.double(), ri, rj, rk)


def linear_bound(grad: torch.Tensor, in_shape) -> torch.Tensor:
    """``(12 u c + (N_v + 6) u) G_v`` with ``c`` the longest axis: a float32 source coordinate ``o * scale`` is within ``u c`` of
    the float64 one and its weight pair within a few ``u c`` - ``d <= 4 u c`` per factor; a three-factor weight then moves by at
    most ``3 d``; the summation adds ``(N_v + 6) u`` as against the dense matrix."""
    counts = linear_reach_sums(torch.ones_like(grad[:, :1]), in_shape)
    sums = linear_reach_sums(grad.abs(), in_shape)
    longest = float(max(*in_shape, *grad.shape[2:]))
    return (12 * U * longest + (counts + 6) * U) * sums


def exact_weight_bound(adjoint64, grad: torch.Tensor) -> torch.Tensor:
    """``(N_v + 1) u G_v`` for an op whose weights are exactly 0 or 1 (nearest, padding): *adjoint64* is the float64 reference
    itself, which applied to ones and to ``|g|`` gives ``N_v`` and ``G_v`` exactly."""
    counts = adjoint64(torch.ones_like(grad[:1, :1]))
    return (counts + 1) * U * adjoint64(grad.abs())


def assert_within(actual: torch.Tensor, expected: torch.Tensor, tolerance: torch.Tensor, what: str) -> float:
    error = (actual.double() - expected.double()).abs()
    ratio = torch.where(tolerance > 0, error / tolerance, torch.where(error > 0, torch.full_like(error, math.inf), torch.zeros_like(error)))
    print(f"[autograd64] {what}: worst error / bound = {float(ratio.max()):.3g}")
    bad = int((error > tolerance).sum())
    assert bad == 0, f"{what}: {bad} of {error.numel()} voxels beyond their bound, worst error / bound = {float(ratio.max()):.3g}"
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# the CSR inversion of the axis tables, index by index
# ---------------------------------------------------------------------------------------------------------------------
def brute_force_lists(lower: torch.Tensor, upper: torch.Tensor | None, weight: torch.Tensor | None):
    """Per element and source index the list of ``(position, weight)``: the ``lower`` uses by ascending position, then the
    ``upper`` uses (what ``Engine.axis_gather_lists`` documents)."""
    batch, length = lower.shape
    lists = [[[] for _ in range(length)] for _ in range(batch)]
    for b in range(batch):
        for p in range(length):
            w = None if weight is None else weight[b, p]
            if 0 <= int(lower[b, p]) < length:
                lists[b][int(lower[b, p])].append((p, 1.0 if w is None else float(torch.tensor(1.0) - w)))
        if upper is not None:
            for p in range(length):
                if 0 <= int(upper[b, p]) < length:
                    lists[b][int(upper[b, p])].append((p, float(weight[b, p])))
    return lists
