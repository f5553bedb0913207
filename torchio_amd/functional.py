"""Functional entry points on plain tensors (no ``Subject``, no parameter draws)."""
from __future__ import annotations

from collections.abc import Sequence

import torch
from torch import Tensor

from . import ops


def warp(
    data: Tensor,
    mapping: Tensor,
    control_points: Tensor | None = None,
    *,
    out_shape: Sequence[int] | None = None,
    in_spacing: Sequence[float] = (1, 1, 1),
    out_spacing: Sequence[float] = (1, 1, 1),
    affine_first: bool = True,
    fill: float | Sequence[float] | Tensor | None = None,
) -> Tensor:
    """Resample one ``(B, C, I, J, K)`` tensor trilinearly through an affine map and an optional elastic displacement.

    ``mapping`` is ``(3, 4)`` or ``(1|B, 3, 4)``: output voxel -> input voxel.  ``control_points`` is ``(ni, nj, nk, 3)`` or
    ``(1|B, ni, nj, nk, 3)``: displacements in mm on a coarse grid that spans the output grid corner to corner, interpolated
    trilinearly; with ``affine_first`` the sampling coordinate is ``M c + d / in_spacing``, otherwise ``M (c + d / out_spacing)``.
    Voxels that sample outside the input read zero padding; with ``fill`` (one value, or one per channel) a voxel whose
    in-bounds weight is at most one half receives the fill value instead.  ``out_shape`` defaults to the input's.

    Differentiable in all three tensors: ``data`` through the adjoint scatter, ``mapping`` and ``control_points`` through one
    fused reduction launch (``tio_resample3d_geometry_grad``) - no ``(B, I, J, K, 3)`` grid is built in either direction.  The
    geometry may live on the host and in float64: its gradient arrives in the leaf's dtype, on the leaf's device.
    """
    if data.ndim != 5:
        raise ValueError(f"warp: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
    if mapping.ndim == 2:
        mapping = mapping[None]
    if control_points is not None and control_points.ndim == 4:
        control_points = control_points[None]
    if fill is not None and not isinstance(fill, Tensor):
        values = [float(fill)] * data.shape[1] if isinstance(fill, (int, float)) else [float(v) for v in fill]
        fill = torch.tensor(values, dtype=torch.float32)
    (out,) = ops.engine().resample3d(
        [data], out_shape=tuple(data.shape[2:]) if out_shape is None else tuple(int(s) for s in out_shape), mapping=mapping,
        control_points=control_points, in_spacing=in_spacing, out_spacing=out_spacing, affine_first=affine_first, interps=["linear"],
        fills=[fill],
    )
    return out
