"""Functional entry points on plain tensors (no ``Subject``, no parameter draws)."""
from __future__ import annotations

import math
from collections.abc import Sequence

import numpy as np
import torch
from torch import Tensor

from . import ops


def _volume(data: Tensor, what: str) -> None:
    if not isinstance(data, Tensor) or data.ndim != 5:
        raise ValueError(f"{what}: expected a (B, C, I, J, K) tensor, got {tuple(data.shape) if isinstance(data, Tensor) else type(data).__name__}")


def _one_or_per_element(value, batch: int, what: str):
    """A number, or a tensor of 1 or ``batch`` values (its shape is kept: that is the shape its gradient arrives in)."""
    if isinstance(value, Tensor):
        if value.numel() not in (1, batch):
            raise ValueError(f"{what} must hold 1 or {batch} values, got {tuple(value.shape)}")
        return value
    return float(value)


def bias_field(data: Tensor, coarse: Tensor, *, divide: bool = False) -> Tensor:
    """``data * exp(trilinear_upsample(coarse))`` (``divide``: ``data / ...``) on a ``(B, C, I, J, K)`` tensor.

    ``coarse`` is ``(B, C, si, sj, sk)`` (or ``(si, sj, sk)`` for ``B == C == 1``): the logarithm of the field on a coarse grid that
    spans the volume corner to corner.  Differentiable in both tensors: ``data`` through the same multiply, ``coarse`` through one
    fused reduction launch (``tio_bias_field_grad``) - no full-size field or gradient of it reaches memory.  ``coarse`` may live on
    the host and in float64: its gradient arrives in the leaf's dtype, on the leaf's device.
    """
    _volume(data, "bias_field")
    if not isinstance(coarse, Tensor) or coarse.ndim not in (3, 5):
        raise ValueError("bias_field: coarse must be (B, C, si, sj, sk) or (si, sj, sk)")
    if coarse.ndim == 3:
        coarse = coarse[None, None]
    if tuple(coarse.shape[:2]) != tuple(data.shape[:2]):
        raise ValueError(f"bias_field: coarse {tuple(coarse.shape)} does not carry the data's (B, C) = {tuple(data.shape[:2])}")
    if not coarse.requires_grad:
        coarse = ops.h2d(coarse.to(torch.float32), data.device)
    return ops.engine().bias_field_apply(data, coarse, divide=divide)


def gamma(data: Tensor, gamma: float | Tensor) -> Tensor:  # noqa: A002 (the transform's own name)
    """``sign(data) * |data| ** gamma`` with one exponent or one per batch element (a number, or a tensor of 1 or ``B`` values).

    Differentiable in ``data`` and in a tensor ``gamma`` (``tio_gamma_grad``: ``sum grad * y * log|x|`` over ``x != 0``).
    """
    _volume(data, "gamma")
    return ops.engine().gamma_pow(data, _one_or_per_element(gamma, data.shape[0], "gamma"))


def noise(data: Tensor, mean: float | Tensor, std: float | Tensor, *, seed: int | None = None, draws: Tensor | Sequence[Tensor] | None = None,
          rician: bool = False) -> Tensor:
    """``data + (mean + std * z)``; ``rician``: ``sqrt((data + n1)^2 + n2^2)`` with ``n_i = mean + std * z_i``.

    ``z`` is standard normal: ``draws`` (one float32 tensor shaped like ``data``; two for ``rician``), or the Philox stream of
    ``seed``.  ``mean`` / ``std`` are numbers or tensors of 1 or ``B`` values.  Differentiable in ``data`` and in tensor ``mean`` /
    ``std`` (``tio_noise_grad``); with Philox draws the backward pass regenerates them, none is stored.
    """
    _volume(data, "noise")
    if (seed is None) == (draws is None):
        raise ValueError("noise: give either `seed` (Philox draws) or `draws`, not both")
    mean = _one_or_per_element(mean, data.shape[0], "mean")
    std = _one_or_per_element(std, data.shape[0], "std")
    base1 = base2 = None
    if draws is not None:
        given = [draws] if isinstance(draws, Tensor) else list(draws)
        if len(given) != (2 if rician else 1):
            raise ValueError(f"noise: {'rician noise needs two tensors of draws' if rician else 'additive noise needs one tensor of draws'}")
        for base in given:
            if tuple(base.shape) != tuple(data.shape):
                raise ValueError(f"noise: draws {tuple(base.shape)} are not shaped like the data {tuple(data.shape)}")
        base1, base2 = (given + [None])[:2]
        base1 = base1.to(device=data.device, dtype=torch.float32)
        base2 = None if base2 is None else base2.to(device=data.device, dtype=torch.float32)
    return ops.engine().add_noise(data, mean, std, rician=rician, base1=base1, base2=base2, philox_seed=0 if seed is None else int(seed))


def _gaussian_taps(sigmas: Tensor, per_element: bool) -> tuple[Tensor, list[int], np.ndarray | None]:
    """``transforms/blur.py::_stacked_gaussian_taps`` on a TENSOR of sigmas ``(n, 3)``, differentiable in it: the same float32
    expressions in the same order (for the same sigmas the taps are the same, bit for bit), on the host; the radii are read from
    the values.  Returns ``(taps (n, 3, stride) float32, radius[3], skip | None)``."""
    from .transforms.blur import _tap_distance, _tap_offsets  # noqa: PLC0415

    values = sigmas.detach().to(device="cpu", dtype=torch.float64).numpy()
    sigma32 = sigmas.to(device="cpu", dtype=torch.float32)  # (in the graph: what the taps are a function of)
    n = values.shape[0]
    radii_rows = [[max(math.ceil(3 * value), 1) if value > 0 else 0 for value in row] for row in values.tolist()]
    radius = [max(row[axis] for row in radii_rows) for axis in range(3)]
    stride = 2 * max(radius) + 1
    taps = torch.zeros(n, 3, stride, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    radii = positive = None
    if per_element:
        radii = np.asarray(radii_rows, dtype=np.int64)
        positive = radii > 0
        if bool(positive.all()):
            reach = max(radius)
            offsets = _tap_offsets(reach)
            kernels = torch.exp(-0.5 * (offsets[None, None, :] / sigma32[:, :, None]) ** 2)
            kernels = torch.where(_tap_distance(reach)[None, None, :] <= torch.from_numpy(radii)[:, :, None], kernels, zero)
            for axis in range(3):
                r = radius[axis]
                window = kernels[:, axis, reach - r : reach + r + 1]
                taps[:, axis, : 2 * r + 1] = window / window.sum(dim=1, keepdim=True)
            return taps, radius, None
    for axis in range(3):
        r = radius[axis]
        if r == 0:
            continue
        offsets = _tap_offsets(r)
        if not per_element:
            kernel = torch.exp(-0.5 * (offsets / sigma32[0, axis]) ** 2)
            taps[0, axis, : 2 * r + 1] = kernel / kernel.sum()
            continue
        sigma_column = sigma32[:, axis][:, None]
        all_active = bool(positive[:, axis].all())
        safe = sigma_column if all_active else torch.where(sigma_column > 0, sigma_column, torch.ones_like(sigma_column))
        kernels = torch.exp(-0.5 * (offsets[None, :] / safe) ** 2)
        if int(radii[:, axis].min()) != r:
            radius_column = torch.as_tensor(radii[:, axis])[:, None]
            kernels = torch.where(offsets[None, :].abs() <= radius_column, kernels, torch.zeros_like(kernels))
        if not all_active:
            delta = torch.zeros_like(kernels)
            delta[:, r] = 1.0
            kernels = torch.where(sigma_column > 0, kernels, delta)
        taps[:, axis, : 2 * r + 1] = kernels / kernels.sum(dim=1, keepdim=True)
    skip = None
    if per_element:
        no_blur = np.all(values <= 0, axis=1)
        if no_blur.any():
            skip = no_blur.astype(np.uint8)
    return taps, radius, skip


def blur(data: Tensor, sigma_vox: Tensor | Sequence[float]) -> Tensor:
    """Separable Gaussian smoothing with replicate padding; ``sigma_vox`` is ``(3,)`` or ``(B, 3)``, in voxels (``<= 0`` skips an axis).

    Differentiable in ``data`` (the transposed clamped stencil) and in a tensor ``sigma_vox``: the taps' gradient is one clamped
    tap correlation per axis (``tio_separable_conv3d_taps_grad``), and the chain from the taps to the sigmas runs in torch on the
    handful of tap values.  The radius of each axis is read from the VALUE of its sigma (``ceil(3 sigma)``) and is not differentiated.
    """
    _volume(data, "blur")
    sigmas = sigma_vox if isinstance(sigma_vox, Tensor) else torch.as_tensor(np.asarray(sigma_vox, dtype=np.float64))
    if sigmas.ndim == 1:
        sigmas = sigmas[None]
    if sigmas.ndim != 2 or sigmas.shape[1] != 3 or sigmas.shape[0] not in (1, data.shape[0]):
        raise ValueError(f"blur: sigma_vox must be (3,) or ({data.shape[0]}, 3), got {tuple(sigmas.shape)}")
    values = sigmas.detach().to(device="cpu", dtype=torch.float64).numpy()
    if np.all(values <= 0):
        return data
    # identical rows collapse to the shared kernel set, unless they take part in autograd (each row then receives its own gradient)
    per_element = values.shape[0] > 1 and (not np.all(values == values[0]) or (sigmas.requires_grad and torch.is_grad_enabled()))
    rows = sigmas if per_element else sigmas[:1]
    taps, radius, skip = _gaussian_taps(rows, per_element)
    if not taps.requires_grad:
        taps = ops.h2d(taps, data.device)
    skip_flags = None if skip is None else ops.h2d(torch.from_numpy(skip), data.device)
    return ops.engine().separable_conv3d(data, taps, radius, skip=skip_flags)


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
