"""Seeded input builders shared by the parity tests (``test_gpu_ops_parity.py`` and the modules that import from it) and
the guarded cases (``guarded_cases.py``): CPU tensors only, so they serve the oracle and the HIP engine alike."""
from __future__ import annotations

import torch


def _mapping(batch, seed, scale=0.15, shift=3.0):
    g = torch.Generator().manual_seed(seed)
    m = torch.eye(3, 4).repeat(batch, 1, 1)
    m[:, :, :3] += scale * torch.randn(batch, 3, 3, generator=g)
    m[:, :, 3] = shift * torch.randn(batch, 3, generator=g)
    return m.float()


def _control_points(batch, shape, seed, amplitude=4.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(batch, *shape, 3, generator=g) - 0.5) * 2 * amplitude).float()


def _data(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        return (torch.rand(*shape, generator=g) * 4 - 1).to(dtype)
    return torch.randint(0, 7, shape, generator=g).to(dtype)


def _taps(batch, sigmas, stride):
    taps = torch.zeros(batch, 3, stride)
    radius = [0, 0, 0]
    for b in range(batch):
        for axis in range(3):
            s = sigmas[b][axis]
            if s <= 0:
                continue
            r = max(int(-(-3 * s // 1)), 1)
            radius[axis] = max(radius[axis], r)
    for b in range(batch):
        for axis in range(3):
            r = radius[axis]
            if r == 0:
                continue
            s = sigmas[b][axis]
            x = torch.arange(2 * r + 1, dtype=torch.float32) - r
            if s > 0:
                k = torch.exp(-0.5 * (x / s) ** 2)
                k[(x.abs() > max(int(-(-3 * s // 1)), 1))] = 0
            else:
                k = (x == 0).float()
            taps[b, axis, : 2 * r + 1] = k / k.sum()
    return taps, radius


def _segments(shape, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(*shape, generator=g) * 4 - 1) for _ in range(n)]


def _rotation_mapping(degrees, size):
    """``(1, 3, 4)`` output -> input voxel mapping: a rotation by *degrees* about every axis, about the centre of a *size*^3
    volume, shifted by 1.5 voxels (boxes of rotated bricks exceed the resamplers' staging tile from about 30 degrees)."""
    import math

    angle = math.radians(degrees)
    c, s = math.cos(angle), math.sin(angle)
    rx = torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float64)
    ry = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    rz = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64)
    rotation = rz @ ry @ rx
    centre = torch.full((3,), (size - 1) / 2.0, dtype=torch.float64)
    shift = centre - rotation @ centre + 1.5
    return torch.cat([rotation, shift[:, None]], dim=1).to(torch.float32)[None]


def _blocky_labels(shape, dtype, seed, count):
    """Label volumes of 2-voxel blocks with values 0 .. count - 1 (plenty of mixed neighbourhoods), 15 % of the voxels redrawn."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, count, tuple((s + 1) // 2 for s in shape[-3:]), generator=g)
    full = coarse.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)[: shape[-3], : shape[-2], : shape[-1]]
    noise = torch.randint(0, count, shape, generator=g)
    pick = torch.rand(shape, generator=g) < 0.15
    return torch.where(pick, noise, full.expand(shape)).to(dtype)
