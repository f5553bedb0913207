"""Geometries, expected outputs and the trilinear bound of ``test_gpu_resample_size_gates.py`` (a plain module, no tests in it; the
host test of the bound's teeth is in ``test_size_gates_host.py``).

Nearest cases: an integer translation plus axis flips.  The mapping's entries are integers of at most 2^24 in magnitude, so every
product and partial sum of the affine row is an integer of at most 2^24: exact in float32.  The round trip through the normalised
grid (``2 v / (S - 1) - 1`` and back) then rounds four times; at extents of a few thousand that moves the coordinate by 1e-3 voxel
at most, far from the rounding tie at one half.  On the long axis of 2^23 / 2^24 voxels float32 has no room for a fraction: the
chain's result is an integer, and the cases there rely on it being the RIGHT integer — which the CPU oracle, the restatement of
the reference's chain with 64-bit indices, confirms for each of them (it reproduces the analytic shift bit for bit, in about a
second per case).  The expected output is the analytic input at the shifted position, zero outside.

Trilinear cases: the affine input ``f = bc + i/I + 2 j/J + 4 k/K`` under a mapping with a small rotation.  Trilinear interpolation
of an affine function is the function at the sample coordinate, so the reference is ``f`` in float64 at the float64 coordinate
``x_r = sum_c m_rc o_c + m_r3`` (the float32 mapping entries, exact in float64), and the bound per voxel is

    sum_r |df/dx_r| delta_r + 8 ulp32(|f|).

``delta_r``, the float32 coordinate error of resample_exact_chain.hpp / resample_coords.hpp along input axis ``r``, counted from
its operations with ``u = 2^-24`` and ``P_r = sum_c |m_rc| (S_out,c - 1) + |m_r3|``, which bounds every partial sum of the row and,
for voxels inside the volume, the coordinate itself:

* the affine row (``TIO_AFFINE_ROW``): one product and three fused multiply-adds, four roundings of at most ``u P_r`` each;
* ``normalise_roundtrip``: ``2 v`` is exact; the division by ``S - 1`` is correctly rounded, ``u 2P/(S-1)`` in normalised units;
  ``- 1`` and ``+ 1`` round at magnitudes of at most ``2P/(S-1) + 1`` and ``2P/(S-1)``; ``* 0.5`` is exact; these three errors are
  scaled by ``(S - 1) / 2``, which gives ``u (3 P_r + (S - 1) / 2)``; the last product rounds once more, ``u P_r``.

Together ``delta_r <= u (8 P_r + (S_r - 1) / 2) <= 8.5 u P_r`` (``P_r >= S_r - 1`` for a mapping that covers the volume): 5e-4 voxel
at extents of 1024.  Nothing here is taken from a run of the kernels.  The comparison leaves out the voxels whose coordinate lies
within one voxel of the volume's surface (zero padding enters their taps).
"""
from __future__ import annotations

import math

import torch

U = 2.0**-24

#: name -> (in_shape == out_shape, dtype, shift per axis, flipped axes): one side of a gate each
NEAREST_CASES = {
    # I * J <= 2^24 keeps the nearest kernel; beyond it nearest images run in the per-voxel gather kernel (resample.hip: sort_images)
    "ij_2_24": ((4096, 4096, 3), None, (3, -2, 1), (True, False, True)),
    "ij_beyond_2_24": ((4097, 4096, 3), None, (3, -2, 1), (True, False, True)),
    # K * es < 2^24 (the buffer-load kernels' 24-bit offsets) and K < 2^24 (the nearest kernel at all), with the neighbours one shorter;
    # at these lengths the exact-coordinate kernel is out anyway (no short division): see test_gpu_resample_size_gates.py
    "k_int16_2_23": ((2, 2, 2**23), torch.int16, (0, 1, -3), (False, True, True)),
    "k_int16_below_2_23": ((2, 2, 2**23 - 1), torch.int16, (0, 1, -3), (False, True, True)),
    "k_uint8_2_24": ((1, 2, 2**24), torch.uint8, (0, 0, 5), (False, True, False)),
    "k_uint8_below_2_24": ((1, 2, 2**24 - 1), torch.uint8, (0, 0, 5), (False, True, False)),
    # n_in * es and n_out * es against 2^32 - 16: int64 labels of 513 / 511 planes of 2^20 voxels
    "bytes_int64_513": ((513, 1024, 1024), torch.int64, (2, -3, 4), (True, False, False)),
    "bytes_int64_511": ((511, 1024, 1024), torch.int64, (2, -3, 4), (True, False, False)),
}
NEAREST_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32)  # of the cases whose dtype is None

#: name -> (channels, in_shape == out_shape): I J K = 2^30 takes the per-voxel gather road, the neighbour below a staged road
TRILINEAR_CASES = {
    "voxels_2_30": (2, (1024, 1024, 1024)),
    "voxels_below_2_30": (2, (1024, 1024, 1023)),
}


# -- nearest: integer translation and flips --------------------------------------------------------------------------------------
def shift_flip_mapping(shape, shift, flips) -> torch.Tensor:
    """``(1, 3, 4)`` float32, output voxel -> input voxel: ``in_d = out_d + shift_d``, or ``S_d - 1 - out_d + shift_d`` on a flipped axis."""
    mapping = torch.zeros(1, 3, 4)
    for d in range(3):
        mapping[0, d, d] = -1.0 if flips[d] else 1.0
        mapping[0, d, 3] = float(shape[d] - 1 + shift[d]) if flips[d] else float(shift[d])
    assert bool((mapping == mapping.round()).all()) and float(mapping.abs().max()) <= 2.0**24
    return mapping


def source_indices(shape, shift, flips, device):
    """Per axis: the source index of every output position (int64) and whether it lies inside the volume."""
    found = []
    for d in range(3):
        position = torch.arange(shape[d], device=device)
        source = (shape[d] - 1 - position + shift[d]) if flips[d] else position + shift[d]
        found.append((source.clamp(0, shape[d] - 1), (source >= 0) & (source < shape[d])))
    return found


def analytic_input(shape, dtype, device, channels: int = 1) -> torch.Tensor:
    """``(1, C, I, J, K)``: the "distinct" form of large_offset_cases.py."""
    import large_offset_cases as big

    return big.distinct((1, channels, *shape), dtype, device)


def shifted(data: torch.Tensor, shift, flips) -> torch.Tensor:
    """The expected output of a nearest launch: ``data`` at the source position, zero outside."""
    shape = tuple(data.shape[2:])
    (si, vi), (sj, vj), (sk, vk) = source_indices(shape, shift, flips, data.device)
    out = data.index_select(2, si).index_select(3, sj).index_select(4, sk)
    out[:, :, ~vi] = 0
    out[:, :, :, ~vj] = 0
    out[..., ~vk] = 0
    return out


# -- trilinear: the affine input under a small rotation ----------------------------------------------------------------------------
def rotation_mapping(shape) -> torch.Tensor:
    """``(1, 3, 4)`` float32: rotations of 0.4, -0.3 and 0.5 degrees about the three axes, about the volume's centre, then a shift of
    a fraction of a voxel (so no sample sits on a lattice point)."""
    angles = [math.radians(a) for a in (0.4, -0.3, 0.5)]
    (ca, sa), (cb, sb), (cc, sc) = [(math.cos(a), math.sin(a)) for a in angles]
    rx = torch.tensor([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], dtype=torch.float64)
    ry = torch.tensor([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], dtype=torch.float64)
    rz = torch.tensor([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]], dtype=torch.float64)
    rotation = rx @ ry @ rz
    centre = torch.tensor([(s - 1) / 2 for s in shape], dtype=torch.float64)
    offset = centre - rotation @ centre + torch.tensor([1.25, -0.75, 0.5], dtype=torch.float64)
    return torch.cat([rotation, offset[:, None]], dim=1)[None].to(torch.float32)


def coordinate_error(mapping: torch.Tensor, shape) -> list[float]:
    """``delta_r`` of the module docstring for each input axis."""
    m = mapping[0].double().abs()
    extents = torch.tensor([s - 1 for s in shape], dtype=torch.float64)
    return [U * (8 * float((m[r, :3] * extents).sum() + m[r, 3]) + (shape[r] - 1) / 2) for r in range(3)]


def ulp32(value: torch.Tensor) -> torch.Tensor:
    """The float32 spacing at ``|value|`` (float64 in, float64 out; at least the smallest normal's)."""
    return torch.exp2(torch.floor(torch.log2(value.abs().clamp_min(2.0**-126))) - 23)


def trilinear_reference(mapping: torch.Tensor, shape, channel: int, planes: slice, device, sample=None):
    """``(f, bound, interior, coordinates)`` in float64 for the output planes ``planes`` of one channel (or, with *sample*, for
    the ``(n, 3)`` int64 output positions given)."""
    m = mapping[0].double().to(device)
    if sample is None:
        i = torch.arange(shape[0], device=device, dtype=torch.float64)[planes].reshape(-1, 1, 1)
        j = torch.arange(shape[1], device=device, dtype=torch.float64).reshape(1, -1, 1)
        k = torch.arange(shape[2], device=device, dtype=torch.float64).reshape(1, 1, -1)
    else:
        i, j, k = (sample[:, d].double().to(device) for d in range(3))
    x = [m[r, 0] * i + m[r, 1] * j + m[r, 2] * k + m[r, 3] for r in range(3)]
    f = channel + x[0] / shape[0] + 2 * x[1] / shape[1] + 4 * x[2] / shape[2]
    delta = coordinate_error(mapping, shape)
    slope = delta[0] / shape[0] + 2 * delta[1] / shape[1] + 4 * delta[2] / shape[2]
    interior = (x[0] >= 1) & (x[0] <= shape[0] - 2) & (x[1] >= 1) & (x[1] <= shape[1] - 2) & (x[2] >= 1) & (x[2] <= shape[2] - 2)
    return f, slope + 8 * ulp32(f), interior, x


def simulated_wrap(name: str, wrap: str, samples: int = 50_000) -> tuple[int, int]:
    """``(touched, broken)`` over a random sample of interior output voxels of both channels: the voxel's source corner as a flat
    element index in the whole input tensor, wrapped modulo 2^30 elements or modulo 2^32 bytes (the same wrap for float32 — both are
    stated, both are run), decoded to the position such a kernel would read instead; *touched* counts the voxels whose index
    changes, *broken* those of them whose value ``f`` at the position read instead is outside the bound."""
    channels, shape = TRILINEAR_CASES[name]
    mapping = rotation_mapping(shape)
    generator = torch.Generator().manual_seed(30)
    sample = torch.stack([torch.randint(0, s, (samples,), generator=generator) for s in shape], dim=1)
    per_channel = shape[0] * shape[1] * shape[2]
    modulus = {"2^30 elements": 2**30, "2^32 bytes": 2**32 // 4}[wrap]
    touched = broken = 0
    for channel in range(channels):
        f, bound, interior, x = trilinear_reference(mapping, shape, channel, slice(None), "cpu", sample=sample)
        corner = [xr.floor().long() for xr in x]
        flat = channel * per_channel + (corner[0] * shape[1] + corner[1]) * shape[2] + corner[2]
        wrapped = flat % modulus
        moved = interior & (wrapped != flat)
        read_channel, rest = wrapped // per_channel, wrapped % per_channel
        read = [rest // (shape[1] * shape[2]), rest // shape[2] % shape[1], rest % shape[2]]
        position = [xr - c + r for xr, c, r in zip(x, corner, read)]
        value = read_channel + position[0] / shape[0] + 2 * position[1] / shape[1] + 4 * position[2] / shape[2]
        touched += int(moved.sum())
        broken += int((moved & ((value - f).abs() > bound)).sum())
    return touched, broken
