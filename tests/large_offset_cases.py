"""Shapes, analytic inputs, threshold crossings and slicing for the tests that run an entry point on a tensor whose offsets
pass 2^31 bytes, 2^32 bytes, 2^31 elements and (one-byte types) 2^32 elements (a plain module, no tests in it; importing it
needs no GPU).

Inputs are FUNCTIONS OF THE POSITION, built on the device from broadcast ``torch.arange`` terms, so no multi-GiB tensor crosses
the bus and an expected value can be rebuilt for any slice.  A wrapped index reads the value of another position: the
"distinct" form has periods 251 / 241 / 239 / 233 along i / j / k / the batch-channel index, all prime and none a divisor of
2^31 or 2^32, so a read that is off by a power of two (in elements or in bytes) sees another value on nearly every voxel.

Shapes keep the channel volume near 2^26 voxels and take many batch-channel slices.  Extents are no powers of two, so every
crossing falls strictly inside a K-row (``crossings`` asserts it): a kernel that handles rows, planes or channels in 64 bits
but narrows the offset inside one is then still caught.  K is a multiple of 4 (the fused stencil needs it).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

VOLUME = (400, 404, 420)  # 67 872 000 voxels = 2^26 * 1.011; 2^31 and 2^32 are multiples of none of 400, 404, 420
STENCIL_VOLUME = (516, 520, 252)  # 67 616 640 voxels; K <= 256 and K % 4 == 0: the fused J + K pass takes it (stencil.hip: plan_conv)
BYTE_SLICES = (13, 5)  # one-byte types: 65 batch-channel slices = 4 411 680 000 elements, beyond 2^32
FLOAT_SLICES = (17, 1)  # float32 past 2^32 bytes: 1 153 824 000 elements = 4.3 GiB
FLOAT_WIDE_SLICES = (11, 3)  # float32-only operations: 2 239 776 000 elements, beyond 2^31 (8.3 GiB)
WINDOW = 4096
SLICE_LIMIT = 2**31  # bytes: every operand of a sliced call stays below it
MEMORY_CAP_GIB = 48


def shape_for(dtype: torch.dtype, wide: bool = False, volume: Sequence[int] = VOLUME) -> tuple[int, ...]:
    if dtype.itemsize == 1:
        return (*BYTE_SLICES, *volume)
    return (*(FLOAT_WIDE_SLICES if wide else FLOAT_SLICES), *volume)


# -- inputs ----------------------------------------------------------------------------------------------------------------
def _terms(shape, device):
    """The four index vectors (batch-channel, i, j, k), shaped to broadcast over ``(B, C, I, J, K)``."""
    batch, channels, extent_i, extent_j, extent_k = shape
    arange = lambda n: torch.arange(n, device=device)  # noqa: E731
    return (arange(batch * channels).reshape(batch, channels, 1, 1, 1), arange(extent_i).reshape(1, 1, -1, 1, 1),
            arange(extent_j).reshape(1, 1, 1, -1, 1), arange(extent_k).reshape(1, 1, 1, 1, -1))


def distinct(shape: Sequence[int], dtype: torch.dtype, device, first_slice: int = 0) -> torch.Tensor:
    """``(i*7 % 251) + (j*13 % 241) + (k*31 % 239) + (bc*17 % 233)`` in *dtype* (0 .. 960; one-byte sums wrap and stay a function
    of the position).  The terms are cast BEFORE they are broadcast: nothing wider than the result is ever allocated.
    ``first_slice``: the batch-channel index of the tensor's first slice (to rebuild a part of a larger tensor)."""
    bc, i, j, k = _terms(shape, device)
    parts = [(bc + first_slice) * 17 % 233, i * 7 % 251, j * 13 % 241, k * 31 % 239]
    out = parts[0].to(dtype)
    for part in parts[1:]:
        out = out + part.to(dtype)
    return out.contiguous()


def affine_field(shape: Sequence[int], device, dtype=torch.float32, first_slice: int = 0) -> torch.Tensor:
    """``f = bc + i/I + 2j/J + 4k/K``: trilinear interpolation of it is ``f`` at the sample coordinate."""
    bc, i, j, k = _terms(shape, device)
    _, _, extent_i, extent_j, extent_k = shape
    out = (bc + first_slice).to(dtype) + i.to(dtype) / extent_i
    out = out + 2 * j.to(dtype) / extent_j
    return (out + 4 * k.to(dtype) / extent_k).contiguous()


# -- thresholds ------------------------------------------------------------------------------------------------------------
def thresholds(numel: int, itemsize: int) -> list[tuple[str, int]]:
    """``(name, element index)`` of the first element AT each threshold the tensor reaches, in ascending order."""
    found = {}
    for name, element in (("2^31 bytes", 2**31 // itemsize), ("2^32 bytes", 2**32 // itemsize), ("2^31 elements", 2**31), ("2^32 elements", 2**32)):
        if element < numel:
            found.setdefault(element, name)  # (one-byte types: bytes and elements coincide)
    return [(name, element) for element, name in sorted(found.items())]


def crossings(shape: Sequence[int], dtype: torch.dtype) -> list[tuple[str, int, tuple[int, int, int, int]]]:
    """``(name, element, (bc, i, j, k))`` of each threshold of a dense ``(B, C, I, J, K)`` tensor.  Asserts that the step onto it
    is a step inside a K-row, away from the row's ends."""
    batch, channels, extent_i, extent_j, extent_k = shape
    found = []
    for name, element in thresholds(math.prod(shape), dtype.itemsize):
        bc, rest = divmod(element, extent_i * extent_j * extent_k)
        i, rest = divmod(rest, extent_j * extent_k)
        j, k = divmod(rest, extent_k)
        assert 0 < k < extent_k - 1, f"{name} of {tuple(shape)} falls on a row boundary (k = {k})"
        assert bc < batch * channels
        found.append((name, element, (bc, i, j, k)))
    return found


def crossing_slices(shape: Sequence[int], dtype: torch.dtype) -> list[int]:
    """The batch-channel slices that contain a crossing, plus the first and the last one."""
    return sorted({0, shape[0] * shape[1] - 1, *(where[0] for _, _, where in crossings(shape, dtype))})


def windows(shape: Sequence[int], dtype: torch.dtype) -> list[tuple[str, int, int]]:
    """``(name, start, stop)`` of the flat index ranges to look at closely: WINDOW elements centred on each crossing, the first
    and the last WINDOW elements.  Starts are multiples of 4 (a Philox block holds four draws)."""
    numel = math.prod(shape)
    found = [("first", 0, min(WINDOW, numel)), ("last", (max(numel - WINDOW, 0) + 3) // 4 * 4, numel)]
    for name, element, _ in crossings(shape, dtype):
        found.append((name, element - WINDOW // 2, min(element + WINDOW // 2, numel)))
    assert all(start % 4 == 0 for _, start, _ in found)
    return found


# -- slicing ---------------------------------------------------------------------------------------------------------------
def batch_step(tensor: torch.Tensor, widest_itemsize: int) -> int:
    """How many batch elements of *tensor* one slice may hold when its widest operand has *widest_itemsize* bytes per voxel."""
    per_element = tensor[0].numel() * max(widest_itemsize, tensor.element_size())
    assert per_element < SLICE_LIMIT, f"one batch element needs {per_element} bytes: no slice stays below 2^31"
    return max(1, (SLICE_LIMIT - 1) // per_element)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """``torch.equal`` with the shapes and dtypes compared first."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def first_difference(a: torch.Tensor, b: torch.Tensor) -> str:
    """Where two tensors that should be equal first differ (for the assertion message; one pass over a chunked view)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    flat_a, flat_b = a.reshape(-1), b.reshape(-1)
    chunk = 2**28
    for begin in range(0, flat_a.numel(), chunk):
        differs = flat_a[begin : begin + chunk] != flat_b[begin : begin + chunk]
        if bool(differs.any()):
            at = begin + int(differs.nonzero()[0])
            return f"first difference at flat element {at} of {flat_a.numel()}: {flat_a[at].item()} against {flat_b[at].item()}"
    return "no difference (NaN?)"


# -- memory ----------------------------------------------------------------------------------------------------------------
def needs_gib(gib: float) -> None:
    """Skip (with both figures) when the device has less than *gib* GiB free; no test may ask for more than MEMORY_CAP_GIB."""
    import pytest

    assert gib <= MEMORY_CAP_GIB, f"a test may need at most {MEMORY_CAP_GIB} GiB, this one asks for {gib}"
    free, _ = torch.cuda.mem_get_info()
    if free < gib * 1024**3:
        pytest.skip(f"needs {gib:.0f} GiB of free device memory, {free / 1024**3:.1f} GiB are free")


def release() -> None:
    import gc

    gc.collect()
    torch.cuda.empty_cache()


# -- the Philox reference at an offset -----------------------------------------------------------------------------------------
def philox_window(seed: int, stream_id: int, start: int, stop: int) -> torch.Tensor:
    """Float64 normals of the elements ``start .. stop - 1`` of the stream (``intensity_pointwise_cases``' numpy Philox and its
    Box-Muller, evaluated at blocks ``start / 4 ...`` instead of from zero)."""
    from intensity_pointwise_cases import philox4x32_10

    assert start % 4 == 0
    blocks = np.arange(start // 4, (stop + 3) // 4, dtype=np.uint64)
    low, shift = np.uint64(0xFFFFFFFF), np.uint64(32)
    words = philox4x32_10((blocks & low, blocks >> shift, np.full_like(blocks, stream_id), np.zeros_like(blocks)),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    uniforms = [((word >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-24) for word in words]
    z = np.empty((blocks.size, 4), dtype=np.float64)
    for half in range(2):
        u1, u2 = uniforms[2 * half].astype(np.float64), uniforms[2 * half + 1].astype(np.float64)
        radius = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * half] = radius * np.cos(2.0 * np.pi * u2)
        z[:, 2 * half + 1] = radius * np.sin(2.0 * np.pi * u2)
    return torch.from_numpy(z.reshape(-1)[: stop - start].copy()) + 0.0
