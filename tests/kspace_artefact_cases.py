"""Inputs, case tables and float64 restatements shared by the Ghosting / Spike tests (a plain module, no tests).

The restatements go through the FFT ROUTE in numpy float64, written from the transforms' definitions: ``fftn`` over the three
spatial axes, ``fftshift``, the line mask (Ghosting) or the added points (Spike), ``ifftshift``, ``ifftn``, real part.  They
are the independent yardstick for the closed forms the engine computes (``csrc/kspace_artefacts.hip``), which never form a
spectrum.  ``tests/test_kspace_artefacts_host.py`` holds them against the golden file made from the reference itself
(``tests/golden/make_golden_kspace_artefacts.py``); the GPU tests compare the engine with them.
"""
from __future__ import annotations

import functools
import warnings

import numpy as np
import torch

GOLDEN_SEED = 41
FLOAT_BAR = 1e-5  # |d| <= FLOAT_BAR * max|expected|: the bar of test_kspace_segment_mix_matches_the_fft_route
#: one rounding step of the storage type on top of the float bar: half an ulp at max|expected|
STORAGE_STEP = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
AXES = (0, 1, 2)


# -- seeded inputs -------------------------------------------------------------------------------------------------------
def randn(shape, seed, scale=1.0, shift=0.0) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


@functools.lru_cache(maxsize=None)
def signed_image(shape: tuple, seed: int = GOLDEN_SEED) -> torch.Tensor:
    """``N(0, 40)`` plus a slow wave that outweighs the mean: the spectrum's peak is NOT the DC term (do not modify: cached)."""
    grid = torch.arange(shape[-3], dtype=torch.float32).view(-1, 1, 1)
    wave = 60.0 * torch.cos(2 * torch.pi * grid / max(shape[-3], 1) + 0.3)
    return randn(shape, seed, 40.0, 1.0) + (wave if shape[-3] > 2 else 0.0)


@functools.lru_cache(maxsize=None)
def positive_image(shape: tuple, seed: int = GOLDEN_SEED) -> torch.Tensor:
    """Uniform in [20, 200), float32: the peak is the DC term, the sum of the voxels (do not modify: cached)."""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 180.0 + 20.0


def typed_positive(shape: tuple, dtype: torch.dtype, seed: int = GOLDEN_SEED) -> torch.Tensor:
    """Positive, integer-scale values every dtype holds: whole numbers in [20, 200) for the integer types."""
    image = positive_image(tuple(shape), seed)
    if dtype == torch.float64:
        return image.double() + 2.0**-30  # (more bits than float32 keeps: the transforms drop them first)
    return image.floor().to(dtype) if not dtype.is_floating_point else image.to(dtype)


# -- Ghosting ------------------------------------------------------------------------------------------------------------
def brute_force_scaled(size: int, num_ghosts: int, restore: float) -> list[int]:
    """SHIFTED indices whose plane the reference scales, index by index: a multiple of ``step`` that is not in the restored
    window — the window taken by slicing ``range(size)``, so a start below zero counts from the end as in the reference."""
    step = max(size // num_ghosts, 1)
    restored: set[int] = set()
    if restore > 0:
        mid = size // 2
        half = max(int(size * restore / 2), 1)
        restored = set(range(size)[mid - half : mid + half])
    return [u for u in range(size) if u % step == 0 and u not in restored]


def reference_line_mask(size: int, num_ghosts: int, strength: float, restore: float, *, float32_mask: bool = True) -> np.ndarray:
    """The reference's mask over SHIFTED indices as float64 values (it stores ``1 - strength`` in float32)."""
    mask = np.ones(size)
    value = 1.0 - strength
    mask[brute_force_scaled(size, num_ghosts, restore)] = float(np.float32(value)) if float32_mask else value
    return mask


def ghost_fft(data: torch.Tensor, axes, masks) -> np.ndarray:
    """float64 ``(B, C, I, J, K)``: element ``b``'s shifted spectrum times ``masks[b]`` along ``axes[b]`` and back; ``None``
    leaves the element as it is.  The input is taken as float32 first, as the reference does."""
    x = data.float().double().numpy()
    out = x.copy()
    for b, (axis, mask) in enumerate(zip(axes, masks, strict=True)):
        if mask is None:
            continue
        spectrum = np.fft.fftshift(np.fft.fftn(x[b], axes=(-3, -2, -1)), axes=(-3, -2, -1))
        view = [1, 1, 1, 1]
        view[axis + 1] = -1
        spectrum = spectrum * np.asarray(mask, dtype=np.float64).reshape(view)
        out[b] = np.fft.ifftn(np.fft.ifftshift(spectrum, axes=(-3, -2, -1)), axes=(-3, -2, -1)).real
    return out


def mask_from_frequencies(size: int, frequencies, strength: float) -> np.ndarray:
    """A SHIFTED mask that scales the UNSHIFTED ``frequencies`` by ``1 - strength`` each time they are listed."""
    mask = np.ones(size)
    for f in frequencies:
        mask[(f + size // 2) % size] -= strength
    return mask


def ghost_expected_from_params(data: torch.Tensor, params: dict) -> np.ndarray:
    """The FFT route for a recorded parameter dictionary of ``Ghosting`` (shared or per element)."""
    batch = data.shape[0]
    if "_batched_keys" in params:
        ghosts, axes, strengths = params["num_ghosts"], params["axis"], params["intensity"]
    else:
        ghosts, axes, strengths = [params["num_ghosts"]] * batch, [params["axis"]] * batch, [params["intensity"]] * batch
    masks = [
        reference_line_mask(data.shape[2 + axis], n, s, params["restore"]) if n and s != 0 else None
        for n, axis, s in zip(ghosts, axes, strengths, strict=True)
    ]
    return ghost_fft(data, axes, masks)


# -- Spike ---------------------------------------------------------------------------------------------------------------
def spike_fft(data: torch.Tensor, index_lists, intensities) -> tuple[np.ndarray, np.ndarray]:
    """float64 ``(B, C, I, J, K)`` and the ``(B, C)`` peaks: ``peak * intensities[b]`` added at the SHIFTED indices
    ``index_lists[b]`` of element ``b``'s spectrum (as often as listed), and back.  Empty list or zero intensity: untouched."""
    x = data.float().double().numpy()
    out = x.copy()
    peaks = np.zeros(x.shape[:2])
    for b, (indices, intensity) in enumerate(zip(index_lists, intensities, strict=True)):
        spectrum = np.fft.fftshift(np.fft.fftn(x[b], axes=(-3, -2, -1)), axes=(-3, -2, -1))
        peaks[b] = np.abs(spectrum).max(axis=(-3, -2, -1))
        if not indices or intensity == 0:
            continue
        for i, j, k in indices:
            spectrum[:, i, j, k] += peaks[b] * intensity
        out[b] = np.fft.ifftn(np.fft.ifftshift(spectrum, axes=(-3, -2, -1)), axes=(-3, -2, -1)).real
    return out, peaks


def shifted_indices(positions, shape) -> list[tuple[int, int, int]]:
    return [tuple(int(p * s) % s for p, s in zip(position, shape, strict=True)) for position in positions]


def unshifted(indices, shape) -> list[tuple[int, int, int]]:
    return [tuple((u - s // 2) % s for u, s in zip(index, shape, strict=True)) for index in indices]


def spike_expected_from_params(data: torch.Tensor, params: dict) -> np.ndarray:
    batch, shape = data.shape[0], tuple(data.shape[2:])
    if "_batched_keys" in params:
        positions, intensities = params["positions"], params["intensity"]
    else:
        positions, intensities = [params["positions"]] * batch, [params["intensity"]] * batch
    return spike_fft(data, [shifted_indices(p, shape) for p in positions], intensities)[0]


# -- bars ----------------------------------------------------------------------------------------------------------------
def integer_result(expected: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """``.to(dtype)`` of an exact result: truncated toward zero."""
    return torch.from_numpy(np.trunc(expected)).to(dtype)


def check(got: torch.Tensor, expected: np.ndarray, what: str = "") -> None:
    """The issue's bars.  Float dtypes: ``|d| <= 1e-5 * max|expected|`` plus half an ulp of the storage type there.  Integer
    dtypes: ``|d| <= 1`` and at most a share ``2 * 1e-5 * max|expected|`` of the voxels different — the share the float bar
    itself lets cross a whole number."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(expected.shape), (what, got.shape, expected.shape)
    top = float(np.abs(expected).max()) if expected.size else 0.0
    if got.dtype.is_floating_point:
        worst = float(np.abs(got.double().numpy() - expected).max()) if expected.size else 0.0
        bar = (FLOAT_BAR + STORAGE_STEP[got.dtype]) * top
        print(f"{what}: max|d| = {worst:.3e}, bar = {bar:.3e} (max|expected| = {top:.4g})")
        assert worst <= bar, (what, worst, bar)
        return
    difference = (got.double() - integer_result(expected, got.dtype).double()).abs()
    share, cap = float((difference != 0).double().mean()), 2 * FLOAT_BAR * top
    print(f"{what}: max|d| = {float(difference.max()):.0f}, share = {share:.3e}, cap = {cap:.3e} ({got.numel()} voxels)")
    assert got.numel() >= 4000, "an integer case has at least 4000 voxels"
    assert float(difference.max()) <= 1 and share <= cap, (what, float(difference.max()), share, cap)


# -- the golden cases ----------------------------------------------------------------------------------------------------
#: The integer cases' shape: 5491 voxels.  The share cap of `check` counts on results whose fractional parts are spread out.
#: Where the step between scaled planes divides the axis (16 / 4, 15 / 3) the planes form a comb and the correction is the
#: strength over the step times a sum of whole numbers; on a 16-voxel axis Spike's phase hits a quarter turn (cosine exactly
#: zero) on an eighth of the voxels.  Both leave results that are whole numbers in exact arithmetic, which any rounding error
#: truncates either way.  With 17 and 19 voxels (steps of 4 that divide neither, no quarter turns) neither happens.
INTEGER_SHAPE = (17, 19, 17)
#: name -> (class arguments, batch, spatial shape, image dtype, seed of the global generator, input kind)
GHOST_CASES = {
    "ghost_shared": ({"intensity": 0.7, "per_instance": False}, 2, (12, 9, 7), torch.float32, 51, "signed"),
    "ghost_per_instance": ({"intensity": (0.3, 0.9), "num_ghosts": (2, 6)}, 3, (12, 9, 7), torch.float32, 52, "signed"),
    "ghost_gated": ({"intensity": (0.5, 1.0), "p": 0.5}, 6, (8, 7, 6), torch.float32, 53, "signed"),
    "ghost_restore_thin": ({"intensity": 0.8, "restore": 0.02, "axes": (0,)}, 1, (16, 8, 8), torch.float32, 54, "signed"),
    "ghost_restore_half": ({"intensity": 0.8, "restore": 0.5, "num_ghosts": 8, "axes": (0,)}, 1, (16, 8, 8), torch.float32, 55, "signed"),
    "ghost_restore_all": ({"intensity": 0.8, "restore": 1.0, "num_ghosts": 8, "axes": (0,)}, 1, (16, 8, 8), torch.float32, 56, "signed"),
    "ghost_restore_wraps": ({"intensity": 0.8, "restore": 1.5, "num_ghosts": 8, "axes": (0,)}, 1, (16, 8, 8), torch.float32, 57, "signed"),
    "ghost_every_plane": ({"intensity": 0.6, "num_ghosts": 40, "axes": (1,)}, 1, (5, 33, 6), torch.float32, 58, "positive"),
    "ghost_axis_of_one": ({"intensity": 0.6, "axes": (0,)}, 1, (1, 4, 9), torch.float32, 59, "positive"),
    "ghost_odd_last_axis": ({"intensity": 0.9, "axes": (2,)}, 2, (7, 6, 65), torch.float32, 60, "signed"),
    "ghost_int16": ({"intensity": 0.05}, 1, INTEGER_SHAPE, torch.int16, 61, "positive"),
    "ghost_uint8": ({"intensity": 0.05}, 1, INTEGER_SHAPE, torch.uint8, 62, "positive"),
    "ghost_noop": ({}, 2, (4, 5, 6), torch.float32, 63, "signed"),
}
SPIKE_CASES = {
    "spike_shared": ({"intensity": 1.5, "per_instance": False}, 2, (12, 9, 7), torch.float32, 71, "signed"),
    "spike_per_instance": ({"num_spikes": (1, 6), "intensity": (-2.0, 2.0)}, 3, (12, 9, 7), torch.float32, 72, "signed"),
    "spike_gated": ({"intensity": (1.0, 3.0), "p": 0.5}, 6, (8, 7, 6), torch.float32, 73, "signed"),
    "spike_positive": ({"num_spikes": 3, "intensity": -0.8}, 2, (5, 33, 6), torch.float32, 74, "positive"),
    "spike_axis_of_one": ({"intensity": 0.5}, 1, (1, 4, 9), torch.float32, 75, "positive"),
    "spike_int16": ({"intensity": 0.05, "num_spikes": 2}, 1, INTEGER_SHAPE, torch.int16, 76, "positive"),
    "spike_uint8": ({"intensity": 0.05, "num_spikes": 2}, 1, INTEGER_SHAPE, torch.uint8, 77, "positive"),
    "spike_noop": ({}, 2, (4, 5, 6), torch.float32, 78, "signed"),
}
CASES = [*GHOST_CASES, *SPIKE_CASES]


def case_input(name: str) -> torch.Tensor:
    _, batch, shape, dtype, seed, kind = (GHOST_CASES if name in GHOST_CASES else SPIKE_CASES)[name]
    full = (batch, 1, *shape)
    return typed_positive(full, dtype, seed) if kind == "positive" else signed_image(full, seed).to(dtype)


def case_transform(tio, name: str):
    if name in GHOST_CASES:
        return tio.Ghosting(**GHOST_CASES[name][0])
    return tio.Spike(**SPIKE_CASES[name][0])


def case_seed(name: str) -> int:
    return (GHOST_CASES if name in GHOST_CASES else SPIKE_CASES)[name][4]


def make_batch(tio, image: torch.Tensor, device: str = "cpu"):
    subjects = [tio.Subject(t1=tio.ScalarImage(image[b].clone())) for b in range(image.shape[0])]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    return batch if device == "cpu" else batch.to(device)


def construct(tio, name: str):
    """The transform and the warnings of its constructor."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        transform = case_transform(tio, name)
    return transform, [str(w.message) for w in caught]


def run_case(tio, name: str, device: str = "cpu"):
    """The case through ``tio`` (the reference or this package): ``(output tensor, recorded params, history name,
    constructor warnings, the call's warnings)``."""
    transform, built = construct(tio, name)
    batch = make_batch(tio, case_input(name), device)
    torch.manual_seed(case_seed(name))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = transform(batch)
    record = out.applied_transforms[-1] if out.applied_transforms else None
    return (out.images["t1"].data, None if record is None else record.params, None if record is None else record.name, built,
            [str(w.message) for w in caught])


def expected_for(name: str, params: dict) -> np.ndarray:
    image = case_input(name)
    return ghost_expected_from_params(image, params) if name in GHOST_CASES else spike_expected_from_params(image, params)


# -- the GPU tests' shapes -----------------------------------------------------------------------------------------------
SHAPES = [(2, 2, 12, 9, 7), (1, 1, 16, 8, 8), (1, 1, 5, 33, 6), (1, 1, 7, 6, 65), (1, 1, 1, 4, 9), (1, 1, 70, 3, 130)]
