"""Inputs and torch-CPU restatements shared by the Swap / HistogramStandardization tests (a plain module, no tests).

The restatements are written from the transforms' definitions, not copied: the swap as the sequential loop over patch
slices AND, independently, as the backward trace of every output voxel through the swaps; the standardization as
``np.percentile`` -> float32 table -> ``torch.bucketize`` -> map; the landmark training as the averaged lines through the
cutoff percentiles.  ``tests/test_swap_histogram_host.py`` holds them against the golden file made from the reference itself
(``tests/golden/make_golden_swap_histogram.py``), and the GPU tests compare the engine with them.

``CASES`` lists the golden cases; ``run_case(tio, name, device)`` runs one through the reference or through this package.
"""
from __future__ import annotations

import functools
import itertools
import sys
import warnings

import numpy as np
import torch

import label_cases

GOLDEN_SEED = 23
DEFAULT_QUANTILES = (0.01, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.99)
WIDE_QUANTILES = (0.01, 0.02, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.98, 0.99)
ALL_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]


# -- seeded inputs -------------------------------------------------------------------------------------------------------
def randn(shape, seed, scale=1.0, shift=0.0) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


@functools.lru_cache(maxsize=None)
def golden_image(batch: int, shape: tuple, channels: int = 1, seed: int = GOLDEN_SEED) -> torch.Tensor:
    """``N(20, 40)`` float32 ``(batch, channels, *shape)`` (do not modify: cached)."""
    return randn((batch, channels, *shape), seed, 40.0, 20.0)


def above_twenty(x: torch.Tensor) -> torch.Tensor:
    return x > 20.0


def landmarks_for(quantiles) -> torch.Tensor:
    """Uneven, increasing standard-space landmarks, one per quantile."""
    steps = torch.tensor([3.0 + (k * 7) % 5 for k in range(len(quantiles))])
    values = torch.cumsum(steps, 0)
    return (values - values[0]) / (values[-1] - values[0]) * 100.0


#: name -> (class arguments, batch, spatial shape, seed of the global generator, with a label map)
SWAP_CASES = {
    "swap_default_per_instance": ({}, 2, (16, 17, 18), 31, False),  # patch 15, 100 iterations
    "swap_shared": ({"patch_size": (3, 4, 5), "num_iterations": 10, "per_instance": False}, 2, (9, 10, 13), 32, False),
    "swap_iteration_range": ({"patch_size": 2, "num_iterations": (2, 9)}, 2, (9, 10, 13), 33, False),
    "swap_gated": ({"patch_size": 3, "num_iterations": 5, "p": 0.5}, 6, (7, 8, 9), 34, False),
    "swap_all_pairs_overlap": ({"patch_size": (3, 4, 4), "num_iterations": 30, "per_instance": False}, 2, (5, 6, 7), 35, False),
    "swap_patch_spans_an_axis": ({"patch_size": (3, 10, 4), "num_iterations": 8}, 2, (9, 10, 13), 36, False),
    "swap_with_label_map": ({"patch_size": 3, "num_iterations": 6}, 2, (9, 10, 13), 37, True),
}
#: name -> (image dtype, batch, channels, spatial shape, cutoff or None, constructor extras)
HISTOGRAM_CASES = {
    "histogram_float32": (torch.float32, 2, 1, (9, 10, 13), None, {}),
    "histogram_int16": (torch.int16, 2, 1, (9, 10, 13), None, {}),
    "histogram_include": (torch.float32, 2, 2, (6, 7, 11), None, {"include": ["t1"]}),
    "histogram_wide_cutoff": (torch.float32, 2, 1, (9, 10, 13), (0.02, 0.98), {}),
}
LANDMARK_CASES = {"landmarks_plain": None, "landmarks_callable_mask": above_twenty}
CASES = [*SWAP_CASES, *HISTOGRAM_CASES, *LANDMARK_CASES]


def _batch(tio, images: dict, device: str):
    """``images``: name -> (image class, ``(B, C, I, J, K)`` tensor)."""
    count = next(iter(images.values()))[1].shape[0]
    subjects = [tio.Subject(**{name: image_class(data[b].clone()) for name, (image_class, data) in images.items()}) for b in range(count)]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    return batch if device == "cpu" else batch.to(device)


def swap_inputs(name: str):
    arguments, batch, shape, seed, with_labels = SWAP_CASES[name]
    image = golden_image(batch, shape)
    labels = label_cases.label_field((batch, 1, *shape), seed).to(torch.int16) if with_labels else None
    return arguments, image, labels, seed


def histogram_inputs(name: str):
    dtype, batch, channels, shape, cutoff, extras = HISTOGRAM_CASES[name]
    image = golden_image(batch, shape, channels)
    image = image.round().to(dtype) if not dtype.is_floating_point else image.to(dtype)
    other = golden_image(batch, shape, channels, GOLDEN_SEED + 1)
    quantiles = DEFAULT_QUANTILES if cutoff is None else WIDE_QUANTILES
    arguments = dict(extras) if cutoff is None else {"cutoff": cutoff, **extras}
    return arguments, image, other, landmarks_for(quantiles), quantiles


def training_images():
    """Three float32 ``(C, I, J, K)`` images of different spread."""
    return [randn((1, 9, 10, 13), 50 + k, 30.0 + 10 * k, 15.0 * k) for k in range(3)]


def run_case(tio, name: str, device: str = "cpu"):
    """The case through ``tio`` (the reference or this package).  Swap and HistogramStandardization cases:
    ``(output batch, recorded params, history name, warning messages)``; landmark cases: the landmarks tensor."""
    if name in LANDMARK_CASES:
        module = sys.modules[tio.HistogramStandardization.__module__]
        images = [tio.ScalarImage(image.clone() if device == "cpu" else image.to(device)) for image in training_images()]
        return module.compute_histogram_landmarks(images, masking_method=LANDMARK_CASES[name])
    if name in SWAP_CASES:
        arguments, image, labels, seed = swap_inputs(name)
        images = {"t1": (tio.ScalarImage, image)}
        if labels is not None:
            images["seg"] = (tio.LabelMap, labels)
        transform = tio.Swap(**arguments)
    else:
        arguments, image, other, landmarks, _ = histogram_inputs(name)
        images = {"t1": (tio.ScalarImage, image), "t2": (tio.ScalarImage, other)} if "include" in arguments else {"t1": (tio.ScalarImage, image)}
        seed = 0
        transform = tio.HistogramStandardization(landmarks.clone(), **arguments)
    batch = _batch(tio, images, device)
    torch.manual_seed(seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = transform(batch)
    record = out.applied_transforms[-1] if out.applied_transforms else None
    messages = [str(w.message) for w in caught]
    return out, None if record is None else record.params, None if record is None else record.name, messages


# -- Swap, twice ---------------------------------------------------------------------------------------------------------
def is_pair(entry) -> bool:
    return len(entry) == 2 and all(len(origin) == 3 and not hasattr(origin[0], "__len__") for origin in entry)


def location_lists(locations, batch: int):
    """One list of pairs per batch element (a shared list repeated)."""
    locations = list(locations)
    if all(is_pair(entry) for entry in locations):
        return [locations] * batch
    assert len(locations) == batch
    return locations


def swap_sequential(data: torch.Tensor, locations, patch) -> torch.Tensor:
    """The definition: per element, swap after swap, on all channels; both patches are read, A is written, then B."""
    out = data.clone()
    pi, pj, pk = patch
    for b, pairs in enumerate(location_lists(locations, data.shape[0])):
        for (ai, aj, ak), (bi, bj, bk) in pairs:
            first = out[b, :, ai : ai + pi, aj : aj + pj, ak : ak + pk].clone()
            second = out[b, :, bi : bi + pi, bj : bj + pj, bk : bk + pk].clone()
            out[b, :, ai : ai + pi, aj : aj + pj, ak : ak + pk] = second
            out[b, :, bi : bi + pi, bj : bj + pj, bk : bk + pk] = first
    return out


def swap_backward_trace(data: torch.Tensor, locations, patch) -> torch.Tensor:
    """The gather: every output voxel walks the swaps from the last to the first — inside B it came from A, else inside A
    it came from B — and takes the input's value where it ends."""
    out = torch.empty_like(data)
    shape = data.shape[2:]
    for b, pairs in enumerate(location_lists(locations, data.shape[0])):
        for voxel in itertools.product(*(range(s) for s in shape)):
            at = list(voxel)
            for a, c in reversed(pairs):
                if all(c[d] <= at[d] < c[d] + patch[d] for d in range(3)):
                    at = [at[d] + a[d] - c[d] for d in range(3)]
                elif all(a[d] <= at[d] < a[d] + patch[d] for d in range(3)):
                    at = [at[d] + c[d] - a[d] for d in range(3)]
            out[(b, slice(None), *voxel)] = data[(b, slice(None), *at)]
    return out


def random_locations(shape, patch, count: int, seed: int):
    """``count`` pairs of origins anywhere in range (overlapping or not)."""
    generator = torch.Generator().manual_seed(seed)
    highs = [s - p + 1 for s, p in zip(shape, patch, strict=True)]
    draw = lambda: tuple(int(torch.randint(h, (1,), generator=generator)) for h in highs)  # noqa: E731
    return [(draw(), draw()) for _ in range(count)]


# -- HistogramStandardization --------------------------------------------------------------------------------------------
def percentiles(values: torch.Tensor, quantiles) -> np.ndarray:
    """``np.percentile`` of the float32 values at ``100 q``: float64; NaN for no values."""
    array = values.float().reshape(-1).numpy()
    if array.size == 0:
        return np.full(len(quantiles), np.nan)
    with np.errstate(invalid="ignore"):
        return np.percentile(array, [100.0 * q for q in quantiles])


def inside_values(element: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    return (element[mask.bool().expand_as(element)] if mask is not None else element.reshape(-1)).float()


def standardize_element(element: torch.Tensor, landmarks: torch.Tensor, quantiles) -> torch.Tensor:
    """One ``(C, I, J, K)`` element: float32 table from its percentiles, ``bucketize``, map; the result in float32."""
    flat = element.float().reshape(-1)
    found = torch.as_tensor(percentiles(flat, quantiles), dtype=torch.float32)
    landmarks = landmarks.float()
    widths = found[1:] - found[:-1]
    widths = torch.where(widths.abs() < 1e-5, torch.tensor(float("inf")), widths)
    slopes = (landmarks[1:] - landmarks[:-1]) / widths
    intercepts = landmarks[:-1] - slopes * found[:-1]
    bins = torch.bucketize(flat, found[1:-1], right=False)
    return (slopes[bins] * flat + intercepts[bins]).reshape(element.shape)


def standardize(data: torch.Tensor, landmarks: torch.Tensor, quantiles) -> torch.Tensor:
    """Every batch element, assigned into a tensor of the input's dtype (as the reference assigns into ``data[i]``)."""
    out = data.clone()
    for b in range(data.shape[0]):
        out[b] = standardize_element(data[b], landmarks, quantiles)
    return out


def average_landmarks(database: np.ndarray) -> np.ndarray:
    """``(N, P)`` percentiles -> ``(P,)`` landmarks: each image's line through its first and last percentile onto
    [0, 100], the lines averaged (float64)."""
    low, high = database[:, 0], database[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        slopes = np.nan_to_num(100.0 / (high - low))
    offset = float(np.mean(0.0 - slopes * low))
    return slopes @ database / len(database) + offset


def train_landmarks(images, quantiles, mask_fn=None) -> torch.Tensor:
    rows = [percentiles(inside_values(image, None if mask_fn is None else mask_fn(image)), quantiles) for image in images]
    return torch.as_tensor(average_landmarks(np.vstack(rows)), dtype=torch.float32)


# -- the selection inputs of the intensity-statistics tests, rebuilt ------------------------------------------------------
ONE, TWO, EXACT, SMALL, BLOCKS = (1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 1, 1, 1, 101), (1, 2, 5, 6, 67), (1, 1, 33, 47, 67)


@functools.lru_cache(maxsize=None)
def selection_inputs():
    """name -> (data ``(B, C, I, J, K)``, mask ``(1 or C, I, J, K)`` or None), CPU tensors (do not modify: cached)."""
    n_small = 2 * 5 * 6 * 67
    half = randn(BLOCKS, 3)
    half.view(-1)[: half.numel() // 2] = 0.0
    half.view(-1)[1::3] = 0.0
    steps = (1.0 + torch.randperm(n_small, generator=torch.Generator().manual_seed(4)).double() * 2.0**-23).float().view(SMALL)
    nans = randn(SMALL, 6)
    nans.view(-1)[[0, 17, 1000, 4019]] = float("nan")
    labels = label_cases.label_field((1, 1, *SMALL[2:]), 1)[0].to(torch.int16)
    small = randn(SMALL, 1, 30.0, 5.0)
    return {
        "one_voxel_volume": (randn(ONE, 0), None),
        "two_voxels": (randn(TWO, 0), None),
        "ranks_on_data_values": (randn(EXACT, 9, 10.0), None),
        "small": (small, None),
        "many_blocks": (randn(BLOCKS, 2, 100.0), None),
        "all_equal": (torch.full(SMALL, 3.25), None),
        "half_exact_zeros": (half, None),
        "duplicates": (torch.randint(0, 5, BLOCKS, generator=torch.Generator().manual_seed(7)).float(), None),
        "last_digit_only": (steps, None),
        "a_few_nans": (nans, None),
        "mask_one_channel_int16": (small, labels),
        "mask_per_channel_bool": (small, torch.stack([labels[0] == 1, labels[0] >= 2])),
        "mask_no_voxel": (small, torch.zeros(1, *SMALL[2:], dtype=torch.int16)),
        "two_elements": (torch.cat([small, randn(SMALL, 12, 3.0, -40.0)]), None),
    }


def typed(shape, seed, dtype) -> torch.Tensor:
    """Values every dtype holds differently (integers across the dtype's range, float64 with more bits than float32 keeps)."""
    generator = torch.Generator().manual_seed(seed)
    if dtype == torch.float64:
        return torch.randn(shape, generator=generator, dtype=torch.float64) * 50 + 10
    if dtype.is_floating_point:
        return (torch.randn(shape, generator=generator) * 50 + 10).to(dtype)
    if dtype == torch.int64:
        return torch.randint(-(2**40), 2**40, shape, generator=generator)
    info = torch.iinfo(dtype)
    return torch.randint(max(info.min, -40000), min(info.max, 40000) + 1, shape, generator=generator).to(dtype)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same dtype, shape and values, NaN where NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def same_bits64(a, b) -> bool:
    """Two float64 arrays: equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
