"""Inputs and torch-CPU restatements shared by the Normalize / Standardize / Clamp / Mask tests (a plain module, no tests).

The restatements are the reference's own expressions (``transforms/_statistics.py``, ``transforms/intensity/normalize.py``,
``standardize.py``, ``clamp.py``, ``mask.py``) on CPU tensors; ``tests/test_intensity_stats_host.py`` holds them against
the golden file made from the reference itself, and the GPU tests compare the engine with them.

``CASES`` is the list of golden cases: what ``tests/golden/make_golden_intensity_stats.py`` runs through the reference and
the GPU test through this package — the same constructor arguments for both.
"""
from __future__ import annotations

import functools
import math

import torch

import label_cases

GOLDEN_SHAPE = (2, 2, 4, 5, 35)
GOLDEN_SEED = 7


@functools.lru_cache(maxsize=None)
def golden_image() -> torch.Tensor:
    """``N(20, 40)`` float32 of ``GOLDEN_SHAPE`` (do not modify: cached)."""
    generator = torch.Generator().manual_seed(GOLDEN_SEED)
    return torch.randn(GOLDEN_SHAPE, generator=generator) * 40.0 + 20.0


@functools.lru_cache(maxsize=None)
def golden_labels() -> torch.Tensor:
    """An int16 label map of the values 0..3, one channel (do not modify: cached)."""
    return label_cases.label_field((GOLDEN_SHAPE[0], 1, *GOLDEN_SHAPE[2:]), GOLDEN_SEED).to(torch.int16)


def above_twenty(x: torch.Tensor) -> torch.Tensor:
    """A callable mask without a reduction in it (a reduction's last bit could move a voxel across the threshold)."""
    return x > 20.0


#: name -> (class name, constructor arguments, seed of the global generator in front of the call)
CASES = {
    "normalize_default": ("Normalize", {}, 11),
    "normalize_0_255": ("Normalize", {"out_min": 0.0, "out_max": 255.0, "per_instance": False}, 12),
    "normalize_ct_window": ("Normalize", {"out_min": 0.0, "out_max": 1.0, "in_min": -20.0, "in_max": 60.0, "per_instance": False}, 13),
    "normalize_percentiles_key_mask": ("Normalize", {"percentile_low": 0.5, "percentile_high": 99.5, "masking_method": "seg"}, 14),
    "normalize_callable_mask": ("Normalize", {"percentile_low": 1.0, "percentile_high": 97.0, "masking_method": above_twenty}, 15),
    "normalize_per_instance": ("Normalize", {"out_min": (-1.0, 0.0), "out_max": (0.5, 1.0), "percentile_low": (0.0, 2.0)}, 16),
    "standardize_plain": ("Standardize", {}, 17),
    "standardize_masked": ("Standardize", {"masking_method": "seg"}, 18),
    "clamp_one_bound": ("Clamp", {"out_min": 0.0}, 19),
    "clamp_both_bounds": ("Clamp", {"out_min": -10.0, "out_max": 50.5}, 20),
    "mask_by_key": ("Mask", {"masking_method": "seg"}, 21),
    "mask_labels": ("Mask", {"masking_method": "seg", "labels": [1, 3], "outside_value": -7}, 22),
}
#: the cases whose history is also replayed backwards on their output
INVERSES = ["normalize_0_255", "standardize_masked"]
#: replayed on the golden image itself: one per-instance element with out_min == out_max, which stays as it is
ZERO_RANGE_INVERSE = {"out_min": [-1.0, 0.5], "out_max": [1.0, 0.5], "in_ranges": {"t1": (-3.5, 41.25)}, "_batch_size": 2,
                      "_batched_keys": ["out_min", "out_max"]}


def run_case(tio, name: str, device: str = "cpu"):
    """The case through ``tio`` (the reference or this package): ``(output batch, recorded params, history name)``."""
    class_name, arguments, seed = CASES[name]
    subjects = [tio.Subject(t1=tio.ScalarImage(golden_image()[b].clone()), seg=tio.LabelMap(golden_labels()[b].clone())) for b in range(GOLDEN_SHAPE[0])]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    if device != "cpu":
        batch = batch.to(device)
    torch.manual_seed(seed)
    out = getattr(tio, class_name)(**arguments)(batch)
    record = out.applied_transforms[-1]
    return out, record.params, record.name


# -- selection and quantiles ---------------------------------------------------------------------------------------------
def inside_values(element: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    """``tensor[mask.expand_as(tensor)]`` / ``tensor.reshape(-1)`` as float32 (normalize.py:352, :363)."""
    values = element[mask.bool().expand_as(element)] if mask is not None else element.reshape(-1)
    return values.float()


def order_statistics(values: torch.Tensor, q: float):
    """``(lower_value, upper_value)``: the ``(lower + 1)``-th and ``(lower + 2)``-th smallest by ``torch.kthvalue``."""
    n = values.numel()
    lower = math.floor(q * (n - 1))
    return torch.kthvalue(values, lower + 1).values, torch.kthvalue(values, min(lower + 2, n)).values


def compute_quantile(values: torch.Tensor, q: float) -> float:
    """_statistics.py:36-43."""
    index = q * (values.numel() - 1)
    lower = math.floor(index)
    lower_value = torch.kthvalue(values, lower + 1).values
    if index == lower:
        return float(lower_value.item())
    upper_value = torch.kthvalue(values, lower + 2).values
    return float(lower_value.lerp(upper_value, index - lower).item())


def percentile_range(element, mask, pct_low, pct_high):
    """normalize.py:352-365 (the empty mask falls back to every voxel)."""
    values = inside_values(element, mask)
    if values.numel() == 0:
        values = inside_values(element, None)
    return compute_quantile(values, pct_low / 100.0), compute_quantile(values, pct_high / 100.0)


# -- the elementwise halves ----------------------------------------------------------------------------------------------
def _out_min_and_range(out_min, out_max):
    if isinstance(out_min, list):
        min_b = torch.tensor(out_min, dtype=torch.float32).view(-1, 1, 1, 1, 1)
        max_b = torch.tensor(out_max, dtype=torch.float32).view(-1, 1, 1, 1, 1)
        return min_b, max_b - min_b
    return out_min, out_max - out_min


def normalize(data, in_min, in_max, out_min, out_max):
    """normalize.py:167-183."""
    in_range = in_max - in_min
    data = data.float()
    low, out_range = _out_min_and_range(out_min, out_max)
    data = data.clamp(in_min, in_max)
    return (data - in_min) / in_range * out_range + low


def normalize_inverse(data, in_min, in_max, out_min, out_max):
    """normalize.py:274-299."""
    in_range = in_max - in_min
    data = data.float()
    low, out_range = _out_min_and_range(out_min, out_max)
    if isinstance(out_range, float):
        return (data - low) / out_range * in_range + in_min
    zero = out_range == 0
    safe = torch.where(zero, torch.ones_like(out_range), out_range)
    return torch.where(zero, data, (data - low) / safe * in_range + in_min)


def standardize(data, mean, std):
    """standardize.py:97."""
    return (data.float() - mean) / std


def standardize_inverse(data, mean, std):
    """standardize.py:138."""
    return data.float() * std + mean


def clamp(data, out_min=None, out_max=None):
    """clamp.py:56."""
    return data.clamp(min=out_min, max=out_max)


def mask_where(data, mask, outside_value):
    """mask.py:69-70."""
    return torch.where(mask.bool().expand_as(data), data, outside_value)


def label_mask(labels_element, labels=None):
    """mask.py:91-97."""
    if labels is None:
        return labels_element.bool()
    mask = torch.zeros_like(labels_element, dtype=torch.bool)
    for label in labels:
        mask = mask | (labels_element == label)
    return mask


# -- float32 ulps --------------------------------------------------------------------------------------------------------
def ulps_off(value: float, exact: float) -> float:
    """``|value - exact|`` in units of the float32 spacing at ``exact`` (a normal number)."""
    return abs(value - exact) / 2.0 ** (math.floor(math.log2(abs(exact))) - 23)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same dtype, shape and values, NaN where NaN; ``==`` on the rest, so -0 and +0 agree."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())
