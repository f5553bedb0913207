"""``Swap`` on the HIP engine (mirror of reference ``transforms/intensity/swap.py``).

The reference replays the swaps one after the other — two patch clones and two assignments each, on the per-instance
path through advanced-indexing gathers over index tensors: 400 small launches for the default 100 iterations.  Every swap
moves whole voxels, so the result is a gather from the input; ``tio_swap_patches`` computes it with one copy and one launch
whatever the number of swaps (``csrc/swap.hip``).  Same constructor, draw order, parameter dictionary, warning and error.
``make_params`` reads shapes only and never touches the device.
"""
from __future__ import annotations

import warnings
from typing import Any

import torch

from .. import ops
from ..data.batch import SubjectsBatch
from ..data.image import LabelMap
from .parameter_range import to_nonneg_range
from .transform import IntensityTransform

Origin = tuple[int, int, int]
SwapLocation = tuple[Origin, Origin]


class Swap(IntensityTransform):
    """Exchange the contents of randomly placed pairs of same-sized patches (swap.py:22-131), for context restoration.

    ``patch_size``: an integer ``n`` means ``(n, n, n)``.  ``num_iterations``: the number of pairs, or a ``(a, b)`` range it is
    drawn from.  With per-instance parameters every batch element gets its own pairs.  A subject with a ``LabelMap`` gets the
    reference's warning: its labels no longer match the swapped image.  Not invertible.
    """

    def __init__(self, *, patch_size: int | tuple[int, int, int] = 15, num_iterations: int | tuple[int, int] = 100, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if isinstance(patch_size, int):
            patch_size = (patch_size, patch_size, patch_size)
        self.patch_size = patch_size
        self.num_iterations = to_nonneg_range(num_iterations)

    @property
    def supports_per_instance_params(self) -> bool:
        return True

    @property
    def supports_per_instance_p(self) -> bool:
        return True

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        for img_batch in batch.images.values():
            if issubclass(img_batch._image_class, LabelMap):
                warnings.warn(
                    "Swap is applied to a subject containing LabelMap "
                    "images. The spatial rearrangement will make labels "
                    "inconsistent with the swapped image. This transform "
                    "is intended for self-supervised learning.",
                    stacklevel=2,
                )
                break
        any_img = next(iter(batch.images.values()))
        spatial_shape = tuple(int(s) for s in any_img.data.shape[2:])
        n = self._resolve_n(batch)
        if n is None:
            iterations = max(1, round(self.num_iterations.sample_1d()))
            return {"locations": _sample_swap_locations(spatial_shape, self.patch_size, iterations)}
        keep = self._keep_mask(batch, n)
        locations_list: list[Any] = []
        for index in range(n):
            if keep is not None and not keep[index]:
                locations_list.append([])
                continue
            iterations = max(1, round(self.num_iterations.sample_1d()))
            locations_list.append(_sample_swap_locations(spatial_shape, self.patch_size, iterations))
        params = {"locations": locations_list}
        self._tag_batched(params, batch, n, keep, ["locations"])
        return params

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for img_batch in self._get_images(batch).values():
            img_batch.data = ops.engine().swap_patches(img_batch.data, params["locations"], self.patch_size)
        return batch


def _sample_swap_locations(spatial_shape: tuple[int, ...], patch_size: tuple[int, int, int], num_iterations: int) -> list[SwapLocation]:
    """Pairs of origins (swap.py:134-167): the second one is redrawn up to 100 times until its patch clears the first's —
    the last draw stays when none does, so overlapping pairs occur once the patch is more than half the volume."""
    max_ini = [s - p for s, p in zip(spatial_shape, patch_size, strict=True)]
    if any(m < 0 for m in max_ini):
        raise ValueError(f"Patch size {patch_size} cannot be larger than spatial shape {tuple(spatial_shape)}")
    locations: list[SwapLocation] = []
    for _ in range(num_iterations):
        first = _random_origin(max_ini)
        for _ in range(100):
            second = _random_origin(max_ini)
            if not _patches_overlap(first, second, patch_size):
                break
        locations.append((first, second))
    return locations


def _random_origin(max_ini: list[int]) -> Origin:
    """One draw per axis that has room to move (swap.py:170-180)."""
    coords = [0 if m == 0 else int(torch.randint(m + 1, (1,)).item()) for m in max_ini]
    return (coords[0], coords[1], coords[2])


def _patches_overlap(a: Origin, b: Origin, patch_size: tuple[int, int, int]) -> bool:
    return all(not (ai + p <= bi or bi + p <= ai) for ai, bi, p in zip(a, b, patch_size, strict=True))
