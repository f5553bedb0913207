"""``Normalize``, ``Standardize``, ``Clamp`` and ``Mask`` on the HIP engine (mirror of reference
``transforms/intensity/normalize.py``, ``standardize.py``, ``clamp.py`` and ``mask.py``).

The statistics are computed on the device: the percentiles of ``Normalize`` by an exact radix select
(``tio_intensity_quantiles``: three reads of the first batch element and one read-back for both percentiles, where the
reference runs ``torch.kthvalue`` up to four times), the mean and deviation of ``Standardize`` by a float64 reduction
(``tio_intensity_moments``: one read, one read-back).  The elementwise halves are one fused pass each
(``tio_intensity_map``, ``tio_intensity_clamp``, ``tio_intensity_mask``), with the float32 rounding sequence of the
reference's expressions.  Same constructors, draw order, parameter dictionaries, warnings, errors and inverses.
"""
from __future__ import annotations

import warnings
from collections.abc import Callable
from typing import Any

import torch
from torch import Tensor

from .. import ops
from ..data.batch import ImagesBatch
from ..data.batch import SubjectsBatch
from ..data.image import LabelMap
from .parameter_range import Choice
from .parameter_range import _ParameterRange
from .transform import IntensityTransform


def _to_range(value) -> _ParameterRange:
    if isinstance(value, (torch.distributions.Distribution, Choice)):
        return _ParameterRange(value)
    if isinstance(value, (int, float)):
        return _ParameterRange(float(value))
    return _ParameterRange(tuple(float(v) for v in value))


def _label_map_element(key: str, batch: SubjectsBatch) -> Tensor:
    """The first element of the label map ``key`` (normalize.py:215-227, standardize.py:161-172, mask.py:79-91)."""
    if key not in batch.images:
        raise KeyError(f'Masking method "{key}" not found in batch images. Available: {list(batch.images.keys())}')
    mask_batch = batch.images[key]
    if not issubclass(mask_batch._image_class, LabelMap):
        raise TypeError(f'Masking method "{key}" must refer to a LabelMap.')
    return mask_batch.data[0]


def _as_engine_mask(mask: Tensor, element: Tensor) -> Tensor:
    """A mask the kernels take — ``(1 or C, I, J, K)``, nonzero = inside, which is what ``.bool()`` means — from whatever
    broadcasts over ``element`` the way ``mask.expand_as(element)`` does."""
    if mask.ndim == 4 and mask.shape[0] in (1, element.shape[0]) and tuple(mask.shape[1:]) == tuple(element.shape[1:]):
        return mask
    return mask.expand_as(element)


def _statistics_mask(masking_method, img_batch: ImagesBatch, batch: SubjectsBatch) -> Tensor | None:
    """``_get_mask`` of the reference (normalize.py:204-232, standardize.py:142-174); the callable receives the device tensor."""
    if masking_method is None:
        return None
    element = img_batch.data[0]
    if callable(masking_method) and not isinstance(masking_method, str):
        return _as_engine_mask(masking_method(element), element)
    if isinstance(masking_method, str):
        return _as_engine_mask(_label_map_element(masking_method, batch), element)
    raise TypeError(f"masking_method must be None, str, or callable, got {type(masking_method)}")


class Normalize(IntensityTransform):
    """Clip to an input range and map it linearly onto ``[out_min, out_max]`` (normalize.py:35-232).

    The input range is ``in_min`` / ``in_max`` when both are given, else the ``percentile_low`` / ``percentile_high``
    percentiles of the (masked) first batch element of each image.  All six numbers take a scalar, a ``(low, high)``
    range, a ``Choice`` or a distribution.
    """

    def __init__(
        self,
        *,
        out_min=-1.0,
        out_max=1.0,
        in_min=None,
        in_max=None,
        percentile_low=0.0,
        percentile_high=100.0,
        masking_method: str | Callable[[Tensor], Tensor] | None = None,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        self.out_min = _to_range(out_min)
        self.out_max = _to_range(out_max)
        self.in_min = _to_range(in_min) if in_min is not None else None
        self.in_max = _to_range(in_max) if in_max is not None else None
        self.percentile_low = _to_range(percentile_low)
        self.percentile_high = _to_range(percentile_high)
        self.masking_method = masking_method

    @property
    def supports_per_instance_params(self) -> bool:
        return True

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        n = self._resolve_n(batch)
        out_min = self.out_min.sample_1d(n)
        out_max = self.out_max.sample_1d(n)
        pct_low = self.percentile_low.sample_1d()
        pct_high = self.percentile_high.sample_1d()
        params: dict[str, Any] = {"out_min": self._serialize_param(out_min), "out_max": self._serialize_param(out_max)}
        if self.in_min is not None and self.in_max is not None:
            params["in_min"] = self.in_min.sample_1d()
            params["in_max"] = self.in_max.sample_1d()
        else:
            in_ranges: dict[str, tuple[float, float]] = {}
            for name, img_batch in self._get_images(batch).items():
                mask = _statistics_mask(self.masking_method, img_batch, batch)
                in_ranges[name] = _percentile_range(img_batch.data, mask, pct_low, pct_high, name)
            params["in_ranges"] = in_ranges
        if n is not None:
            self._tag_batched(params, batch, n, None, ["out_min", "out_max"])
        return params

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for name, img_batch in self._get_images(batch).items():
            if "in_min" in params:
                in_min, in_max = params["in_min"], params["in_max"]
            else:
                in_ranges = params.get("in_ranges", {})
                if name not in in_ranges:
                    continue
                in_min, in_max = in_ranges[name]
            in_range = in_max - in_min
            if in_range == 0:
                warnings.warn(f'Cannot rescale "{name}": input range is zero.', RuntimeWarning, stacklevel=2)
                continue
            out_min, out_range = _out_min_and_range(params["out_min"], params["out_max"], img_batch.data)
            img_batch.data = ops.engine().intensity_map(img_batch.data, "rescale_clip", in_min=in_min, in_max=in_max, in_range=in_range,
                                                        out_min=out_min, out_range=out_range)
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "_RescaleInverse":
        return _RescaleInverse(out_min=params["out_min"], out_max=params["out_max"], in_min=params.get("in_min"), in_max=params.get("in_max"),
                               in_ranges=params.get("in_ranges"), copy=False)


class _RescaleInverse(IntensityTransform):
    """Inverse of ``Normalize`` for history replay (normalize.py:235-301); what the clip removed stays removed."""

    def __init__(self, *, out_min, out_max, in_min, in_max, in_ranges, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._out_min = out_min
        self._out_max = out_max
        self._in_min = in_min
        self._in_max = in_max
        self._in_ranges = in_ranges

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for name, img_batch in self._get_images(batch).items():
            if self._in_min is not None and self._in_max is not None:
                in_min, in_max = self._in_min, self._in_max
            elif self._in_ranges is not None and name in self._in_ranges:
                in_min, in_max = self._in_ranges[name]
            else:
                continue
            in_range = in_max - in_min
            if in_range == 0:
                continue
            out_min, out_range = _out_min_and_range(self._out_min, self._out_max, img_batch.data)
            if isinstance(out_range, float) and out_range == 0:
                continue
            # (per element: the kernel leaves the elements whose out_min == out_max as they are)
            img_batch.data = ops.engine().intensity_map(img_batch.data, "rescale", in_min=in_min, in_range=in_range, out_min=out_min,
                                                        out_range=out_range)
        return batch


def _out_min_and_range(out_min, out_max, data: Tensor):
    """The output minimum and range: two Python floats, or two ``(B,)`` float32 device tensors for per-instance parameters —
    the range subtracted in float32, as ``max_b - min_b`` is (normalize.py:304-330)."""
    if isinstance(out_min, list):
        min_t = torch.tensor(out_min, dtype=torch.float32)
        max_t = torch.tensor(out_max, dtype=torch.float32)
        both = ops.h2d(torch.stack([min_t, max_t - min_t]), data.device)
        return both[0], both[1]
    return out_min, float(out_max - out_min)


def _percentile_range(data: Tensor, mask: Tensor | None, pct_low: float, pct_high: float, image_name: str) -> tuple[float, float]:
    """``(in_min, in_max)`` from the percentiles of the first batch element inside the mask (normalize.py:333-365)."""
    engine = ops.engine()
    fractions = [pct_low / 100.0, pct_high / 100.0]
    (low, high), count = engine.intensity_quantiles(data, fractions, mask, return_count=True)
    if count == 0 and mask is not None:
        warnings.warn(f'Cannot compute percentiles for "{image_name}": mask is empty. Using full range.', RuntimeWarning, stacklevel=3)
        low, high = engine.intensity_quantiles(data, fractions)
    return low, high


RescaleIntensity = Normalize


class Standardize(IntensityTransform):
    """Subtract the mean and divide by the (unbiased) standard deviation of the (masked) first batch element
    (standardize.py:17-107).  The statistics are accumulated in float64 and rounded once, so they lie within one float32
    ulp of the exact values; the reference's float32 reductions land next to them, not on the same bits."""

    def __init__(self, *, masking_method: str | Callable[[Tensor], Tensor] | None = None, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.masking_method = masking_method

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        engine = ops.engine()
        stats: dict[str, tuple[float, float]] = {}
        for name, img_batch in self._get_images(batch).items():
            mask = _statistics_mask(self.masking_method, img_batch, batch)
            count, mean, std = engine.intensity_moments(img_batch.data, mask)
            if count == 0 and mask is not None:
                warnings.warn(f'Mask is empty for "{name}". Using all voxels.', RuntimeWarning, stacklevel=2)
                count, mean, std = engine.intensity_moments(img_batch.data)
            stats[name] = (mean, std)
        return {"stats": stats}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        stats = params["stats"]
        for name, img_batch in self._get_images(batch).items():
            if name not in stats:
                continue
            mean, std = stats[name]
            if std == 0:
                raise RuntimeError(f'Standard deviation is zero for masked values in "{name}". Cannot standardize.')
            img_batch.data = ops.engine().intensity_map(img_batch.data, "sub_div", in_min=mean, in_range=std)
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "_StandardizeInverse":
        return _StandardizeInverse(stats=params["stats"], copy=False)


class _StandardizeInverse(IntensityTransform):
    """Inverse of ``Standardize`` for history replay: ``data * std + mean`` (standardize.py:110-139)."""

    def __init__(self, *, stats: dict[str, tuple[float, float]], **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._stats = stats

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for name, img_batch in self._get_images(batch).items():
            if name not in self._stats:
                continue
            mean, std = self._stats[name]
            if std == 0:
                continue
            img_batch.data = ops.engine().intensity_map(img_batch.data, "mul_add", in_min=mean, in_range=std)
        return batch


ZNormalization = Standardize


class Clamp(IntensityTransform):
    """``data.clamp(min=out_min, max=out_max)`` (clamp.py:11-57); ``None`` leaves that side open.

    The bounds are taken as Python floats, so an integer image comes out as float32 — also with integer bounds
    (``Clamp(out_min=-1000, out_max=1000)`` on int16 data), where the reference, through torch's type promotion, keeps the
    integer dtype.  Floating images keep their dtype in both."""

    def __init__(self, *, out_min: float | None = None, out_max: float | None = None, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if out_min is not None and out_max is not None and out_min > out_max:
            raise ValueError(f"out_min ({out_min}) must be <= out_max ({out_max})")
        self.out_min = out_min
        self.out_max = out_max

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {"out_min": self.out_min, "out_max": self.out_max}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for img_batch in self._get_images(batch).values():
            img_batch.data = ops.engine().clamp(img_batch.data, params["out_min"], params["out_max"])
        return batch


class Mask(IntensityTransform):
    """Set the voxels outside a mask to ``outside_value`` (mask.py:16-102).  The mask — a label map of the subject, all its
    nonzero values or the listed ``labels``, or what a callable makes of the first image — is taken from the first batch
    element and applies to every element and channel.

    ``outside_value`` is taken as a Python float: an integer image comes out as float32 — also with an integer
    ``outside_value``, where the reference keeps the integer dtype.  Floating images keep their dtype in both."""

    def __init__(self, *, masking_method: str | Callable = "brain", outside_value: float = 0.0, labels: list[int] | None = None,
                 **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.masking_method = masking_method
        self.outside_value = outside_value
        self.labels = labels

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        mask = self._resolve_mask(batch)
        for img_batch in self._get_images(batch).values():
            data = img_batch.data
            img_batch.data = ops.engine().mask_where(data, _as_engine_mask(mask, data[0]), self.outside_value)
        return batch

    def _resolve_mask(self, batch: SubjectsBatch) -> Tensor:
        if callable(self.masking_method) and not isinstance(self.masking_method, str):
            first_img = next(iter(self._get_images(batch).values()))
            return self.masking_method(first_img.data[0])
        if isinstance(self.masking_method, str):
            mask_data = _label_map_element(self.masking_method, batch)
            if self.labels is not None:
                # the OR of `mask_data == label`: one remap pass to 1 / 0
                return ops.engine().label_remap(mask_data, dict.fromkeys(self.labels, 1), default=0)
            return mask_data
        raise TypeError(f"masking_method must be a str or callable, got {type(self.masking_method)}")
