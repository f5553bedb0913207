"""``HistogramStandardization`` and ``compute_histogram_landmarks`` on the HIP engine (mirror of reference
``transforms/intensity/histogram_standardization.py``; Nyúl and Udupa 1999).

The reference copies every batch element to the host, runs ``np.percentile`` there and returns to the device for ``diff`` /
``bucketize`` / gather.  Here the percentiles of every element come from one selection on the device
(``tio_intensity_multi_quantiles``: three reads of the batch for all ranks, finished by numpy's rule in float64), a one-block
kernel turns them into each element's table and one pass applies it (``tio_histogram_standardize``), every step the
reference's float32 operation: no read-back and no synchronisation in the transform.  The training reads each image's
percentiles back once and runs the reference's regression on the host in float64.
"""
from __future__ import annotations

from collections.abc import Callable
from collections.abc import Sequence
from pathlib import Path
from typing import Any

import numpy as np
import torch
from torch import Tensor

from .. import ops
from ..data.batch import SubjectsBatch
from ..data.image import ScalarImage
from .transform import IntensityTransform

DEFAULT_CUTOFF: tuple[float, float] = (0.01, 0.99)
STANDARD_RANGE: tuple[float, float] = (0.0, 100.0)

# the cutoff endpoints, the deciles and the quartiles (histogram_standardization.py:32-46)
_DEFAULT_QUANTILES: tuple[float, ...] = (0.01, 0.10, 0.20, 0.25, 0.30, 0.40, 0.50, 0.60, 0.70, 0.75, 0.80, 0.90, 0.99)


def _build_quantiles(cutoff: tuple[float, float]) -> tuple[float, ...]:
    return tuple(sorted({*_DEFAULT_QUANTILES, cutoff[0], cutoff[1]}))


def _validate_quantiles(quantiles: tuple[float, ...], cutoff: tuple[float, float]) -> None:
    if len(quantiles) < 2:
        raise ValueError(f"Need at least 2 quantiles, got {len(quantiles)}")
    if any(q < 0 or q > 1 for q in quantiles):
        raise ValueError("All quantiles must be in [0, 1]")
    if cutoff[0] not in quantiles or cutoff[1] not in quantiles:
        raise ValueError(f"Cutoff values {cutoff} must be included in quantiles. Got quantiles: {quantiles}")


def _load_tensor(source) -> Tensor:
    """The image's ``(C, I, J, K)`` tensor; a path raises what ``ScalarImage(path)`` raises here (no file I/O in this package)."""
    if isinstance(source, ScalarImage):
        return source.data
    return ScalarImage(source).data


def _compute_average_mapping(database: np.ndarray) -> np.ndarray:
    """``(N, P)`` percentiles of N images -> ``(P,)`` landmarks in the standard range (histogram_standardization.py:148-166):
    each image's line through its two cutoff percentiles, averaged; float64 on the host."""
    pc_low, pc_high = database[:, 0], database[:, -1]
    s_low, s_high = STANDARD_RANGE
    with np.errstate(divide="ignore", invalid="ignore"):
        slopes = np.nan_to_num((s_high - s_low) / (pc_high - pc_low))
    intercept = float(np.mean(s_low - slopes * pc_low))
    return slopes @ database / len(database) + intercept


def compute_histogram_landmarks(
    images: Sequence[ScalarImage],
    *,
    quantiles: Sequence[float] | None = None,
    cutoff: tuple[float, float] = DEFAULT_CUTOFF,
    masking_method: Callable[[Tensor], Tensor] | None = None,
) -> Tensor:
    """Average landmarks of the training images (histogram_standardization.py:49-111), to be handed to
    ``HistogramStandardization``.  ``masking_method`` takes an image's ``(C, I, J, K)`` device tensor and returns a mask of
    that shape.  Each image's percentiles are selected on the device and read back once."""
    quantiles = _build_quantiles(cutoff) if quantiles is None else tuple(sorted(set(quantiles)))
    _validate_quantiles(quantiles, cutoff)
    engine = ops.engine()
    rows: list[np.ndarray] = []
    for source in images:
        tensor = _load_tensor(source)
        if tensor.device.type != engine.device_type and engine.device_type == "cuda" and torch.cuda.is_available():
            tensor = ops.h2d(tensor, torch.device("cuda", torch.cuda.current_device()))
        mask = None
        if masking_method is not None:
            mask = masking_method(tensor)
            if tuple(mask.shape) != tuple(tensor.shape):
                mask = mask.expand_as(tensor)
        values, _ = engine.intensity_multi_quantiles(tensor[None], quantiles, mask)
        rows.append(values[0].cpu().numpy())
    return torch.as_tensor(_compute_average_mapping(np.vstack(rows)), dtype=torch.float32)


def _load_landmarks(source) -> Tensor:
    if isinstance(source, Tensor):
        return source.float()
    path = Path(source)
    if path.suffix == ".npy":
        return torch.as_tensor(np.load(path), dtype=torch.float32)
    if path.suffix in (".pt", ".pth"):
        data = torch.load(path, weights_only=True)
        if isinstance(data, Tensor):
            return data.float()
        raise TypeError(f"Expected a Tensor in {path}, got {type(data).__name__}")
    raise ValueError(f"Unsupported landmarks file extension: {path.suffix}")


class HistogramStandardization(IntensityTransform):
    """Map each image's intensities piecewise-linearly so that its percentiles land on ``landmarks``
    (histogram_standardization.py:169-229).  ``landmarks``: a 1-D tensor, or the path of a ``.npy`` / ``.pt`` / ``.pth`` file,
    as ``compute_histogram_landmarks`` returns them; one instance per modality (``include=[...]``).  Every batch element
    gets the table of its own percentiles.  The image keeps its dtype."""

    def __init__(self, landmarks: Tensor | Path | str, *, cutoff: tuple[float, float] = DEFAULT_CUTOFF, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.landmarks = _load_landmarks(landmarks)
        self.cutoff = cutoff

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        quantiles = _build_quantiles(self.cutoff)
        for img_batch in self._get_images(batch).values():
            if img_batch.batch_size == 0:
                continue
            if len(self.landmarks) != len(quantiles):
                raise ValueError(
                    f"Number of landmarks ({len(self.landmarks)}) does not match "
                    f"the number of quantile positions ({len(quantiles)}). "
                    "Ensure the same quantile scheme was used for training."
                )
            img_batch.data = ops.engine().histogram_standardize(img_batch.data, self.landmarks, quantiles)
        return batch
