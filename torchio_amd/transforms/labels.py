"""The label-map transforms on the HIP engine (mirror of reference ``transforms/label/*.py``).

``RemapLabels``, ``RemoveLabels`` and ``SequentialLabels`` are one launch of ``tio_label_remap`` per label map whatever
the number of labels (the reference runs a full-volume compare and a masked write per label); ``OneHot`` reads the map
once (``tio_label_one_hot``); ``Contour`` is one launch (``tio_label_contour``: the reference pads, negates, max-pools
and compares); ``KeepLargestComponent`` labels the connected components of every listed value of the whole batch on the
device (``tio_keep_largest_component``: the reference copies one mask per label and element to the host for SimpleITK).
Same constructors, ``make_params`` dictionaries, history and inverses as the reference.  Every transform acts on
``LabelMap`` batches only.
"""
from __future__ import annotations

from collections.abc import Sequence
from typing import Any

import torch

from .. import ops
from ..data.batch import ImagesBatch
from ..data.batch import SubjectsBatch
from ..data.image import LabelMap
from .transform import Transform


def _check_representable(value, dtype: torch.dtype, what: str) -> None:
    """The reference writes a Python number into the tensor and lets the cast do what it does; here a value the label
    map's dtype cannot hold is an error."""
    number = float(value)
    if dtype.is_floating_point:
        ok = number == number and abs(number) != float("inf") and float(torch.tensor(number, dtype=torch.float64).to(dtype)) == number
    else:
        info = torch.iinfo(dtype)
        ok = number.is_integer() and info.min <= number <= info.max
    if not ok:
        raise ValueError(f"{what} {value!r} cannot be represented in a {dtype} label map")


class _LabelTransform(Transform):
    def _label_maps(self, batch: SubjectsBatch) -> dict[str, ImagesBatch]:
        return {name: image for name, image in self._get_images(batch).items() if issubclass(image._image_class, LabelMap)}


def _remap(data: torch.Tensor, mapping: dict, default=None) -> torch.Tensor:
    for new in mapping.values():
        _check_representable(new, data.dtype, "label")
    if default is not None:
        _check_representable(default, data.dtype, "label")
    return ops.engine().label_remap(data, mapping, default=default)


class RemapLabels(_LabelTransform):
    """Replace every key of ``remapping`` by its value; other labels stay (remap_labels.py:12-69)."""

    def __init__(self, remapping: dict[int, int], **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.remapping = remapping

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {"remapping": self.remapping}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for image in self._label_maps(batch).values():
            image.data = _remap(image.data, params["remapping"])
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "RemapLabels":
        return RemapLabels(remapping={new: old for old, new in params["remapping"].items()}, copy=False)


class RemoveLabels(_LabelTransform):
    """Set the listed label values to ``background_label`` (remove_labels.py:13-61)."""

    def __init__(self, labels: Sequence[int], *, background_label: int = 0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.labels = list(labels)
        self.background_label = background_label

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        mapping = dict.fromkeys(self.labels, self.background_label)
        for image in self._label_maps(batch).values():
            image.data = _remap(image.data, mapping)
        return batch


class SequentialLabels(_LabelTransform):
    """Renumber the labels to 0, 1, 2 … in ascending order of their values; the mapping comes from the first element of each
    label map, values it does not list become 0 (sequential_labels.py:14-74)."""

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        remappings: dict[str, dict[int, int]] = {}
        for name, image in self._label_maps(batch).items():
            unique = sorted(int(v) for v in ops.engine().unique_labels(image.data[0]).tolist())
            remappings[name] = {old: new for new, old in enumerate(unique)}
        return {"remappings": remappings}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        remappings = params["remappings"]
        for name, image in self._label_maps(batch).items():
            if name in remappings:
                image.data = _remap(image.data, remappings[name], default=0)
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "_SequentialLabelsInverse":
        return _SequentialLabelsInverse(remappings=params["remappings"], copy=False)


class _SequentialLabelsInverse(_LabelTransform):
    """Inverse of ``SequentialLabels`` for history replay (sequential_labels.py:77-105)."""

    def __init__(self, *, remappings: dict[str, dict[int, int]], **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._remappings = remappings

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for name, image in self._label_maps(batch).items():
            if name in self._remappings:
                image.data = _remap(image.data, {new: old for old, new in self._remappings[name].items()}, default=0)
        return batch


class OneHot(_LabelTransform):
    """``(B, 1, I, J, K)`` label maps to float32 ``(B, num_classes, I, J, K)``; ``num_classes=-1`` infers ``max + 1``
    (one_hot.py:14-78).  A value outside ``[0, num_classes)`` raises ``RuntimeError`` like ``F.one_hot``."""

    def __init__(self, *, num_classes: int = -1, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.num_classes = num_classes

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {"num_classes": self.num_classes}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for image in self._label_maps(batch).values():
            image.data = ops.engine().label_one_hot(image.data[:, :1], params["num_classes"])
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "_OneHotInverse":
        return _OneHotInverse(copy=False)


class _OneHotInverse(_LabelTransform):
    """Inverse of ``OneHot``: the argmax over the channels, as float32 (one_hot.py:81-97).  Not a hot path."""

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for image in self._label_maps(batch).values():
            if image.data.shape[1] > 1:
                image.data = image.data.argmax(dim=1, keepdim=True).float()
        return batch


class Contour(_LabelTransform):
    """Binary float32 mask of the label boundaries (contour.py:15-71) — what the reference's code computes: a voxel is marked
    where one of its 26 neighbours is smaller, and every voxel on a face of the volume is marked (unless its value is <= -1)."""

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for image in self._label_maps(batch).values():
            image.data = ops.engine().label_contour(image.data)
        return batch


class KeepLargestComponent(_LabelTransform):
    """Keep only the largest connected component of each label, per batch element (keep_largest.py:17-125).

    ``labels=None``: every value of the label map but ``background_label``.  Of equally large components the one whose
    first voxel comes first in C order stays.
    """

    def __init__(self, labels: Sequence[int] | None = None, *, background_label: int = 0, fully_connected: bool = True, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.labels = list(labels) if labels is not None else None
        self.background_label = background_label
        self.fully_connected = fully_connected

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        engine = ops.engine()
        for image in self._label_maps(batch).values():
            data = image.data
            if data.shape[1] != 1:
                raise RuntimeError(f"KeepLargestComponent requires single-channel label maps, got {data.shape[1]} channels")
            _check_representable(self.background_label, data.dtype, "background_label")
            labels = self.labels
            if labels is None:
                # the union over the batch: a label absent from an element has no voxels there
                found = engine.unique_labels(data)
                labels = found[found != float(self.background_label)]
            image.data = engine.keep_largest_component(data, labels, background=self.background_label, fully_connected=self.fully_connected)
        return batch
