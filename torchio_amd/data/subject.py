"""Subject container (mirror of the in-memory part of reference ``data/subject.py:25``)."""
from __future__ import annotations

import copy as _copy
from typing import Any

from .bboxes import BoundingBoxes
from .image import Image
from .points import Points


class Subject:
    """Named images, point sets and bounding boxes plus arbitrary metadata; carries the transform history."""

    def __init__(self, **entries: Any) -> None:
        object.__setattr__(self, "_images", {})
        object.__setattr__(self, "_points", {})
        object.__setattr__(self, "_bounding_boxes", {})
        object.__setattr__(self, "_metadata", {})
        self.applied_transforms: list = []
        for key, value in entries.items():
            if isinstance(value, Image):
                self._images[key] = value
            elif isinstance(value, Points):
                self._points[key] = value
            elif isinstance(value, BoundingBoxes):
                self._bounding_boxes[key] = value
            else:
                self._metadata[key] = value
        if not self._images and not self._points and not self._bounding_boxes:
            raise ValueError("A Subject needs at least one Image, Points or BoundingBoxes entry")

    @property
    def images(self) -> dict[str, Image]:
        return self._images

    @property
    def points(self) -> dict[str, Points]:
        """The subject-level point sets (a copy of the dict, the sets themselves)."""
        return dict(self._points)

    @property
    def bounding_boxes(self) -> dict[str, BoundingBoxes]:
        """The subject-level box sets (a copy of the dict, the sets themselves)."""
        return dict(self._bounding_boxes)

    def all_points(self) -> dict:
        """Subject-level point sets under their name, image-level ones under ``(image_name, points_name)``."""
        result: dict = dict(self._points)
        for image_name, image in self._images.items():
            for name, points in image.points.items():
                result[(image_name, name)] = points
        return result

    def all_bounding_boxes(self) -> dict:
        """Subject-level box sets under their name, image-level ones under ``(image_name, boxes_name)``."""
        result: dict = dict(self._bounding_boxes)
        for image_name, image in self._images.items():
            for name, boxes in image.bounding_boxes.items():
                result[(image_name, name)] = boxes
        return result

    @property
    def metadata(self) -> dict[str, Any]:
        return self._metadata

    def __getattr__(self, name: str):
        if name.startswith("_"):
            raise AttributeError(name)
        for store in ("_images", "_points", "_bounding_boxes"):
            entries = object.__getattribute__(self, store)
            if name in entries:
                return entries[name]
        metadata = object.__getattribute__(self, "_metadata")
        if name in metadata:
            return metadata[name]
        raise AttributeError(f"Subject has no attribute {name!r}")

    def __getitem__(self, key: str):
        for store in (self._images, self._points, self._bounding_boxes):
            if key in store:
                return store[key]
        return self._metadata[key]

    def __contains__(self, key: str) -> bool:
        return any(key in store for store in (self._images, self._points, self._bounding_boxes, self._metadata))

    def __iter__(self):
        """The names of the spatial entries: images, then point sets, then box sets (subject.py:147-150)."""
        yield from self._images
        yield from self._points
        yield from self._bounding_boxes

    def __len__(self) -> int:
        return len(self._images) + len(self._points) + len(self._bounding_boxes)

    def keys(self):
        return [*self._images, *self._points, *self._bounding_boxes, *self._metadata]

    @property
    def spatial_shape(self) -> tuple[int, int, int]:
        return next(iter(self._images.values())).spatial_shape

    @property
    def device(self):
        return next(iter(self._images.values())).device

    def to(self, *args, **kwargs) -> "Subject":
        for entry in (*self._images.values(), *self._points.values(), *self._bounding_boxes.values()):
            entry.to(*args, **kwargs)
        return self

    @property
    def shape(self) -> tuple[int, int, int, int]:
        """``(C, I, J, K)`` of the first image (from the header alone for an unloaded file-backed image)."""
        return next(iter(self._images.values())).shape

    def load(self, device=None) -> "Subject":
        """Read every file-backed image now (on *device* when given; tensor-backed images are moved there too)."""
        for image in self._images.values():
            image.load(device)
        return self

    # -- history -------------------------------------------------------------
    def get_inverse_transform(self, *, warn: bool = True, ignore_intensity: bool = False):
        from ..transforms.inverse import get_inverse_transform  # noqa: PLC0415

        return get_inverse_transform(self.applied_transforms, warn=warn, ignore_intensity=ignore_intensity)

    def apply_inverse_transform(self, **kwargs):
        result = self.get_inverse_transform(**kwargs)(self)
        result.applied_transforms = []
        return result

    def clear_history(self) -> None:
        self.applied_transforms = []

    def __deepcopy__(self, memo):
        entries = {k: _copy.deepcopy(v, memo) for k, v in self._images.items()}
        for store in (self._points, self._bounding_boxes, self._metadata):
            entries.update({k: _copy.deepcopy(v, memo) for k, v in store.items()})
        new = Subject(**entries)
        new.applied_transforms = list(self.applied_transforms)
        return new

    def __repr__(self) -> str:
        annotations = ""
        if self._points:
            annotations += f", points={list(self._points)}"
        if self._bounding_boxes:
            annotations += f", bboxes={list(self._bounding_boxes)}"
        return f"Subject(images={list(self._images)}{annotations}, metadata={list(self._metadata)})"
