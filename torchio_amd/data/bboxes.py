"""3-D bounding boxes (mirror of reference ``data/bboxes.py``).

``(N, 6)`` rows read through a ``BoundingBoxFormat``: an axis string (``data/axes.py``) and a representation, two opposite
corners or centre plus size.  Spatial transforms move the eight corners of every box as points and keep the axis-aligned hull
(DESIGN.md section 4.18): boxes are neither clipped to the field of view nor removed.
"""
from __future__ import annotations

from enum import Enum
from typing import Any

import numpy as np
import torch
from torch import Tensor

from .affine import AffineMatrix
from .axes import AxesType
from .axes import axes_type
from .axes import get_axis_mapping
from .axes import validate_axes
from .points import _as_affine
from .points import _through


class Representation(Enum):
    """``CORNERS``: ``(a1, b1, c1, a2, b2, c2)``; ``CENTER_SIZE``: ``(ac, bc, cc, sa, sb, sc)``."""

    CORNERS = "corners"
    CENTER_SIZE = "center_size"


class BoundingBoxFormat:
    """Axis string plus representation of the six box columns."""

    IJKIJK: "BoundingBoxFormat"
    IJKWHD: "BoundingBoxFormat"

    __slots__ = ("_axes", "_representation")

    def __init__(self, axes: str, representation: Representation | str = Representation.CORNERS) -> None:
        self._axes = validate_axes(axes)
        self._representation = Representation(representation) if isinstance(representation, str) else representation

    @property
    def axes(self) -> str:
        return self._axes

    @property
    def representation(self) -> Representation:
        return self._representation

    def __eq__(self, other: object) -> bool:
        if not isinstance(other, BoundingBoxFormat):
            return NotImplemented
        return (self._axes, self._representation) == (other._axes, other._representation)

    def __hash__(self) -> int:
        return hash((self._axes, self._representation))

    def __repr__(self) -> str:
        return f"BoundingBoxFormat(axes={self._axes!r}, representation={self._representation.value!r})"


BoundingBoxFormat.IJKIJK = BoundingBoxFormat("IJK", Representation.CORNERS)
BoundingBoxFormat.IJKWHD = BoundingBoxFormat("IJK", Representation.CENTER_SIZE)


def _corners_to_center_size(data: Tensor) -> Tensor:
    low, high = data[..., :3], data[..., 3:]
    return torch.cat([(low + high) / 2, high - low], dim=-1)


def _center_size_to_corners(data: Tensor) -> Tensor:
    center, half = data[..., :3], data[..., 3:] / 2
    return torch.cat([center - half, center + half], dim=-1)


def _sorted_corners(first: Tensor, second: Tensor) -> Tensor:
    """Two opposite corners as (low, high): a flip or an affine may have swapped them per axis."""
    return torch.cat([torch.minimum(first, second), torch.maximum(first, second)], dim=-1)


def _permute_corners(data: Tensor, perm, flips) -> Tensor:
    signs = torch.tensor([-1.0 if flip else 1.0 for flip in flips], dtype=data.dtype, device=data.device)
    return _sorted_corners(data[:, :3][:, list(perm)] * signs, data[:, 3:][:, list(perm)] * signs)


def _corners_through(matrix: Tensor, data: Tensor) -> Tensor:
    return _sorted_corners(_through(matrix, data[:, :3]), _through(matrix, data[:, 3:]))


class BoundingBoxes:
    """``N`` boxes as an ``(N, 6)`` tensor in a ``BoundingBoxFormat``, with optional per-box labels."""

    def __init__(self, data, *, format: BoundingBoxFormat, labels: Tensor | None = None, affine=None,  # noqa: A002
                 metadata: dict[str, Any] | None = None) -> None:
        if not isinstance(data, Tensor):
            data = torch.as_tensor(np.asarray(data), dtype=torch.float32)
        if data.ndim != 2 or data.shape[1] != 6:
            raise ValueError(f"BoundingBoxes must have shape (N, 6), got {tuple(data.shape)}")
        if labels is not None and labels.shape[0] != data.shape[0]:
            raise ValueError(f"Expected {data.shape[0]} labels, got {labels.shape[0]}")
        self._data = data
        self._format = format
        self._labels = labels
        self._affine = _as_affine(affine)
        self._metadata: dict[str, Any] = dict(metadata) if metadata else {}

    @staticmethod
    def _parse_affine(affine) -> AffineMatrix:
        return _as_affine(affine)

    @property
    def data(self) -> Tensor:
        return self._data

    @property
    def format(self) -> BoundingBoxFormat:  # noqa: A003
        return self._format

    @property
    def labels(self) -> Tensor | None:
        return self._labels

    @property
    def affine(self) -> AffineMatrix:
        return self._affine

    @property
    def metadata(self) -> dict[str, Any]:
        return self._metadata

    @property
    def num_boxes(self) -> int:
        return int(self._data.shape[0])

    @property
    def device(self) -> torch.device:
        return self._data.device

    def to(self, *args: Any, **kwargs: Any) -> "BoundingBoxes":
        """Move or cast boxes and labels in place; returns ``self``."""
        self._data = self._data.to(*args, **kwargs)
        if self._labels is not None:
            self._labels = self._labels.to(*args, **kwargs)
        return self

    def to_format(self, format: BoundingBoxFormat) -> "BoundingBoxes":  # noqa: A002
        """New ``BoundingBoxes`` in *format*: through corners in the source axes, the axis change (a permutation with flips
        inside one family, the affine between families), then the target representation."""
        if format == self._format:
            return self._clone(format=format)
        source_axes, target_axes = self._format.axes, format.axes
        data = self._data
        if self._format.representation == Representation.CENTER_SIZE:
            data = _center_size_to_corners(data)
        if source_axes != target_axes:
            source_type, target_type = axes_type(source_axes), axes_type(target_axes)
            if source_type == target_type:
                data = _permute_corners(data, *get_axis_mapping(source_axes, target_axes))
            elif source_type == AxesType.VOXEL:
                if source_axes != "IJK":
                    data = _permute_corners(data, *get_axis_mapping(source_axes, "IJK"))
                data = _corners_through(self._affine.data, data)
                world_axes = "".join(self._affine.orientation)
                if world_axes != target_axes:
                    data = _permute_corners(data, *get_axis_mapping(world_axes, target_axes))
            else:
                world_axes = "".join(self._affine.orientation)
                if source_axes != world_axes:
                    data = _permute_corners(data, *get_axis_mapping(source_axes, world_axes))
                data = _corners_through(self._affine.inverse().data, data)
                if target_axes != "IJK":
                    data = _permute_corners(data, *get_axis_mapping("IJK", target_axes))
        if format.representation == Representation.CENTER_SIZE:
            data = _corners_to_center_size(data)
        return self._clone(data=data, format=format)

    def new_like(self, *, data, labels: Tensor | None = None, affine=None) -> "BoundingBoxes":
        """New boxes with this format and metadata; no labels unless given, *affine* defaults to a copy of this one."""
        new_affine = _as_affine(affine) if affine is not None else self._affine.clone()
        return type(self)(data, format=self._format, labels=labels, affine=new_affine, metadata=dict(self._metadata))

    def _clone(self, *, data: Tensor | None = None, format: BoundingBoxFormat | None = None) -> "BoundingBoxes":  # noqa: A002
        return type(self)(
            self._data.clone() if data is None else data,
            format=self._format if format is None else format,
            labels=None if self._labels is None else self._labels.clone(),
            affine=self._affine.clone(),
            metadata=dict(self._metadata),
        )

    def __len__(self) -> int:
        return self.num_boxes

    def __repr__(self) -> str:
        return (
            f"BoundingBoxes(num_boxes={self.num_boxes}, axes={self._format.axes!r},"
            f" representation={self._format.representation.value!r})"
        )

    def __deepcopy__(self, memo: dict) -> "BoundingBoxes":
        new = self._clone()
        memo[id(self)] = new
        return new
