"""Sets of 3-D points (mirror of reference ``data/points.py``).

An ``(N, 3)`` coordinate tensor, the axis string that says what its columns mean (``data/axes.py``) and the voxel-to-world
affine of the image the points belong to.  Spatial transforms move the points with the image.
"""
from __future__ import annotations

from typing import Any

import numpy as np
import torch
from torch import Tensor

from .affine import AffineMatrix
from .axes import AxesType
from .axes import axes_type
from .axes import get_axis_mapping
from .axes import validate_axes


def _as_affine(affine) -> AffineMatrix:
    if affine is None:
        return AffineMatrix()
    return affine if isinstance(affine, AffineMatrix) else AffineMatrix(affine)


def _through(matrix: Tensor, data: Tensor) -> Tensor:
    """``(N, 3)`` coordinates through a 4x4 in float64, rounded to float32, on the coordinates' device (the affines of this
    package live on the host, ``AffineMatrix.to``)."""
    matrix = matrix.to(device=data.device, dtype=torch.float64)
    moved = data.to(torch.float64) @ matrix[:3, :3].T + matrix[:3, 3]
    return moved.to(torch.float32)


def _reorder(data: Tensor, perm, flips) -> Tensor:
    """Columns ``perm`` of *data*, negated where ``flips`` (a new tensor)."""
    signs = torch.tensor([-1.0 if flip else 1.0 for flip in flips], dtype=data.dtype, device=data.device)
    return data[:, list(perm)] * signs


def axes_matrix(axes: str, affine: AffineMatrix) -> np.ndarray:
    """The float64 4x4 that takes IJK voxel coordinates of *affine*'s grid to coordinates in *axes*."""
    matrix = np.eye(4)
    source = "IJK"
    if axes_type(axes) == AxesType.ANATOMICAL:
        matrix = affine.numpy().astype(np.float64)
        source = "".join(affine.orientation)
    perm, flips = get_axis_mapping(source, axes)
    reorder = np.zeros((4, 4))
    reorder[3, 3] = 1.0
    for column, (origin, flip) in enumerate(zip(perm, flips, strict=True)):
        reorder[column, origin] = -1.0 if flip else 1.0
    return reorder @ matrix


class Points:
    """``(N, 3)`` coordinates in a named axis convention (default ``"IJK"``: voxel indices)."""

    def __init__(self, data, *, axes: str = "IJK", affine=None, metadata: dict[str, Any] | None = None) -> None:
        if not isinstance(data, Tensor):
            data = torch.as_tensor(np.asarray(data), dtype=torch.float32)
        if data.ndim != 2 or data.shape[1] != 3:
            raise ValueError(f"Points must have shape (N, 3), got {tuple(data.shape)}")
        self._data = data
        self._axes = validate_axes(axes)
        self._affine = _as_affine(affine)
        self._metadata: dict[str, Any] = dict(metadata) if metadata else {}

    # kept under the reference's names: callers and subclasses use them
    @staticmethod
    def _parse_affine(affine) -> AffineMatrix:
        return _as_affine(affine)

    @property
    def data(self) -> Tensor:
        return self._data

    @property
    def axes(self) -> str:
        return self._axes

    @property
    def affine(self) -> AffineMatrix:
        return self._affine

    @property
    def metadata(self) -> dict[str, Any]:
        return self._metadata

    @property
    def num_points(self) -> int:
        return int(self._data.shape[0])

    @property
    def device(self) -> torch.device:
        return self._data.device

    def to(self, *args: Any, **kwargs: Any) -> "Points":
        """Move or cast the coordinates in place; returns ``self``."""
        self._data = self._data.to(*args, **kwargs)
        return self

    def to_world(self) -> Tensor:
        """The stored coordinates through the affine: ``(N, 3)`` float32 in world millimetres."""
        return _through(self._affine.data, self._data)

    def to_axes(self, target: str) -> "Points":
        """New ``Points`` in the *target* convention: a permutation with sign flips inside one family, through the affine
        between voxel and anatomical conventions."""
        target = validate_axes(target)
        if target == self._axes:
            return self._clone(axes=target)
        source_type, target_type = axes_type(self._axes), axes_type(target)
        if source_type == target_type:
            converted = _reorder(self._data, *get_axis_mapping(self._axes, target))
        elif source_type == AxesType.VOXEL:
            ijk = self._data if self._axes == "IJK" else _reorder(self._data, *get_axis_mapping(self._axes, "IJK"))
            converted = _through(self._affine.data, ijk)
            world_axes = "".join(self._affine.orientation)
            if world_axes != target:
                converted = _reorder(converted, *get_axis_mapping(world_axes, target))
        else:
            world_axes = "".join(self._affine.orientation)
            world = self._data if self._axes == world_axes else _reorder(self._data, *get_axis_mapping(self._axes, world_axes))
            converted = _through(self._affine.inverse().data, world)
            if target != "IJK":
                converted = _reorder(converted, *get_axis_mapping("IJK", target))
        return self._clone(data=converted, axes=target)

    def new_like(self, *, data, affine=None) -> "Points":
        """New ``Points`` with these axes and metadata; *affine* defaults to a copy of this one."""
        new_affine = _as_affine(affine) if affine is not None else self._affine.clone()
        return type(self)(data, axes=self._axes, affine=new_affine, metadata=dict(self._metadata))

    def _clone(self, *, data: Tensor | None = None, axes: str | None = None) -> "Points":
        return type(self)(
            self._data.clone() if data is None else data,
            axes=self._axes if axes is None else axes,
            affine=self._affine.clone(),
            metadata=dict(self._metadata),
        )

    def __len__(self) -> int:
        return self.num_points

    def __repr__(self) -> str:
        return f"Points(num_points={self.num_points}, axes={self._axes!r})"

    def __deepcopy__(self, memo: dict) -> "Points":
        new = self._clone()
        memo[id(self)] = new
        return new
