"""Points and BoundingBoxes through the spatial transforms.

One rule: a transform that produces ``out(o) = in(s(o))`` moves the annotations attached to that image by ``s^-1``, and the
moved annotation adopts the image's output affine.  Image-level annotations are governed by their own image, subject-level
ones by the first image the transform applies to.  ``s`` is a float64 4x4 (output voxel -> input voxel) built on the host,
for the ``Spatial`` family plus the coarse displacement field; every transform goes through the same ``tio_points_warp``
launch (``Engine.warp_points``), one per transform application for all annotations of the batch.

A batch without annotations never gets here: ``track`` returns ``None`` first.
"""
from __future__ import annotations

from typing import Any
from typing import Callable

import numpy as np
import torch

from .. import _abi
from .. import ops
from ..data.affine import AffineMatrix
from ..data.bboxes import BoundingBoxes
from ..data.bboxes import BoundingBoxFormat
from ..data.points import axes_matrix

_EYE4 = np.eye(4)
#: the eight corners of a (low, high) box as column picks of its six values
_CORNER_COLUMNS = [[3 * ((corner >> axis) & 1) + axis for axis in range(3)] for corner in range(8)]


class GridMap:
    """How the images of ONE batch element were resampled: ``out(o) = in(s(o))`` with ``s(o) = matrix o`` plus, when *field*
    is given, the displacement of the reference's sampling grid (spatial.py:1570-1577)."""

    __slots__ = ("matrix", "in_affine", "out_affine", "out_shape", "field", "affine_first")

    def __init__(self, matrix, in_affine: AffineMatrix, out_affine: AffineMatrix, out_shape=(1, 1, 1), field=None,
                 affine_first: bool = True) -> None:
        self.matrix = np.asarray(matrix, dtype=np.float64)
        self.in_affine, self.out_affine = in_affine, out_affine
        self.out_shape = tuple(int(s) for s in out_shape)
        self.field = field
        self.affine_first = bool(affine_first)


def parameter_block(matrix, *, inverse=None, out_shape=(1, 1, 1), in_spacing=(1.0, 1.0, 1.0), out_spacing=(1.0, 1.0, 1.0),
                    affine_first: bool = True, grid=(0, 0, 0), cp_offset: int = -1) -> np.ndarray:
    """One element's float64 parameter block of ``tio_points_warp`` as ``include/tio_hip.h`` lays it out."""
    matrix = np.asarray(matrix, dtype=np.float64)
    if inverse is None:
        try:
            inverse = np.linalg.inv(matrix if matrix.shape == (4, 4) else np.vstack([matrix, [0.0, 0.0, 0.0, 1.0]]))
        except np.linalg.LinAlgError:
            raise ValueError("annotations cannot follow a resampling whose voxel mapping is not invertible") from None
    block = np.zeros(_abi.POINTS_BLOCK_DOUBLES, dtype=np.float64)
    block[0:12] = matrix[:3].reshape(-1)
    block[12:24] = np.asarray(inverse, dtype=np.float64)[:3].reshape(-1)
    block[24:27] = out_shape
    block[27:30] = in_spacing
    block[30:33] = out_spacing
    block[33] = 1.0 if affine_first else 0.0
    block[34:37] = grid
    block[37] = cp_offset
    return block


def _launch(tensors: list, blocks: list, fields: list) -> list:
    """One ``Engine.warp_points`` call: item ``n`` owns ``tensors[n]``, ``blocks[n]`` and, unless ``None``, ``fields[n]``."""
    counts = [int(t.shape[0]) for t in tensors]
    if sum(counts) == 0:
        return tensors
    offsets = np.concatenate([[0], np.cumsum(counts)])
    unique: dict[int, tuple[int, Any]] = {}
    total = 0
    for n, field in enumerate(fields):
        if field is None:
            continue
        if id(field) not in unique:
            unique[id(field)] = (total, field)
            total += field.numel()
        blocks[n][37] = unique[id(field)][0]
    control_points = None
    if unique:
        flat = [field.detach().to(torch.float32).reshape(-1) for _, field in unique.values()]
        if len({f.device for f in flat}) > 1:
            flat = [f.cpu() for f in flat]
        control_points = flat[0] if len(flat) == 1 else torch.cat(flat)
    points = tensors[0] if len(tensors) == 1 else torch.cat(tensors)
    out = ops.engine().warp_points(points, offsets, torch.from_numpy(np.stack(blocks)), control_points)
    return list(torch.split(out, counts))


def _move_items(items: list, device) -> None:
    """``items``: ``(annotation, container, key, GridMap)``; every annotation is replaced in its container by the moved one."""
    if not items:
        return
    device = torch.device(device)
    tensors, pre, post = [], [], []
    for annotation, _, _, grid in items:
        if isinstance(annotation, BoundingBoxes):
            # corners in IJK of the governing image's input grid, the eight of every box as points
            ijk = annotation.new_like(data=annotation.data, labels=annotation.labels, affine=grid.in_affine).to_format(BoundingBoxFormat.IJKIJK)
            coords = ijk.data.to(torch.float32)[:, _CORNER_COLUMNS].reshape(-1, 3)
            pre.append(_EYE4), post.append(_EYE4)
        else:
            coords = annotation.data.to(torch.float32)
            # stored coordinates -> input voxels, output voxels -> stored coordinates: folded into the launch's matrices
            is_ijk = annotation.axes == "IJK"
            pre.append(_EYE4 if is_ijk else np.linalg.inv(axes_matrix(annotation.axes, grid.in_affine)))
            post.append(_EYE4 if is_ijk else axes_matrix(annotation.axes, grid.out_affine))
        tensors.append(coords.to(device).contiguous())

    def affine_stage(matrices: list, chosen: list) -> None:
        moved = _launch([tensors[n] for n in chosen], [parameter_block(np.linalg.inv(matrices[n]), inverse=matrices[n]) for n in chosen],
                        [None] * len(chosen))
        for n, tensor in zip(chosen, moved, strict=True):
            tensors[n] = tensor

    # an annotation in other axes than IJK under a displacement field: its conversions cannot be folded into the solve,
    # they are affine-only launches of the same kernel in front of and behind it
    wrapped = [n for n, item in enumerate(items) if item[3].field is not None and not (pre[n] is _EYE4 and post[n] is _EYE4)]
    if wrapped:
        affine_stage(pre, wrapped)
    blocks, fields = [], []
    for n, (_, _, _, grid) in enumerate(items):
        try:
            inverse = np.linalg.inv(grid.matrix)
        except np.linalg.LinAlgError:
            raise ValueError("annotations cannot follow a resampling whose voxel mapping is not invertible") from None
        if grid.field is None:
            total_inverse = post[n] @ inverse @ pre[n]
            blocks.append(parameter_block(np.linalg.inv(total_inverse), inverse=total_inverse))
        else:
            blocks.append(parameter_block(
                grid.matrix, inverse=inverse, out_shape=grid.out_shape, in_spacing=grid.in_affine.spacing, out_spacing=grid.out_affine.spacing,
                affine_first=grid.affine_first, grid=tuple(grid.field.shape[:3]),
            ))
        fields.append(grid.field)
    tensors = _launch(tensors, blocks, fields)
    if wrapped:
        affine_stage(post, wrapped)

    for (annotation, container, key, grid), moved in zip(items, tensors, strict=True):
        moved = moved.to(annotation.data.device)
        if isinstance(annotation, BoundingBoxes):
            corners = moved.reshape(-1, 8, 3)
            hull = torch.cat([corners.amin(dim=1), corners.amax(dim=1)], dim=1)  # axis-aligned, neither clipped nor dropped
            boxes = BoundingBoxes(hull, format=BoundingBoxFormat.IJKIJK, labels=annotation.labels, affine=grid.out_affine.clone(),
                                  metadata=dict(annotation.metadata))
            container[key] = boxes.to_format(annotation.format)
        else:
            container[key] = annotation.new_like(data=moved, affine=grid.out_affine.clone())


def _collect(stores, index: int | None, grid: GridMap | None, items: list) -> None:
    if grid is None:
        return
    for store in stores:
        if not store:
            continue
        container = store if index is None else store[index]
        for key, annotation in container.items():
            items.append((annotation, container, key, grid))


def move_batch(batch, maps: dict[str, list]) -> None:
    """Move every annotation of *batch*: ``maps[name][b]`` is the ``GridMap`` of image *name* at element ``b`` (``None``: that
    element was left alone).  The first name governs the subject-level annotations."""
    if not maps:
        return
    items: list = []
    governing = next(iter(maps.values()))
    for index, grid in enumerate(governing):
        _collect((batch.points, batch.bounding_boxes), index, grid, items)
    for name, grids in maps.items():
        images = batch.images[name]
        for index, grid in enumerate(grids):
            _collect((images.points, images.bounding_boxes), index, grid, items)
    _move_items(items, batch.images[next(iter(maps))].device)


def move_subject(subject, maps: dict[str, GridMap], device) -> None:
    """The same for one ``Subject`` whose images were replaced one by one (``CropOrPad``'s per-image road)."""
    if not maps:
        return
    items: list = []
    _collect((subject._points, subject._bounding_boxes), None, next(iter(maps.values())), items)
    for name, grid in maps.items():
        image = subject._images[name]
        _collect((image._points, image._bounding_boxes), None, grid, items)
    _move_items(items, device)


class _Tracker:
    """The grids of the images a transform is about to change, taken before it does."""

    def __init__(self, batch, images: dict) -> None:
        self.batch = batch
        self.images = images
        self.before = {name: ([affine.clone() for affine in img.affines], tuple(int(s) for s in img._data.shape[2:])) for name, img in images.items()}

    def finish(self, matrix_of: Callable) -> None:
        """``matrix_of(name, index, in_shape, out_shape)`` -> the float64 4x4 output voxel -> input voxel of element *index* of
        image *name*, which went from *in_shape* to *out_shape*, or ``None`` for an element the transform left alone."""
        maps: dict[str, list] = {}
        for name, (affines, in_shape) in self.before.items():
            img = self.images[name]
            out_shape = tuple(int(s) for s in img._data.shape[2:])
            grids = []
            for index, in_affine in enumerate(affines):
                matrix = matrix_of(name, index, in_shape, out_shape)
                grids.append(None if matrix is None else GridMap(matrix, in_affine, img.affines[index], out_shape))
            maps[name] = grids
        move_batch(self.batch, maps)


def track(batch, images: dict) -> _Tracker | None:
    """A tracker for *images* (the ``ImagesBatch``es the transform applies to, in order) when *batch* carries annotations,
    else ``None``: no annotation, no work."""
    if not images or not batch.has_annotations:
        return None
    return _Tracker(batch, images)


# -- the voxel mappings of the grid-changing transforms (output voxel -> input voxel, exact small integers) --------------------
def shift_matrix(start) -> np.ndarray:
    """``in = out + start``: a crop that starts at *start*; a pad of ``p`` leading voxels is ``start = -p``."""
    matrix = np.eye(4)
    matrix[:3, 3] = [float(v) for v in start]
    return matrix


def flip_matrix(axes, shape) -> np.ndarray | None:
    """``in_a = shape_a - 1 - out_a`` along every axis of *axes*; ``None`` without axes."""
    axes = [int(a) for a in axes]
    if not axes:
        return None
    matrix = np.eye(4)
    for axis in axes:
        matrix[axis, axis] = -1.0
        matrix[axis, 3] = float(shape[axis] - 1)
    return matrix


def permute_matrix(perm, flip_axes, in_shape) -> np.ndarray:
    """``tio_permute3d``'s addressing: input axis ``perm[d]`` runs along output axis ``d``, reversed when it is in
    *flip_axes*."""
    matrix = np.zeros((4, 4))
    matrix[3, 3] = 1.0
    for d, source in enumerate(perm):
        flipped = source in flip_axes
        matrix[source, d] = -1.0 if flipped else 1.0
        matrix[source, 3] = float(in_shape[source] - 1) if flipped else 0.0
    return matrix


def resize_matrix(in_shape, out_shape, *, nearest: bool) -> np.ndarray:
    """``F.interpolate``'s source coordinate: ``out (S_in - 1) / (S_out - 1)`` for trilinear ``align_corners=True``,
    ``out S_in / S_out`` for legacy nearest (and along an axis of one voxel, where the first has no inverse)."""
    matrix = np.eye(4)
    for axis in range(3):
        size_in, size_out = int(in_shape[axis]), int(out_shape[axis])
        if nearest or size_in == 1 or size_out == 1:
            matrix[axis, axis] = size_in / size_out
        else:
            matrix[axis, axis] = (size_in - 1) / (size_out - 1)
    return matrix
