"""Tensor-backed images (mirror of the in-memory part of reference ``data/image.py``).

The reference ``Image`` is a lazy, file-backed object (image.py:104); the
augmentation path only ever sees its ``(C, I, J, K)`` tensor and its affine, so
this mirror keeps exactly those.  An image built from a ``pathlib.Path`` (or ``Image.from_file``) is file-backed and lazy
as in the reference: NIfTI-1 ``.nii`` / ``.nii.gz`` only (``data/nifti.py``), header attributes without a load, the voxels
decoded on first use - on the device when that is where the image is going (``tio_nifti_decode``).
"""
from __future__ import annotations

import copy as _copy
import os
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

from . import nifti as _nifti
from .affine import AffineMatrix
from .bboxes import BoundingBoxes
from .points import Points


def _parse_annotations(annotations, expected: type) -> dict:
    """A shallow copy of a ``{name: Points}`` / ``{name: BoundingBoxes}`` dict (``None``: empty), every value checked."""
    if annotations is None:
        return {}
    for key, value in annotations.items():
        if not isinstance(value, expected):
            raise TypeError(f"Expected {expected.__name__} for key {key!r}, got {type(value).__name__}")
    return dict(annotations)


class Image:
    """A 4-D ``(C, I, J, K)`` tensor plus its voxel-to-world affine."""

    def __init__(self, data, *, affine=None, points=None, bounding_boxes=None, **metadata) -> None:
        self._points = _parse_annotations(points, Points)
        self._bounding_boxes = _parse_annotations(bounding_boxes, BoundingBoxes)
        self._header = None  # file-backed images: the parsed NIfTI header; the voxels come on first use
        self._tensor = None
        self._destination = (torch.device("cpu"), None)  # where (and as which dtype) an unloaded image will be decoded
        if isinstance(data, (Path, _nifti.NiftiHeader)):
            self._header = data if isinstance(data, _nifti.NiftiHeader) else _nifti.read_header(data)  # (a header: a copy of an image)
            if affine is None:
                affine = self._header.affine
        else:
            if isinstance(data, np.ndarray):
                data = torch.as_tensor(data)
            if not isinstance(data, Tensor):
                hint = " (to read a file, use Image.from_file(path) or pass a pathlib.Path)" if isinstance(data, (str, os.PathLike)) else ""
                raise TypeError(f"Image data must be a tensor or ndarray, got {type(data).__name__}{hint}")
            if data.ndim == 3:
                data = data.unsqueeze(0)
            if data.ndim != 4:
                raise ValueError(f"Image data must be 4D (C, I, J, K), got {data.ndim}D")
            self._tensor = data
        self._affine = affine if isinstance(affine, AffineMatrix) else AffineMatrix(affine)
        self.metadata = dict(metadata)
        self.applied_transforms: list = []

    @classmethod
    def from_file(cls, path, *, device=None, dtype=None, affine=None, **metadata) -> "Image":
        """A lazy image over a ``.nii`` / ``.nii.gz`` file: only the header is read now.  *device*: where the voxels will be
        decoded (default: the host); *dtype*: what they are converted to (default: the file's natural type); *affine*:
        replaces the header's."""
        new = cls(Path(os.fspath(path)), affine=affine, **metadata)
        new._destination = (torch.device("cpu" if device is None else device), dtype)
        return new

    # -- file-backed images --------------------------------------------------
    @property
    def path(self) -> Path | None:
        """The file behind this image (``None`` for tensor-backed images)."""
        return None if self._header is None else Path(self._header.path)

    @property
    def is_loaded(self) -> bool:
        return self._tensor is not None

    def load(self, device=None) -> "Image":
        """Read and decode the voxels now (once; later calls only move them when a *device* is given)."""
        if self._tensor is None:
            where, dtype = self._destination
            self._tensor = _nifti.read_tensor(self._header, where if device is None else torch.device(device), dtype)
        elif device is not None:
            self._tensor = self._tensor.to(device)
        return self

    def save(self, path, *, compresslevel: int = 1) -> None:
        """Write the image as NIfTI-1 (``.nii`` / ``.nii.gz``, ``data/nifti.py:write_nifti``); other suffixes raise ``ValueError``."""
        if not _nifti.is_nifti_path(path):
            raise ValueError(f"Cannot save to {os.fspath(path)!r}: only .nii and .nii.gz are written here (there is no SimpleITK)")
        _nifti.write_nifti(path, self.data, self._affine, compresslevel=compresslevel)

    # -- accessors -----------------------------------------------------------
    @property
    def _data(self) -> Tensor:
        """The voxels; a file-backed image loads them at the first read."""
        if self._tensor is None:
            self.load()
        return self._tensor

    @_data.setter
    def _data(self, value: Tensor) -> None:
        self._tensor = value

    @property
    def data(self) -> Tensor:
        return self._data

    def set_data(self, value: Tensor) -> None:
        if value.ndim != 4:
            raise ValueError(f"Image data must be 4D, got {value.ndim}D")
        self._data = value

    @property
    def affine(self) -> AffineMatrix:
        return self._affine

    @affine.setter
    def affine(self, value) -> None:
        self._affine = value if isinstance(value, AffineMatrix) else AffineMatrix(value)

    @property
    def shape(self) -> tuple[int, int, int, int]:
        if self._tensor is None:
            return (self._header.channels, *self._header.shape)
        return tuple(self._tensor.shape)  # type: ignore[return-value]

    @property
    def spatial_shape(self) -> tuple[int, int, int]:
        return tuple(int(s) for s in self.shape[1:])  # type: ignore[return-value]

    @property
    def num_channels(self) -> int:
        return int(self.shape[0])

    @property
    def spacing(self) -> tuple[float, float, float]:
        return self._affine.spacing

    @property
    def device(self) -> torch.device:
        return self._destination[0] if self._tensor is None else self._tensor.device

    @property
    def dtype(self) -> torch.dtype:
        if self._tensor is None:
            return self._destination[1] or self._header.natural_dtype
        return self._tensor.dtype

    def __getitem__(self, item):
        """Metadata lookup (``str``) or a crop along ``(C, I, J, K)`` with the affine origin moved (image.py:832-899).

        Integers keep their axis (size 1), one ``Ellipsis`` expands to full slices and missing
        trailing indices are full slices (``normalize_index``, data/backends.py:52-106).  The
        result is a view of the same storage on the same device - what the patch samplers
        hand to a ``DataLoader`` or ``Queue``.
        """
        if isinstance(item, str):
            if item in self.metadata:
                return self.metadata[item]
            raise KeyError(f"{type(self).__name__} has no metadata key {item!r}")
        sc, si, sj, sk = _normalize_index(item)
        cropped = self._read_box(sc, si, sj, sk) if self._tensor is None else None
        if cropped is None:
            cropped = self._data[sc, si, sj, sk]
        matrix = self._affine.data.clone()
        starts = [axis.indices(size)[0] for axis, size in zip((si, sj, sk), self.shape[1:], strict=True)]
        matrix[:3, 3] += matrix[:3, :3] @ torch.tensor(starts, dtype=torch.float64, device=matrix.device)
        new = type(self)(cropped, affine=AffineMatrix(matrix), **self._copied_annotations(), **_copy.deepcopy(self.metadata))
        new.applied_transforms = list(self.applied_transforms)
        return new

    def _read_box(self, *slices) -> Tensor | None:
        """The voxels of a crop of an UNLOADED file-backed image, reading (from a ``.nii``) only that box; the image stays
        unloaded.  ``None`` for strided or empty slices (the caller loads everything)."""
        box = []
        for axis, size in zip(slices, self.shape, strict=True):
            start, stop, step = axis.indices(size)
            if step != 1 or stop <= start:
                return None
            box.append((start, stop))
        where, dtype = self._destination
        return _nifti.read_tensor(self._header, where, dtype, box=tuple(box))

    # -- annotations ---------------------------------------------------------
    @property
    def points(self) -> dict[str, Points]:
        """Named point sets attached to this image (image.py:524-526)."""
        return self._points

    @property
    def bounding_boxes(self) -> dict[str, BoundingBoxes]:
        """Named box sets attached to this image (image.py:529-531)."""
        return self._bounding_boxes

    def _copied_annotations(self, memo=None) -> dict:
        return {
            "points": {key: _copy.deepcopy(value, memo) for key, value in self._points.items()},
            "bounding_boxes": {key: _copy.deepcopy(value, memo) for key, value in self._bounding_boxes.items()},
        }

    def new_like(self, *, data, affine=None) -> "Image":
        """A new image of this class around *data*: metadata and annotations copied, this affine unless one is given
        (image.py:670-697)."""
        new_affine = self._affine.clone() if affine is None else (affine if isinstance(affine, AffineMatrix) else AffineMatrix(affine))
        return type(self)(data, affine=new_affine, **self._copied_annotations(), **dict(self.metadata))

    def to(self, *args, **kwargs) -> "Image":
        if self._tensor is None:  # not loaded yet: only record where (and as what) the voxels will be decoded
            device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
            self._destination = (self._destination[0] if device is None else device, self._destination[1] if dtype is None else dtype)
        else:
            self._tensor = self._tensor.to(*args, **kwargs)
        for annotation in (*self._points.values(), *self._bounding_boxes.values()):
            annotation.to(*args, **kwargs)
        return self

    def numpy(self) -> np.ndarray:
        return self._data.detach().cpu().numpy()

    def __deepcopy__(self, memo):
        if self._tensor is None:  # an unloaded image stays unloaded
            new = type(self)(self._header, affine=self._affine.clone(), **self._copied_annotations(memo), **_copy.deepcopy(self.metadata, memo))
            new._destination = self._destination
            new.applied_transforms = list(self.applied_transforms)
            return new
        new = type(self)(self._tensor.clone(), affine=self._affine.clone(), **self._copied_annotations(memo), **_copy.deepcopy(self.metadata, memo))
        new.applied_transforms = list(self.applied_transforms)
        return new

    def __repr__(self) -> str:
        annotations = ""
        if self._points:
            annotations += f", points={{{', '.join(self._points)}}}"
        if self._bounding_boxes:
            annotations += f", bboxes={{{', '.join(self._bounding_boxes)}}}"
        source = "" if self._header is None else f", path={self._header.path!r}, loaded={self.is_loaded}"
        return f"{type(self).__name__}(shape={self.shape}, dtype={self.dtype}, device={self.device}{source}{annotations})"


def _normalize_index(item, ndim: int = 4) -> tuple[slice, ...]:
    """An index as exactly ``ndim`` slices (data/backends.py:52-106)."""
    if isinstance(item, (int, slice)) or item is Ellipsis:
        items = (item,)
    elif isinstance(item, tuple):
        items = item
    else:
        raise TypeError(f"Index type {type(item).__name__} not understood")
    if sum(1 for entry in items if entry is Ellipsis) > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if any(entry is Ellipsis for entry in items):
        position = next(index for index, entry in enumerate(items) if entry is Ellipsis)
        fill = max(ndim - (len(items) - 1), 0)
        items = (*items[:position], *([slice(None)] * fill), *items[position + 1 :])
    if len(items) > ndim:
        raise IndexError(f"Too many indices: expected at most {ndim} (C, I, J, K), got {len(items)}")
    parsed = []
    for entry in items:
        if isinstance(entry, bool) or not isinstance(entry, (int, slice)):
            raise TypeError(f"Index type {type(entry).__name__} not understood")
        if isinstance(entry, int):  # keep the axis; slice(-1, 0) would be empty
            parsed.append(slice(entry, None) if entry == -1 else slice(entry, entry + 1))
        else:
            parsed.append(entry)
    parsed += [slice(None)] * (ndim - len(parsed))
    return tuple(parsed)


class ScalarImage(Image):
    """Intensity image: linear interpolation, touched by intensity transforms."""


class LabelMap(Image):
    """Label map: nearest-neighbour interpolation, skipped by intensity transforms."""


def read_image(path, *, image_class: type[Image] = ScalarImage, **kwargs) -> Image:
    """``image_class.from_file(path, **kwargs)``: a lazy image over a ``.nii`` / ``.nii.gz`` file."""
    return image_class.from_file(path, **kwargs)
