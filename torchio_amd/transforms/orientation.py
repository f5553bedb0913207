"""Orientation and shape housekeeping in front of the augmentations (mirror of reference ``transforms/spatial/``
``reorient.py``, ``transpose.py``, ``crop_or_pad.py``, ``ensure_shape_multiple.py``, ``to_reference_space.py`` and
``copy_affine.py``).

``Reorient`` and ``Transpose`` move voxels: one ``tio_permute3d`` launch per image, the flips folded into the
addressing (the reference runs up to three ``torch.flip`` passes and ``permute(...).contiguous()``).  ``CropOrPad`` and
``EnsureShapeMultiple`` are host logic over this package's own ``Pad`` (``tio_pad3d``) and ``Crop`` (a view);
``ToReferenceSpace`` and ``CopyAffine`` change affines only.  File-backed lazy images are out of scope, as for
``Pad`` / ``Crop``: ``Subject`` / ``Image`` inputs take the reference's per-image road with tensors in memory.
"""
from __future__ import annotations

import copy as _copy
import math
from typing import Any

import numpy as np
import torch
from torch import Tensor

from .. import ops
from . import _annotations
from ..data.affine import AffineMatrix
from ..data.affine import axcodes2ornt
from ..data.affine import inv_ornt_aff
from ..data.affine import io_orientation
from ..data.affine import ornt_transform
from ..data.batch import SubjectsBatch
from ..data.image import Image
from ..data.subject import Subject
from .compose import Compose
from .pad import Crop
from .pad import Pad
from .pad import pad_tensor
from .pad import parse_padding_mode
from .transform import AppliedTransform
from .transform import SpatialTransform


# -- Reorient ----------------------------------------------------------------------------------------------------------
def _validate_orientation(orientation: str) -> str:
    """Validate and normalise a 3-letter orientation code (reorient.py:17-45)."""
    if not isinstance(orientation, str) or len(orientation) != 3:
        raise ValueError(f'Orientation must be a 3-letter string, got "{orientation}"')
    orientation = orientation.upper()
    valid_codes = set("RLAPIS")
    if not all(c in valid_codes for c in orientation):
        raise ValueError(f'Orientation code must be composed of three distinct characters in {valid_codes} but got "{orientation}"')
    pairs = [{"R", "L"}, {"A", "P"}, {"S", "I"}]
    if not all(set(orientation) & pair for pair in pairs):
        raise ValueError(
            "Orientation code must include one character for each axis"
            f' direction: R or L, A or P, and S or I, but got "{orientation}"'
        )
    return orientation


def _compute_reorientation(current_affine: np.ndarray, target_codes: str) -> np.ndarray:
    """The (3, 2) orientation transform from the affine's orientation to *target_codes* (reorient.py:48-60)."""
    return ornt_transform(io_orientation(current_affine), axcodes2ornt(tuple(target_codes)))


def _apply_reorientation(data: Tensor, ornt: np.ndarray) -> Tensor:
    """nibabel's ``apply_orientation`` on a (B, C, I, J, K) batch: flip, then transpose, in one launch (reorient.py:63-91)."""
    perm = [int(p) for p in np.argsort(ornt[:, 0])]
    flips = [axis for axis in range(3) if ornt[axis, 1] == -1]
    return ops.engine().permute3d(data, perm, flips)


class Reorient(SpatialTransform):
    """Reorder and flip the voxel axes to a target orientation such as ``'RAS'`` or ``'LPS'`` (reorient.py:94-179)."""

    def __init__(self, orientation: str = "RAS", **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.orientation = _validate_orientation(orientation)

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        first_images = next(iter(batch.images.values()))
        affine_np = first_images.affines[0].numpy()
        current_codes = "".join(first_images.affines[0].orientation)
        ornt = _compute_reorientation(affine_np, self.orientation)
        return {"ornt": ornt.tolist(), "original_orientation": current_codes}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        ornt = np.asarray(params["ornt"])
        if np.array_equal(ornt[:, 0], [0, 1, 2]) and np.all(ornt[:, 1] == 1):  # already there
            return batch
        images = self._get_images(batch)
        tracker = _annotations.track(batch, images)
        for img_batch in images.values():
            original_shape = img_batch.data.shape[-3:]
            img_batch.data = _apply_reorientation(img_batch.data, ornt)
            inv_aff = inv_ornt_aff(ornt, original_shape)
            for affine in img_batch.affines:
                affine._matrix.copy_(torch.as_tensor(affine.numpy() @ inv_aff, dtype=torch.float64))
        if tracker is not None:  # the same permutation and flips as `_apply_reorientation` hands to the kernel
            perm = [int(p) for p in np.argsort(ornt[:, 0])]
            flips = [axis for axis in range(3) if ornt[axis, 1] == -1]
            tracker.finish(lambda name, index, in_shape, out_shape: _annotations.permute_matrix(perm, flips, in_shape))
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "Reorient":
        return Reorient(orientation=params["original_orientation"], copy=False)


# -- Transpose ---------------------------------------------------------------------------------------------------------
class Transpose(SpatialTransform):
    """Swap the first and last spatial axes, (C, I, J, K) -> (C, K, J, I); its own inverse (transpose.py:11-59).

    Like the reference it loops over every image of the batch: ``include`` / ``exclude`` are not consulted."""

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        tracker = _annotations.track(batch, batch.images)
        for img_batch in batch.images.values():
            img_batch.data = ops.engine().permute3d(img_batch.data, (2, 1, 0))
            for affine in img_batch.affines:  # columns 0 and 2 trade places
                m = affine._matrix.clone()
                affine._matrix[:, 0] = m[:, 2]
                affine._matrix[:, 2] = m[:, 0]
        if tracker is not None:
            tracker.finish(lambda name, index, in_shape, out_shape: _annotations.permute_matrix((2, 1, 0), (), in_shape))
        return batch

    @property
    def invertible(self) -> bool:
        return True

    def inverse(self, params: dict[str, Any]) -> "Transpose":
        return Transpose(copy=False)


# -- CropOrPad ---------------------------------------------------------------------------------------------------------
def _parse_target_shape(target_shape) -> tuple[float | None, float | None, float | None]:
    """One number for every axis, or three entries where ``None`` keeps an axis (crop_or_pad.py:50-66)."""
    if isinstance(target_shape, (int, float)):
        return (float(target_shape), float(target_shape), float(target_shape))
    values = list(target_shape)
    if len(values) == 3:
        a, b, c = values
        return (None if a is None else float(a), None if b is None else float(b), None if c is None else float(c))
    raise ValueError(f"target_shape must have 1 or 3 values, got {len(values)}")


def _to_voxels(target, units: str, spacing, current_shape) -> tuple[int, int, int]:
    """The target in whole voxels; ``None`` entries take the current size (crop_or_pad.py:69-88)."""
    result: list[int] = []
    for t, sp, cur in zip(target, spacing, current_shape, strict=True):
        if t is None:
            result.append(cur)
        elif units == "voxels":
            result.append(round(t))
        else:
            factor = 10.0 if units == "cm" else 1.0
            result.append(round(t * factor / sp))
    return (result[0], result[1], result[2])


def _split_per_axis(diff: int, location: str) -> tuple[tuple[int, int], tuple[int, int]]:
    """(pad_ini, pad_fin), (crop_ini, crop_fin) of one axis: ceil in front, floor behind (crop_or_pad.py:91-107)."""
    if diff > 0:
        return (math.ceil(diff / 2), math.floor(diff / 2)), (0, 0)
    if diff < 0:
        amount = -diff
        if location == "random":
            ini = int(torch.randint(0, amount + 1, (1,)).item())
        else:
            ini = math.ceil(amount / 2)
        return (0, 0), (ini, amount - ini)
    return (0, 0), (0, 0)


def _compute_crop_and_pad(current_shape, target_shape, *, only_crop: bool, only_pad: bool, location: str = "center"):
    """``(padding_six, cropping_six)``, either ``None`` when nothing is to do or suppressed (crop_or_pad.py:110-161)."""
    pad_values: list[int] = []
    crop_values: list[int] = []
    for cur, tgt in zip(current_shape, target_shape, strict=True):
        pad, crop = _split_per_axis(tgt - cur, location)
        pad_values.extend(pad)
        crop_values.extend(crop)
    padding = tuple(pad_values) if any(v > 0 for v in pad_values) and not only_crop else None
    cropping = tuple(crop_values) if any(v > 0 for v in crop_values) and not only_pad else None
    return padding, cropping


def _shifted_affine(image: Image, start) -> AffineMatrix:
    matrix = image.affine.data.clone()
    matrix[:3, 3] += matrix[:3, :3] @ matrix.new_tensor([float(v) for v in start])
    return AffineMatrix(matrix)


def _new_like(image: Image, data: Tensor, affine: AffineMatrix) -> Image:
    # (the annotations ride along as they are; `_apply_per_image` moves them once all images stand on the new grid)
    return type(image)(data, affine=affine, points=image.points, bounding_boxes=image.bounding_boxes, **_copy.deepcopy(image.metadata))


def _pad_image(image: Image, padding, padding_mode: str, fill: float) -> Image:
    """crop_or_pad.py:319-346, for an image in memory."""
    i0, _, j0, _, k0, _ = padding
    data, home = image.data, image.data.device
    if home.type == "cpu" and ops.engine().device_type == "cuda" and torch.cuda.is_available():
        data = data.to("cuda")  # host-resident data are staged through the engine's device, as in Transform._forward
    padded = pad_tensor(data, padding, padding_mode, fill).to(home)
    return _new_like(image, padded, _shifted_affine(image, (-i0, -j0, -k0)))


def _crop_image(image: Image, cropping) -> Image:
    """crop_or_pad.py:265-285, for an image in memory."""
    i0, i1, j0, j1, k0, k1 = cropping
    _, si, sj, sk = image.shape
    data = image.data[:, i0 : si - i1 or None, j0 : sj - j1 or None, k0 : sk - k1 or None]
    return _new_like(image, data, _shifted_affine(image, (i0, j0, k0)))


class CropOrPad(SpatialTransform):
    """Crop and / or pad to a target spatial shape given in voxels, mm or cm (crop_or_pad.py:381-635)."""

    def __init__(self, target_shape, *, units: str = "voxels", padding_mode: str = "constant", fill: float = 0,
                 only_crop: bool = False, only_pad: bool = False, location: str = "center", **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if only_crop and only_pad:
            raise ValueError("only_crop and only_pad cannot both be True")
        if units not in ("voxels", "mm", "cm"):
            raise ValueError(f"units must be 'voxels', 'mm', or 'cm', got {units!r}")
        if location not in ("center", "random"):
            raise ValueError(f"location must be 'center' or 'random', got {location!r}")
        self.target_shape = _parse_target_shape(target_shape)
        self.units = units
        self.padding_mode = parse_padding_mode(padding_mode)
        self.fill = fill
        self.only_crop = only_crop
        self.only_pad = only_pad
        self.location = location

    def forward(self, data):
        """``Subject`` and ``Image`` inputs go image by image and record ``Pad``, ``Crop`` and ``CropOrPad`` entries, like
        the reference's lazy road (crop_or_pad.py:464-562); every other input takes the batch road."""
        if isinstance(data, (Subject, Image)):
            return self._forward_per_image(data)
        return super().forward(data)

    def _forward_per_image(self, data):
        is_image = isinstance(data, Image)
        subject = Subject(tio_default_image=data) if is_image else data
        if self.copy:
            subject = _copy.deepcopy(subject)
        if torch.rand(1).item() > self.p:
            return subject.tio_default_image if is_image else subject
        first_image = next(iter(subject.images.values()))
        current_shape = first_image.spatial_shape
        target_voxels = _to_voxels(self.target_shape, self.units, first_image.affine.spacing, current_shape)
        padding, cropping = _compute_crop_and_pad(
            current_shape, target_voxels, only_crop=self.only_crop, only_pad=self.only_pad, location=self.location
        )
        self._apply_per_image(subject, padding, cropping)
        return subject.tio_default_image if is_image else subject

    def _selected(self, subject: Subject) -> dict[str, Image]:
        images = subject.images
        if self.include is not None:
            images = {k: v for k, v in images.items() if k in self.include}
        if self.exclude is not None:
            images = {k: v for k, v in images.items() if k not in self.exclude}
        return images

    def _grids_before(self, subject: Subject):
        """The selected images' affines when the subject carries annotations (``None`` otherwise: nothing to move)."""
        if not subject.all_points() and not subject.all_bounding_boxes():
            return None
        return {name: image.affine.clone() for name, image in self._selected(subject).items()}

    @staticmethod
    def _move_annotations(subject: Subject, before, start) -> None:
        if not before:
            return
        maps = {
            name: _annotations.GridMap(_annotations.shift_matrix(start), affine, subject._images[name].affine, subject._images[name].spatial_shape)
            for name, affine in before.items()
        }
        device = next(iter(subject._images.values())).device
        if device.type == "cpu" and ops.engine().device_type == "cuda" and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())  # staged through the engine's device, like `_pad_image`
        _annotations.move_subject(subject, maps, device)

    def _apply_per_image(self, subject: Subject, padding, cropping) -> None:
        include = None if self.include is None else list(self.include)
        exclude = None if self.exclude is None else list(self.exclude)
        if padding is not None:
            before = self._grids_before(subject)
            for name, image in self._selected(subject).items():
                subject._images[name] = _pad_image(image, padding, self.padding_mode, self.fill)
            self._move_annotations(subject, before, (-padding[0], -padding[2], -padding[4]))
            params = {"padding": padding, "padding_mode": self.padding_mode, "fill": self.fill}
            subject.applied_transforms.append(AppliedTransform(name="Pad", params=params, include=include, exclude=exclude))
        if cropping is not None:
            before = self._grids_before(subject)
            for name, image in self._selected(subject).items():
                subject._images[name] = _crop_image(image, cropping)
            self._move_annotations(subject, before, (cropping[0], cropping[2], cropping[4]))
            subject.applied_transforms.append(AppliedTransform(name="Crop", params={"cropping": cropping}, include=include, exclude=exclude))
        params = {"padding": padding, "cropping": cropping}
        subject.applied_transforms.append(AppliedTransform(name="CropOrPad", params=params, include=include, exclude=exclude))

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        first_images = next(iter(batch.images.values()))
        spacing = first_images.affines[0].spacing
        current_shape = tuple(int(s) for s in first_images.data.shape[-3:])
        target_voxels = _to_voxels(self.target_shape, self.units, spacing, current_shape)
        padding, cropping = _compute_crop_and_pad(
            current_shape, target_voxels, only_crop=self.only_crop, only_pad=self.only_pad, location=self.location
        )
        return {"padding": padding, "cropping": cropping}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        padding, cropping = params["padding"], params["cropping"]
        transforms: list[SpatialTransform] = []
        if padding is not None:
            transforms.append(Pad(padding=padding, padding_mode=self.padding_mode, fill=self.fill, include=self.include, exclude=self.exclude))
        if cropping is not None:
            transforms.append(Crop(cropping=cropping, include=self.include, exclude=self.exclude))
        if transforms:
            batch = Compose(transforms, copy=False)(batch)
        return batch


# -- EnsureShapeMultiple -----------------------------------------------------------------------------------------------
def _parse_target_multiple(value) -> tuple[int, int, int]:
    """One positive int for every axis, or three (ensure_shape_multiple.py:23-38)."""
    if isinstance(value, int):
        if value < 1:
            raise ValueError(f"target_multiple must be >= 1, got {value}")
        return (value, value, value)
    values = tuple(value)
    if len(values) != 3:
        raise ValueError(f"target_multiple must have 1 or 3 values, got {len(values)}")
    for v in values:
        if v < 1:
            raise ValueError(f"All target_multiple values must be >= 1, got {v}")
    return (values[0], values[1], values[2])


def _compute_target_shape(current_shape, target_multiple, method: str) -> tuple[int, int, int]:
    """Every axis rounded up (``pad``) or down (``crop``) to its multiple, never below 1 (ensure_shape_multiple.py:41-55)."""
    result: list[int] = []
    for size, multiple in zip(current_shape, target_multiple, strict=True):
        target = (math.ceil(size / multiple) if method == "pad" else math.floor(size / multiple)) * multiple
        result.append(max(target, 1))
    return (result[0], result[1], result[2])


class EnsureShapeMultiple(SpatialTransform):
    """Pad up or crop down until every spatial size is a multiple of ``target_multiple`` (ensure_shape_multiple.py:58-178)."""

    def __init__(self, target_multiple, *, method: str = "pad", padding_mode: str = "constant", fill: float = 0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.target_multiple = _parse_target_multiple(target_multiple)
        if method not in ("crop", "pad"):
            raise ValueError(f"method must be 'crop' or 'pad', got {method!r}")
        self.method = method
        self.padding_mode = parse_padding_mode(padding_mode)
        self.fill = fill

    def _crop_or_pad(self, target_shape, **kwargs: Any) -> CropOrPad:
        return CropOrPad(
            target_shape=target_shape, padding_mode=self.padding_mode, fill=self.fill, only_crop=self.method == "crop",
            only_pad=self.method == "pad", include=self.include, exclude=self.exclude, **kwargs,
        )

    def forward(self, data: Any) -> Any:
        if isinstance(data, (Subject, Image)):
            target_shape = _compute_target_shape(data.spatial_shape, self.target_multiple, self.method)
            return self._crop_or_pad(target_shape, p=self.p, copy=self.copy).forward(data)
        return super().forward(data)

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        first_images = next(iter(batch.images.values()))
        current_shape = tuple(int(s) for s in first_images.data.shape[-3:])
        return {"target_shape": _compute_target_shape(current_shape, self.target_multiple, self.method)}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        crop_or_pad = self._crop_or_pad(params["target_shape"], copy=False)
        return crop_or_pad.apply_transform(batch, crop_or_pad.make_params(batch))


# -- ToReferenceSpace / CopyAffine -------------------------------------------------------------------------------------
def _reference_space_affine(reference: Image, output_shape) -> AffineMatrix:
    """The affine of a grid of *output_shape* that covers the reference's field of view: same centre and orientation,
    spacing scaled by the ratio of the shapes (to_reference_space.py:98-132)."""
    ref_affine = reference.affine
    rotation = ref_affine.direction.cpu().numpy().astype(np.float64)
    ref_spacing = np.asarray(ref_affine.spacing, dtype=np.float64)
    ref_origin = np.asarray(ref_affine.origin, dtype=np.float64)
    ref_shape = np.asarray(reference.spatial_shape, dtype=np.float64)
    new_shape = np.asarray(output_shape, dtype=np.float64)
    new_spacing = ref_spacing * (ref_shape / new_shape)
    center = ref_origin + rotation @ (((ref_shape - 1) / 2) * ref_spacing)
    new_origin = center - rotation @ (((new_shape - 1) / 2) * new_spacing)
    matrix = np.eye(4, dtype=np.float64)
    matrix[:3, :3] = rotation * new_spacing
    matrix[:3, 3] = new_origin
    return AffineMatrix(matrix)


class ToReferenceSpace(SpatialTransform):
    """Give an image the field of view of a reference image; the data stay as they are (to_reference_space.py:17-95)."""

    def __init__(self, reference: Image, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if not isinstance(reference, Image):
            raise TypeError(f"reference must be a TorchIO Image, got {type(reference).__name__}")
        self.reference = reference

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        images = self._get_images(batch)
        tracker = _annotations.track(batch, images)
        for img_batch in images.values():
            new_affine = _reference_space_affine(self.reference, tuple(int(s) for s in img_batch.data.shape[2:]))
            img_batch.affines[:] = [new_affine.clone() for _ in img_batch.affines]
        if tracker is not None:  # the voxels stay: IJK coordinates keep their values, anatomical ones follow the new affine
            tracker.finish(lambda name, index, in_shape, out_shape: np.eye(4))
        return batch

    @staticmethod
    def from_tensor(tensor: Tensor, reference: Image) -> Image:
        """An image of the reference's class with *tensor* as data and the reference-space affine."""
        new_affine = _reference_space_affine(reference, tuple(int(s) for s in tensor.shape[-3:]))
        return type(reference)(tensor, affine=new_affine)


class CopyAffine(SpatialTransform):
    """Copy the affine of the image named ``target`` to every other image (copy_affine.py:12-57)."""

    def __init__(self, target: str, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.target = target

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        if self.target not in batch.images:
            raise KeyError(f"Reference image '{self.target}' not found. Available: {list(batch.images.keys())}")
        ref_affines = batch.images[self.target].affines
        # the voxels stay, so the annotations stay ON their voxels: IJK coordinates keep their values
        # and adopt the new affine, anatomical ones are re-expressed through it
        tracker = _annotations.track(batch, batch.images)
        for name, img_batch in batch.images.items():
            if name == self.target:
                continue
            for i, affine in enumerate(img_batch.affines):
                affine._matrix.copy_(ref_affines[i]._matrix)
        if tracker is not None:
            tracker.finish(lambda name, index, in_shape, out_shape: None if name == self.target else np.eye(4))
        return batch
