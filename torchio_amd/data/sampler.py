"""Patch samplers: where patches go, and how they are cut out of a (possibly GPU-resident) subject.

Public contract = the reference's (``src/torchio/data/sampler.py``: ``PatchSampler``, ``GridSampler``,
``UniformSampler``, ``WeightedSampler``, ``LabelSampler`` with the same constructor arguments, the same
consumption of the global CPU generator and the same errors), implemented here around three small
pieces:

* :func:`axis_origins` / :func:`grid_placements` — the regular grid of a dense-inference sampler as pure
  functions of (extent, patch, overlap);
* :func:`cut` — a patch is four views (``Image.__getitem__``: no copy, affine origin moved) of
  whatever tensors the subject holds, so a subject that lives in HBM yields device-resident patches and the
  feeding side of the hot path never crosses PCIe;
* :class:`CentreLaw` — a discrete distribution over patch CENTRES (probability map or label weights) with
  the voxels whose patch would stick out of the volume masked by broadcasting three 1-D masks.

Beyond the reference: :meth:`PatchSampler.sample_batch` / :meth:`GridSampler.batches` hand out a whole batch of patches — the
collation of as many cut patches, each image's voxels from one ``Engine.patch_gather`` launch (:func:`gather_batch`) — and
:func:`set_centre_draw` lets the weighted samplers draw a batch's centres on the device (``Engine.centre_draw``; opt-in, the
reference's host draw stays the default and iteration never changes).

``GridSampler`` pairs with :class:`~torchio_amd.data.aggregator.PatchAggregator`.
"""
from __future__ import annotations

import itertools
from collections.abc import Iterator
from typing import Any

import torch
from torch import Tensor
from torch.utils.data import Dataset
from torch.utils.data import IterableDataset

from .batch import SubjectsBatch
from .patch import PatchLocation
from .subject import Subject

Triple = tuple[int, int, int]


def _triple(value) -> Triple:
    return (value, value, value) if isinstance(value, int) else tuple(value)  # type: ignore[return-value]


def axis_origins(extent: int, patch: int, overlap: int) -> list[int]:
    """First voxels of the patches along one axis: stride ``patch - overlap``, plus one flush with the far end."""
    last = max(extent - patch, 0)
    stride = max(patch - overlap, 1)
    origins = list(range(0, extent - patch + 1, stride))
    if not origins or origins[-1] != last:
        origins.append(last)
    return origins


def grid_placements(shape: Triple, patch: Triple, overlap: Triple) -> list[PatchLocation]:
    """Every patch of the regular grid, k fastest (the order the aggregator's batches arrive in)."""
    per_axis = [axis_origins(shape[d], patch[d], overlap[d]) for d in range(3)]
    return [PatchLocation(index=origin, size=patch) for origin in itertools.product(*per_axis)]


def cut(subject: Subject, where: PatchLocation) -> Subject:
    """The sub-volume *where* of every image of *subject* (views), metadata carried over, tagged with its location."""
    window = (slice(None), *where.to_slices())
    fields: dict[str, Any] = {name: image[window] for name, image in subject.images.items()}
    fields.update(subject.metadata)
    fields["patch_location"] = where
    return Subject(**fields)


def corner_of(centre: Triple, shape: Triple, patch: Triple) -> Triple:
    """Patch corner for a centre voxel, pushed back inside the volume where the patch would overhang."""
    return tuple(min(max(centre[d] - patch[d] // 2, 0), shape[d] - patch[d]) for d in range(3))  # type: ignore[return-value]


class CentreLaw:
    """Unnormalised probability of every voxel being a patch centre, as a flat CPU vector to draw from."""

    def __init__(self, weights: Tensor, patch: Triple) -> None:
        shape = tuple(weights.shape)
        allowed = torch.ones(shape, dtype=torch.bool, device=weights.device)
        for axis in range(3):
            half = patch[axis] // 2
            position = torch.arange(shape[axis], device=weights.device)
            inside = (position >= half) & (position < shape[axis] - half) if half > 0 else torch.ones_like(position, dtype=torch.bool)
            view = [1, 1, 1]
            view[axis] = shape[axis]
            allowed &= inside.view(view)
        self.shape: Triple = shape  # type: ignore[assignment]
        self.map = torch.where(allowed, weights, torch.zeros((), dtype=weights.dtype, device=weights.device))

    def flat_cpu(self) -> Tensor:
        # the draw must consume the global CPU generator like the reference's: a device-resident map comes over once
        return self.map.reshape(-1).cpu()

    def centre(self, flat_index: int) -> Triple:
        ij, k = divmod(flat_index, self.shape[2])
        i, j = divmod(ij, self.shape[1])
        return (i, j, k)


_CENTRE_DRAW = "reference"


def set_centre_draw(mode: str) -> None:
    """Where ``WeightedSampler.sample_batch`` / ``LabelSampler.sample_batch`` draw their patch centres.

    ``"reference"`` (default): one ``torch.multinomial`` on the host per patch, consuming the global CPU generator exactly
    as the reference does.  ``"device"``: one ``Engine.centre_draw`` per call from the package's own Philox stream (stream
    id 2), seeded with ONE ``torch.randint(0, 2**62, (1,))`` from the global CPU generator — reproducible under
    ``torch.manual_seed``, but other centres than the reference's and another consumption of the generator.  Iterating a
    sampler is the reference's road in both modes.
    """
    global _CENTRE_DRAW
    if mode not in ("reference", "device"):
        raise ValueError(f"centre draw mode must be 'reference' or 'device', got {mode!r}")
    _CENTRE_DRAW = mode


def get_centre_draw() -> str:
    return _CENTRE_DRAW


def gather_batch(subject: Subject, locations: list[PatchLocation], corners_dev: Tensor | None = None) -> SubjectsBatch:
    """``SubjectsBatch.from_subjects([cut(subject, where) for where in locations])``, each image's voxels from ONE
    ``Engine.patch_gather`` launch where the subject lives on the GPU.  Affines, annotations and metadata are those of the
    slicing road; a host-resident subject, a non-contiguous image and a patch that does not fit take that road for the voxels
    too.  *corners_dev*: the corners as a device draw left them (int32 ``(N, 3)``), else they go up in one staged copy."""
    patches = [cut(subject, where) for where in locations]
    if not patches:
        raise ValueError("Cannot create batch from empty list")
    size = locations[0].size
    images = list(subject.images.values())
    fits = all(where.size == size for where in locations) and all(
        image.data.device.type == "cuda" and image.data.is_contiguous() and all(p <= s for p, s in zip(size, image.data.shape[1:], strict=True))
        for image in images
    )
    if not fits or not images or any(image.data.device != images[0].data.device for image in images):
        return SubjectsBatch.from_subjects(patches)
    from ..ops import engine  # noqa: PLC0415
    from ..ops import h2d  # noqa: PLC0415

    if corners_dev is None:  # one small copy through the pinned staging ring
        corners_dev = h2d(torch.tensor([where.index for where in locations], dtype=torch.int32).reshape(-1, 3), images[0].data.device)
    data = {name: engine().patch_gather(image.data, corners_dev, size) for name, image in subject.images.items()}
    return SubjectsBatch.from_subjects(patches, data=data)


class PatchSampler:
    """Common part: the patch size and the cutting (reference sampler.py:24-72)."""

    def __init__(self, patch_size) -> None:
        self.patch_size: Triple = _triple(patch_size)

    def __call__(self, subject: Subject, num_patches: int | None = None) -> Iterator[Subject]:
        raise NotImplementedError(f"{type(self).__name__} must implement __call__")

    def _extract_patch(self, subject: Subject, location: PatchLocation) -> Subject:
        return cut(subject, location)

    def sample_batch(self, subject: Subject, num_patches: int) -> SubjectsBatch:
        """``num_patches`` patches of *subject* as one batch: the collation of as many patches of ``self(subject)``."""
        raise NotImplementedError(f"{type(self).__name__} must implement sample_batch")


class GridSampler(PatchSampler, Dataset):
    """Dense inference: a map-style dataset of the grid's patches (reference sampler.py:75-190)."""

    def __init__(self, subject: Subject, patch_size, patch_overlap=0, padding_mode=None, fill: float = 0) -> None:
        super().__init__(patch_size)
        self.patch_overlap: Triple = _triple(patch_overlap)
        self.padding_mode = padding_mode
        self.fill = fill
        self.subject = subject if padding_mode is None else self._padded(subject)
        self.locations = grid_placements(tuple(self.subject.spatial_shape), self.patch_size, self.patch_overlap)

    def _padded(self, subject: Subject) -> Subject:
        """Half an overlap of context on every side, so that border patches are blended like inner ones."""
        from ..transforms.pad import Pad  # noqa: PLC0415

        padding = tuple(itertools.chain.from_iterable((o // 2, o // 2) for o in self.patch_overlap))
        return Pad(padding=padding, padding_mode=self.padding_mode, fill=self.fill, copy=False)(subject)

    def __len__(self) -> int:
        return len(self.locations)

    def __getitem__(self, index: int) -> Subject:
        return cut(self.subject, self.locations[index])

    def batches(self, batch_size: int) -> Iterator[SubjectsBatch]:
        """The grid in ``locations`` order, ``batch_size`` patches at a time (the last batch may be shorter): what collating
        consecutive items yields, with one gather launch per image and batch."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size}")
        for start in range(0, len(self.locations), batch_size):
            yield gather_batch(self.subject, self.locations[start : start + batch_size])


class _RandomSampler(PatchSampler, IterableDataset):
    """Iterable samplers: an endless (or ``num_patches`` long) stream of patches of one subject."""

    def __init__(self, subject: Subject, patch_size, num_patches: int | None = None) -> None:
        super().__init__(patch_size)
        self.subject = subject
        self.num_patches = num_patches

    def __iter__(self) -> Iterator[Subject]:
        return self(self.subject, self.num_patches)

    def __call__(self, subject: Subject, num_patches: int | None = None) -> Iterator[Subject]:
        corners = self._corners(subject)
        budget = num_patches or self.num_patches
        stream = corners if budget is None else itertools.islice(corners, budget)
        return (cut(subject, PatchLocation(index=corner, size=self.patch_size)) for corner in stream)

    def _corners(self, subject: Subject) -> Iterator[Triple]:
        raise NotImplementedError

    def _batch_corners(self, subject: Subject, num_patches: int) -> tuple[list[Triple], Tensor | None]:
        """The corners of one batch on the host and, where a device draw made them, on the device as well."""
        return list(itertools.islice(self._corners(subject), num_patches)), None

    def sample_batch(self, subject: Subject, num_patches: int) -> SubjectsBatch:
        corners, corners_dev = self._batch_corners(subject, int(num_patches))
        return gather_batch(subject, [PatchLocation(index=corner, size=self.patch_size) for corner in corners], corners_dev)


class UniformSampler(_RandomSampler):
    """Corners uniform over the positions where the patch fits (reference sampler.py:193-247)."""

    def _corners(self, subject: Subject) -> Iterator[Triple]:
        shape = subject.spatial_shape
        spans = [max(shape[d] - self.patch_size[d], 0) + 1 for d in range(3)]
        while True:  # one scalar torch.randint per axis, i then j then k: the reference's consumption of the generator
            yield tuple(int(torch.randint(0, span, (1,)).item()) for span in spans)  # type: ignore[misc]


class WeightedSampler(_RandomSampler):
    """Centres drawn from a probability-map image of the subject (reference sampler.py:250-310)."""

    def __init__(self, subject: Subject, patch_size, probability_map: str, num_patches: int | None = None) -> None:
        super().__init__(subject, patch_size, num_patches)
        self.probability_map = probability_map

    def _weights(self, subject: Subject) -> Tensor:
        return subject.images[self.probability_map].data[0].float()

    def _law(self, subject: Subject) -> CentreLaw:
        return CentreLaw(self._weights(subject), self.patch_size)

    def _build_probability_map(self) -> Tensor:
        return self._law(self.subject).map

    def _corners(self, subject: Subject) -> Iterator[Triple]:
        law = self._law(subject)
        flat = law.flat_cpu()
        if flat.sum() == 0:
            raise RuntimeError(f"Probability map '{self.probability_map}' is all zeros")
        shape = tuple(subject.spatial_shape)
        while True:
            yield corner_of(law.centre(int(torch.multinomial(flat, 1).item())), shape, self.patch_size)

    def _draw_source(self, subject: Subject) -> tuple[Tensor, list[tuple[float, float]] | None]:
        """What the device draw reads: the weight source ``(I, J, K)`` and, for labels, the table to look them up in."""
        from ..ops import _DTYPE_CODES  # noqa: PLC0415

        data = subject.images[self.probability_map].data
        return (data[0], None) if data.dtype in _DTYPE_CODES else (self._weights(subject), None)

    def _batch_corners(self, subject: Subject, num_patches: int) -> tuple[list[Triple], Tensor | None]:
        if get_centre_draw() != "device":
            return super()._batch_corners(subject, num_patches)
        from ..ops import engine  # noqa: PLC0415

        source, table = self._draw_source(subject)
        if source.device.type != "cuda":
            raise RuntimeError(
                f"set_centre_draw('device') draws on the GPU, but '{self.probability_map}' lives on {source.device}: move the subject"
                " there (`subject.to('cuda')`) or go back to set_centre_draw('reference')"
            )
        seed = int(torch.randint(0, 2**62, (1,)).item())  # the one consumption of the global CPU generator per call
        draw = engine().centre_draw(source, self.patch_size, num_patches, label_table=table, seed=seed)
        corners, total, invalid = draw.on_host()
        if invalid:
            raise RuntimeError("probability tensor contains either `inf`, `nan` or element < 0")
        if total == 0:
            raise RuntimeError(f"Probability map '{self.probability_map}' is all zeros")
        return [tuple(corner) for corner in corners.tolist()], draw.corners  # type: ignore[misc]


class LabelSampler(WeightedSampler):
    """Centres on labelled voxels, optionally weighted per label (reference sampler.py:313-366)."""

    def __init__(self, subject: Subject, patch_size, label_name: str, label_probabilities: dict | None = None,
                 num_patches: int | None = None) -> None:
        super().__init__(subject, patch_size, probability_map=label_name, num_patches=num_patches)
        self.label_name = label_name
        self.label_probabilities = label_probabilities

    def _weights(self, subject: Subject) -> Tensor:
        labels = subject.images[self.label_name].data[0]
        if self.label_probabilities is None:
            return (labels > 0).float()
        weights = torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
        for label, weight in self.label_probabilities.items():
            weights = torch.where(labels == label, torch.full((), float(weight), device=labels.device), weights)
        return weights

    def _draw_source(self, subject: Subject) -> tuple[Tensor, list[tuple[float, float]] | None]:
        from .. import _abi  # noqa: PLC0415
        from ..ops import _DTYPE_CODES  # noqa: PLC0415

        labels = subject.images[self.label_name].data[0]
        table = self.label_probabilities
        if table is None:
            return (labels, []) if labels.dtype in _DTYPE_CODES else (self._weights(subject), None)  # an empty table: label > 0
        if labels.dtype not in _DTYPE_CODES or not 0 < len(table) <= _abi.CENTRE_MAX_LABELS:
            return self._weights(subject), None  # the weight tensor of the reference road, handed over in map mode
        # `labels == label` compares in the labels' own type when that is a floating-point one: the key is rounded to it
        rounded = (lambda key: float(torch.tensor(float(key), dtype=labels.dtype))) if labels.dtype.is_floating_point else float
        return labels, [(rounded(label), float(weight)) for label, weight in table.items()]
