"""Inputs and torch-CPU restatements shared by the label-transform tests (a plain module, no tests in it).

Label fields: ``torch.rand`` box-filtered twice and cut at its 0.4 / 0.6 / 0.8 quantiles into the values 0..3 — blobs of a
few to a few thousand voxels, several components per value.  The restatements follow the reference's operation sequences
(``transforms/label/*.py``) on the CPU; for ``KeepLargestComponent``, whose reference needs SimpleITK, the components come
from a minimum-index propagation run to its fixpoint (the same partition as ``scipy.ndimage.label`` with the full /
cross structuring element; ``tests/test_label_transforms_host.py`` compares them where scipy is present).
"""
from __future__ import annotations

import functools
import itertools

import torch
import torch.nn.functional as F


@functools.lru_cache(maxsize=None)
def label_field(shape: tuple, seed: int) -> torch.Tensor:
    """``(B, 1, I, J, K)`` int64 field of the values 0..3 (do not modify: cached)."""
    generator = torch.Generator().manual_seed(seed)
    noise = torch.rand(shape, generator=generator)
    for _ in range(2):
        noise = F.avg_pool3d(F.pad(noise, [1] * 6, mode="replicate"), 3, stride=1)
    cuts = torch.quantile(noise.reshape(-1), torch.tensor([0.4, 0.6, 0.8]))
    return (noise[..., None] > cuts).sum(-1)


def remap(data: torch.Tensor, mapping: dict, default=None) -> torch.Tensor:
    """remap_labels.py:54-57 / sequential_labels.py:58-61: one masked write per pair, compared with the original."""
    out = data.clone() if default is None else torch.full_like(data, default)
    for old, new in mapping.items():
        out[data == old] = new
    return out


def one_hot(data: torch.Tensor, num_classes: int = -1) -> torch.Tensor:
    """one_hot.py:64-68."""
    return F.one_hot(data.long()[:, 0], num_classes=num_classes).permute(0, 4, 1, 2, 3).float()


def contour(data: torch.Tensor) -> torch.Tensor:
    """contour.py:66-70."""
    padded = F.pad(data.float(), [1] * 6, mode="constant", value=-1)
    eroded = -F.max_pool3d(-padded, kernel_size=3, stride=1, padding=0)
    return (eroded != data.float()).float()


def _offsets(fully_connected: bool):
    for offset in itertools.product((-1, 0, 1), repeat=3):
        if offset != (0, 0, 0) and (fully_connected or sum(abs(o) for o in offset) == 1):
            yield offset


def components(volume: torch.Tensor, fully_connected: bool) -> torch.Tensor:
    """For an ``(I, J, K)`` volume: per voxel the smallest flat (C-order) index of its connected component of EQUAL-valued
    voxels.  Every voxel starts with its own index; a sweep takes the minimum over the equal-valued neighbours, pointer
    jumping (``label[label]``: the label is a voxel of the same component) shortens the chains; repeated to the fixpoint."""
    label = torch.arange(volume.numel()).view(volume.shape)
    shape = volume.shape

    def window(offset, sign):
        return tuple(slice(max(0, sign * o), shape[d] + min(0, sign * o)) for d, o in enumerate(offset))

    while True:
        new = label.clone()
        for offset in _offsets(fully_connected):
            here, there = window(offset, -1), window(offset, 1)  # voxel `here`, its neighbour `there` = here + offset
            same = volume[here] == volume[there]
            new[here] = torch.where(same, torch.minimum(new[here], new[there]), new[here])
        flat = new.view(-1)
        for _ in range(4):
            flat = flat[flat]
        new = flat.view(shape)
        if torch.equal(new, label):
            return label
        label = new


def component_sizes(volume: torch.Tensor, value, fully_connected: bool, label: torch.Tensor | None = None) -> list[tuple[int, int]]:
    """``(size, first voxel)`` of every component of ``value``, largest first, ties by the first voxel."""
    label = components(volume, fully_connected) if label is None else label
    roots, counts = torch.unique(label[volume == value], return_counts=True)
    return sorted(((int(c), int(r)) for r, c in zip(roots, counts, strict=True)), key=lambda sr: (-sr[0], sr[1]))


def keep_largest(data: torch.Tensor, labels, background=0, fully_connected: bool = True) -> torch.Tensor:
    """keep_largest.py:108-125 with the components above; of equally large components the first in C order stays."""
    out = data.clone()
    for b in range(data.shape[0]):
        volume = data[b, 0]
        label = components(volume, fully_connected)
        for value in labels:
            sizes = component_sizes(volume, value, fully_connected, label)
            if sizes:
                out[b, 0][(volume == value) & (label != sizes[0][1])] = background
    return out


def has_tie(data: torch.Tensor, labels, fully_connected: bool) -> bool:
    for b in range(data.shape[0]):
        label = components(data[b, 0], fully_connected)
        for value in labels:
            sizes = component_sizes(data[b, 0], value, fully_connected, label)
            if len(sizes) > 1 and sizes[0][0] == sizes[1][0]:
                return True
    return False
