"""Shared by the patch-feed tests: an independent float64 numpy statement of the weighted centre draw, and the comparison
of two batches.

Nothing here mirrors the kernel's structure (segments, prefix search, per-segment scan): the law is the masked weight vector,
a draw is ``searchsorted(cumsum(w), u * total, side="right")``, the uniform stream is Philox4x32-10 written with numpy
integers.  A plain module: no test in it.
"""
from __future__ import annotations

import numpy as np
import torch

SEGMENT = 2048  # TIO_CENTRE_SEGMENT: only used to AIM uniforms at segment boundaries, never to compute a reference

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter: np.ndarray, key: tuple[int, int]) -> np.ndarray:
    """Random123's Philox4x32-10 on an ``(N, 4)`` uint32 counter array."""
    c = [counter[:, d].astype(np.uint64) for d in range(4)]
    k0, k1 = key
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def centre_uniforms(seed: int, n: int) -> np.ndarray:
    """The package's centre stream: counter ``{n lo, n hi, 2, 0}``, key ``{seed lo, seed hi}``, 53 bits of ``c[0]``, ``c[1]``."""
    index = np.arange(n, dtype=np.uint64)
    counter = np.stack([index & _LOW, index >> np.uint64(32), np.full(n, 2, np.uint64), np.zeros(n, np.uint64)], axis=1).astype(np.uint32)
    c = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    bits = (c[:, 0] >> np.uint64(5)) * np.uint64(1 << 26) + (c[:, 1] >> np.uint64(6))
    return bits.astype(np.float64) * 2.0**-53


def label_weights(labels: np.ndarray, table) -> np.ndarray:
    """float32 weights of a label array: ``label > 0`` without a table, else the pairs in order, later ones overriding."""
    if not table:
        return (labels > 0).astype(np.float32)
    weights = np.zeros(labels.shape, np.float32)
    for value, weight in table:
        weights[labels == value] = np.float32(weight)
    return weights


def masked_weights(weights: np.ndarray, patch) -> np.ndarray:
    """float64 flat vector: *weights* (already float32) where ``half <= pos < shape - half`` on every axis, else 0."""
    allowed = np.ones(weights.shape, bool)
    for axis in range(3):
        half = patch[axis] // 2
        if half > 0:
            position = np.arange(weights.shape[axis])
            inside = (position >= half) & (position < weights.shape[axis] - half)
            allowed &= inside.reshape([-1 if a == axis else 1 for a in range(3)])
    return np.where(allowed, weights.astype(np.float32), np.float32(0)).astype(np.float64).reshape(-1)


def draw_reference(flat: np.ndarray, uniforms: np.ndarray) -> tuple[np.ndarray, np.ndarray, float]:
    """``(indices, cdf, total)``: for every uniform the first voxel whose inclusive cumulative weight exceeds ``u * total``."""
    cdf = np.cumsum(flat)
    total = float(cdf[-1])
    return np.searchsorted(cdf, uniforms * total, side="right"), cdf, total


def corners_reference(indices: np.ndarray, shape, patch) -> np.ndarray:
    centre = np.stack(np.unravel_index(indices, shape), axis=1)
    half = np.array([p // 2 for p in patch])
    return np.minimum(np.maximum(centre - half, 0), np.array(shape) - np.array(patch)).astype(np.int32)


def boundary_uniforms(flat: np.ndarray) -> np.ndarray:
    """Uniforms that put ``t`` exactly on the cumulative weight at every segment boundary (integer weights: ``c / total * total``
    is checked to round back to ``c``), plus 0 and the largest float64 below 1."""
    cdf = np.cumsum(flat)
    total = cdf[-1]
    ends = cdf[SEGMENT - 1 :: SEGMENT]
    candidates = ends[ends < total] / total
    exact = candidates[candidates * total == ends[ends < total]]
    return np.concatenate([[0.0, 1.0 - 2.0**-53], exact, np.linspace(0.0, 1.0, 37, endpoint=False)])


SUBJECT_SHAPE = (12, 10, 9)


def make_subject(seed: int = 0, device: str = "cpu"):
    """A float32 image with two channels and a point set, an int16 label map (0 .. 3), an integer-valued probability map,
    two metadata entries; an oblique affine, so a moved origin shows in every column."""
    import torchio_amd as tio

    rng = np.random.default_rng(seed)
    affine = np.array([[0.0, -2.0, 0.0, 5.0], [1.5, 0.0, 0.0, -3.0], [0.0, 0.0, 3.0, 7.0], [0.0, 0.0, 0.0, 1.0]])
    points = tio.Points(torch.from_numpy(rng.uniform(0, 8, (5, 3)).astype(np.float32)))
    image = tio.ScalarImage(torch.from_numpy(rng.standard_normal((2, *SUBJECT_SHAPE)).astype(np.float32)), affine=affine, points={"tips": points})
    labels = tio.LabelMap(torch.from_numpy(rng.integers(0, 4, (1, *SUBJECT_SHAPE)).astype(np.int16)), affine=affine)
    prob = tio.ScalarImage(torch.from_numpy(rng.integers(0, 4, (1, *SUBJECT_SHAPE)).astype(np.float32)), affine=affine)
    subject = tio.Subject(t1=image, seg=labels, prob=prob, name=f"case{seed}", age=40 + seed)
    return subject.to(device) if device != "cpu" else subject


def samplers(subject) -> dict:
    import torchio_amd as tio

    return {
        "uniform": tio.UniformSampler(subject, (4, 3, 2)),
        "weighted": tio.WeightedSampler(subject, (4, 3, 1), probability_map="prob"),
        "label": tio.LabelSampler(subject, (5, 4, 3), label_name="seg", label_probabilities={1: 1.0, 2: 3.0}),
    }


def assert_same_batch(ours, expected) -> None:
    """Tensors bit for bit, affines, annotations, ``patch_location`` and the other metadata, history."""
    assert list(ours.images) == list(expected.images)
    for name, batch in expected.images.items():
        mine = ours.images[name]
        assert type(mine) is type(batch) and mine._image_class is batch._image_class
        assert mine.data.dtype == batch.data.dtype and mine.data.device == batch.data.device and mine.data.shape == batch.data.shape
        assert mine.data.is_contiguous()
        assert torch.equal(mine.data.view(torch.uint8), batch.data.contiguous().view(torch.uint8)), name
        assert len(mine.affines) == len(batch.affines)
        for a, b in zip(mine.affines, batch.affines, strict=True):
            assert torch.equal(a.data, b.data)
        for store in ("points", "bounding_boxes"):
            assert _annotation_values(getattr(mine, store)) == _annotation_values(getattr(batch, store))
    assert ours.metadata == expected.metadata
    assert "patch_location" in ours.metadata
    for store in ("points", "bounding_boxes"):
        assert _annotation_values(getattr(ours, store)) == _annotation_values(getattr(expected, store))
    assert ours.applied_transforms == expected.applied_transforms
    assert ours._per_element_history == expected._per_element_history


def _annotation_values(store):
    if store is None:
        return None
    return [{name: (type(value).__name__, value.data.cpu().tolist(), str(getattr(value, "axes", ""))) for name, value in element.items()} for element in store]
