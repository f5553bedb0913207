"""GPU: Points and BoundingBoxes through the public spatial transforms.

Every transform gets a ``Subject`` with one image of at most (12, 20, 16) voxels on an oblique grid (two for ``CopyAffine``),
5 subject-level points, 3 image-level points and a subject-level set of 2 boxes.  The expected coordinates come from the float64
reference of ``annotation_cases.py`` applied to the ``s`` the TEST derives — from the transform's recorded parameters and the
image's affine before and after, never from the code under test: for the transforms that only move the grid (``Flip``,
``Pad``, ``Crop``, ``Transpose``, ``Reorient`` and what is built from them) ``s`` is a matrix of small integers and the float32
result is exact.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import annotation_cases as cases
import torchio_amd as tio
from torchio_amd.data.points import axes_matrix

pytestmark = pytest.mark.gpu

SHAPE = (12, 20, 16)
AFFINE = cases.oblique_affine((0.8, 1.0, 2.5), (7.0, -11.0, 4.0), (-9.0, 5.0, 12.0))


def _coordinates(count: int, seed: int, shape=SHAPE) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.uniform(0.05, 0.95, (count, 3)) * (np.asarray(shape) - 1.0)).astype(np.float32))


def _boxes(count: int, seed: int, shape=SHAPE) -> torch.Tensor:
    """``(count, 6)`` centre-size boxes inside the grid, in quarter voxels: centre, size and the corners between them convert
    into each other without rounding, so that a grid move leaves nothing to round either."""
    rng = np.random.default_rng(seed)
    center = np.round(rng.uniform(0.3, 0.7, (count, 3)) * (np.asarray(shape) - 1.0) * 4) / 4
    size = np.round(rng.uniform(0.1, 0.3, (count, 3)) * np.asarray(shape) * 2) / 2
    return torch.from_numpy(np.concatenate([center, size], axis=1).astype(np.float32))


def _subject(seed: int = 0, points: int = 5, shape=SHAPE, axes: str = "IJK", extra_image: bool = False, device="cuda"):
    generator = torch.Generator().manual_seed(seed)
    affine = tio.AffineMatrix(AFFINE)
    landmarks = tio.Points(_coordinates(points, seed, shape), affine=affine.clone(), metadata={"kind": "landmarks"})
    if axes != "IJK":
        landmarks = landmarks.to_axes(axes)
    entries = {
        "t1": tio.ScalarImage(torch.rand((1, *shape), generator=generator), affine=affine.clone(),
                              points={"tips": tio.Points(_coordinates(3, seed + 100, shape), affine=affine.clone())}),
        "landmarks": landmarks,
        "lesions": tio.BoundingBoxes(_boxes(2, seed + 200, shape), format=tio.BoundingBoxFormat.IJKWHD, labels=torch.tensor([4, 9]),
                                     affine=affine.clone(), metadata={"kind": "lesions"}),
    }
    if extra_image:
        other = AFFINE.copy()
        other[:3, 3] += (0.5, -0.25, 0.75)
        entries["t2"] = tio.ScalarImage(torch.rand((1, *shape), generator=generator), affine=tio.AffineMatrix(other))
    return tio.Subject(**entries).to(device)


# -- the float64 expectation ------------------------------------------------------------------------------------------------
def _expected_points(points: tio.Points, m: cases.Map, in_affine, out_affine) -> np.ndarray:
    stored = points.data.cpu().numpy().astype(np.float64)
    ijk = cases.apply34(np.linalg.inv(axes_matrix(points.axes, in_affine)), stored)
    moved, status = cases.solve_ref(m, ijk)
    assert not status.any()
    return cases.apply34(axes_matrix(points.axes, out_affine), moved)


def _expected_boxes(boxes: tio.BoundingBoxes, m: cases.Map) -> np.ndarray:
    """Centre-size IJK boxes: the hull of the eight warped corners, as centre and size again."""
    data = boxes.data.cpu().numpy().astype(np.float64)
    low, high = data[:, :3] - data[:, 3:] / 2, data[:, :3] + data[:, 3:] / 2
    corners = np.stack([np.where([(c >> a) & 1 for a in range(3)], high, low) for c in range(8)], axis=1)  # (N, 8, 3)
    moved, status = cases.solve_ref(m, corners.reshape(-1, 3))
    assert not status.any()
    moved = moved.reshape(-1, 8, 3)
    low, high = moved.min(axis=1), moved.max(axis=1)
    return np.concatenate([(low + high) / 2, high - low], axis=1)


def _tolerance(values: np.ndarray, m: cases.Map, exact: bool, roundings: int = 1) -> float:
    if exact:
        return 0.0
    if m.field is None:  # one rounding of the float32 result, the matrix products of two implementations a few float64 ulps apart
        return roundings * float(np.spacing(np.float32(np.abs(values).max())))
    return cases.elastic_bar(m, values.astype(np.float32))


def _check(before: tio.Subject, after: tio.Subject, m: cases.Map, *, exact: bool = False, image: str = "t1") -> None:
    in_affine, out_affine = before[image].affine, after[image].affine
    for name, old, new in (("landmarks", before.landmarks, after.landmarks), ("tips", before[image].points["tips"], after[image].points["tips"])):
        expected = _expected_points(old, m, in_affine, out_affine)
        got = new.data.cpu().numpy()
        assert new.axes == old.axes and new.metadata == old.metadata and new.data.dtype == torch.float32 and new.data.device == old.data.device
        assert new.affine == out_affine and new.affine is not out_affine, name
        if exact:  # the float64 answer rounded once, bit for bit
            assert np.array_equal(got, expected.astype(np.float32)), name
        elif m.field is None:
            error = np.abs(got - expected).max()
            print(f"{name}: max |error| {error:.3g}")
            assert error <= _tolerance(expected, m, exact), name
        else:  # the bar of the kernel test: the residual of the float32 answer under s
            ijk = cases.apply34(np.linalg.inv(axes_matrix(new.axes, out_affine)), got.astype(np.float64))
            target = cases.apply34(np.linalg.inv(axes_matrix(old.axes, in_affine)), old.data.cpu().numpy().astype(np.float64))
            residual = np.abs(cases.s_ref(m, ijk)[0] - target).max()
            print(f"{name}: residual {residual:.3g}, bar {cases.elastic_bar(m, got):.3g}")
            assert residual <= cases.elastic_bar(m, got), name
    old, new = before.lesions, after.lesions
    expected = _expected_boxes(old, m)
    got = new.data.cpu().numpy()
    assert new.format == old.format and torch.equal(new.labels, old.labels) and new.metadata == old.metadata and new.affine == out_affine
    # centre and size are one more float32 operation away from the warped corners
    error = np.abs(got - expected).max()
    bound = 0.0 if exact else 3 * _tolerance(np.abs(expected[:, :3]) + expected[:, 3:], m, False) + (0.0 if m.field is None else 1e-5)
    print(f"lesions: max |error| {error:.3g}, bound {bound:.3g}")
    assert error <= bound


def _voxel_map(before: tio.Subject, after: tio.Subject, image: str = "t1") -> cases.Map:
    """``s`` of a transform that keeps world positions: ``inv(A_in) A_out``, whose entries are whole numbers (rounded: the
    float64 product is a few ulps off them)."""
    matrix = np.linalg.inv(before[image].affine.numpy()) @ after[image].affine.numpy()
    assert np.abs(matrix - np.round(matrix)).max() < 1e-9
    return cases.Map(np.round(matrix), after[image].spatial_shape)


def _returns(restored: tio.Subject, before: tio.Subject) -> None:
    """Forward and back are two float32 roundings at the size of the grid (``19 - x`` is not a float32 for every float32
    ``x``): within the bar of the affine-only pipelines, ``8 spacing(float32(extent))``; the quarter-voxel boxes exactly."""
    bar = 8 * float(np.spacing(np.float32(max(SHAPE))))
    torch.testing.assert_close(restored.landmarks.data, before.landmarks.data, rtol=0, atol=bar)
    torch.testing.assert_close(restored.t1.points["tips"].data, before.t1.points["tips"].data, rtol=0, atol=bar)
    assert torch.equal(restored.lesions.data, before.lesions.data) and restored.landmarks.affine == restored.t1.affine


# -- the Spatial family -----------------------------------------------------------------------------------------------------
SPATIAL = {
    "Affine": lambda: tio.Affine(degrees=(-15, 15), scales=(0.85, 1.2), translation=(-2, 2)),
    "ElasticDeformation": lambda: tio.ElasticDeformation(max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6)),
    "Spatial": lambda: tio.Spatial(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-2, 2), max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6)),
    "Spatial_elastic_first": lambda: tio.Spatial(degrees=(-10, 10), max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6), affine_first=False),
    "Spatial_target": lambda: tio.Spatial(target=(1.2, 0.9, 2.0), degrees=(-10, 10), max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6)),
    "Resample": lambda: tio.Resample(target=(1.2, 0.9, 2.0)),
}


@pytest.mark.parametrize("name", list(SPATIAL))
def test_spatial_family(hip, name):
    before = _subject(seed=3)
    torch.manual_seed(17)
    after = SPATIAL[name]()(before)
    params = after.applied_transforms[-1].params
    (m,) = cases.spatial_maps(params, before.t1.affine, after.t1.spatial_shape, after.t1.affine, 1)
    assert (m.field is not None) == (name not in ("Affine", "Resample"))
    _check(before, after, m)
    # the inverse in the history moves the annotations by the same rule with its own s
    restored = after.apply_inverse_transform()
    moved = float((after.landmarks.data - before.landmarks.data).abs().max())
    back = float((restored.landmarks.data - before.landmarks.data).abs().max())
    print(f"{name}: moved {moved:.3g}, back within {back:.3g}")
    assert restored.landmarks.affine == before.t1.affine
    if m.field is None:
        assert back <= 8 * float(np.spacing(np.float32(max(SHAPE))))
    else:
        assert back < moved  # the negated field is the reference's approximate inverse


def test_resize(hip):
    before = _subject(seed=4)
    target = (9, 25, 16)
    after = tio.Resize(target)(before)
    scale = [(a - 1) / (b - 1) for a, b in zip(SHAPE, target, strict=True)]  # trilinear, align_corners=True
    _check(before, after, cases.Map(np.diag([*scale, 1.0]), target))


# -- grid moves: exact ------------------------------------------------------------------------------------------------------
def _flip_map(axes) -> cases.Map:
    matrix = np.eye(4)
    for axis in axes:
        matrix[axis, axis], matrix[axis, 3] = -1.0, SHAPE[axis] - 1.0
    return cases.Map(matrix, SHAPE)


def test_flip(hip):
    before = _subject(seed=5)
    after = tio.Flip(axes=(0, 2))(before)
    assert tuple(after.applied_transforms[-1].params["axes"]) == (0, 2)
    _check(before, after, _flip_map((0, 2)), exact=True)
    _returns(after.apply_inverse_transform(), before)


GRID_MOVES = {
    "Pad": lambda: tio.Pad(padding=(1, 2, 0, 3, 4, 0)),
    "Crop": lambda: tio.Crop(cropping=(2, 1, 3, 0, 0, 5)),
    "CropOrPad": lambda: tio.CropOrPad((16, 13, 16)),
    "EnsureShapeMultiple": lambda: tio.EnsureShapeMultiple(8),
    "Transpose": lambda: tio.Transpose(),
    "Reorient": lambda: tio.Reorient("PIR"),
}


@pytest.mark.parametrize("batched", [False, True], ids=["subject", "batch"])
@pytest.mark.parametrize("name", list(GRID_MOVES))
def test_grid_moves_are_exact(hip, name, batched):
    before = _subject(seed=6)
    data = tio.SubjectsBatch.from_subjects([before]) if batched else before
    out = GRID_MOVES[name]()(data)
    after = out.unbatch()[0] if batched else out
    assert after.t1.spatial_shape != SHAPE or name == "Reorient" or name == "Transpose"
    _check(before, after, _voxel_map(before, after), exact=True)
    if batched and name in ("CropOrPad", "EnsureShapeMultiple"):
        return  # (on a batch these two record one entry that has no inverse, as in the reference)
    restored = (out.apply_inverse_transform().unbatch()[0] if batched else after.apply_inverse_transform())
    assert restored.t1.spatial_shape == SHAPE
    _returns(restored, before)


def test_affine_only_changes_keep_the_voxels(hip):
    reference = tio.ScalarImage(torch.zeros(1, 6, 10, 8), affine=tio.AffineMatrix(cases.OUT_AFFINE))
    for axes in ("IJK", "LPS"):
        before = _subject(seed=7, axes=axes, extra_image=True)
        for transform, image in ((tio.ToReferenceSpace(reference), "t1"), (tio.CopyAffine("t2"), "t1")):
            after = transform(before)
            assert after[image].affine != before[image].affine
            _check(before, after, cases.Map(np.eye(4), SHAPE), exact=axes == "IJK", image=image)
            if axes == "IJK":  # voxel coordinates keep their values, the affine is the image's new one
                assert torch.equal(after.landmarks.data, before.landmarks.data)


def test_anisotropy_and_intensity_transforms_leave_annotations_alone(hip):
    before = _subject(seed=8)
    torch.manual_seed(1)
    after = tio.Compose([tio.Anisotropy(downsampling=2.0), tio.Noise(), tio.Gamma()])(before)
    assert torch.equal(after.landmarks.data, before.landmarks.data) and torch.equal(after.lesions.data, before.lesions.data)
    assert torch.equal(after.t1.points["tips"].data, before.t1.points["tips"].data) and after.landmarks.affine == before.landmarks.affine


def test_anatomical_points_go_through_the_affines(hip):
    before = _subject(seed=9, axes="LPS")
    torch.manual_seed(5)
    after = tio.Affine(degrees=(-15, 15), translation=(-2, 2))(before)
    (m,) = cases.spatial_maps(after.applied_transforms[-1].params, before.t1.affine, SHAPE, after.t1.affine, 1)
    expected = _expected_points(before.landmarks, m, before.t1.affine, after.t1.affine)
    assert after.landmarks.axes == "LPS"
    assert np.abs(after.landmarks.data.cpu().numpy() - expected).max() <= 2 * np.spacing(np.float32(np.abs(expected).max()))
    torch.manual_seed(5)
    elastic = tio.ElasticDeformation(max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6))(before)
    (m,) = cases.spatial_maps(elastic.applied_transforms[-1].params, before.t1.affine, SHAPE, elastic.t1.affine, 1)
    expected = _expected_points(before.landmarks, m, before.t1.affine, elastic.t1.affine)
    # two more float32 roundings in world millimetres, in front of and behind the solve
    bound = cases.elastic_bar(m, elastic.landmarks.data.cpu().numpy()) + 4 * np.spacing(np.float32(np.abs(expected).max())) * cases.jacobian_bound(m)
    assert np.abs(elastic.landmarks.data.cpu().numpy() - expected).max() <= bound


# -- a batched pipeline and its inverse -------------------------------------------------------------------------------------
def _pipeline(elastic: bool):
    steps = [tio.Affine(degrees=(-12, 12), scales=(0.9, 1.1), translation=(-1.5, 1.5))]
    if elastic:
        steps.append(tio.ElasticDeformation(max_displacement=(0.4, 0.8), num_control_points=(5, 7, 6)))
    steps += [tio.Flip(axes=(0, 1, 2), flip_probability=0.5), tio.CropOrPad((14, 16, 16))]
    return tio.Compose(steps)


@pytest.mark.parametrize("elastic", [False, True], ids=["affine_only", "with_elastic"])
def test_batched_pipeline_and_its_inverse(hip, elastic):
    subjects = [_subject(seed=20 + index, points=count) for index, count in enumerate((5, 1, 9))]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    torch.manual_seed(31)
    out = _pipeline(elastic)(batch)
    assert [len(p["landmarks"]) for p in out.points] == [5, 1, 9]
    restored = out.apply_inverse_transform()
    for before, after, back in zip(subjects, out.unbatch(), restored.unbatch(), strict=True):
        assert after.t1.spatial_shape == (14, 16, 16) and back.t1.spatial_shape == SHAPE
        assert after.landmarks.affine == after.t1.affine and back.landmarks.affine == before.t1.affine
        for old, new, end in ((before.landmarks, after.landmarks, back.landmarks), (before.t1.points["tips"], after.t1.points["tips"], back.t1.points["tips"])):
            moved = float((new.data - old.data).abs().max())
            error = float((end.data - old.data).abs().max())
            print(f"moved {moved:.3g}, back within {error:.3g}")
            if elastic:
                assert error < moved
            else:
                assert error <= 8 * float(np.spacing(np.float32(max(SHAPE))))


# -- image and points stay together -----------------------------------------------------------------------------------------
BLOB_SHAPE = (32, 40, 36)
LANDMARKS = np.array([[10.0, 12.0, 11.0], [20.0, 27.0, 14.0], [13.0, 25.0, 24.0], [21.0, 14.0, 23.0]])


def blob_subject(device="cuda"):
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in BLOB_SHAPE], indexing="ij"), axis=-1)
    image = sum(np.exp(-((grid - center) ** 2).sum(axis=-1) / (2 * 2.0**2)) for center in LANDMARKS)
    affine = tio.AffineMatrix(cases.oblique_affine((1.0, 0.9, 1.1), (3.0, -4.0, 5.0), (-15.0, -18.0, -20.0)))
    return tio.Subject(
        t1=tio.ScalarImage(torch.from_numpy(image[None].astype(np.float32)), affine=affine),
        landmarks=tio.Points(torch.from_numpy(LANDMARKS.astype(np.float32)), affine=affine.clone()),
    ).to(device)


def blob_transform():
    # rotation, scale and a field of regime (a): at most 1/8 of a coarse cell ((S - 1) / (n - 1) >= 6.2 voxels of >= 0.9 mm)
    return tio.Spatial(degrees=(8, -6, 10), scales=(1.1, 0.92, 1.05), max_displacement=0.69, num_control_points=(6, 7, 6), default_pad_value=0.0)


def blob_centroids(image: np.ndarray, around: np.ndarray, radius: float = 7.0) -> np.ndarray:
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in image.shape], indexing="ij"), axis=-1)
    centroids = []
    for center in around:
        weight = np.where(((grid - center) ** 2).sum(axis=-1) <= radius**2, image, 0.0)
        centroids.append((grid * weight[..., None]).sum(axis=(0, 1, 2)) / weight.sum())
    return np.stack(centroids)


def test_image_and_points_stay_together(hip):
    """A cap against gross errors (sign, axis order, inverse direction miss by many voxels), not a precision bar: with these
    parameters the float64 reference itself keeps every centroid within 0.2 voxel of its landmark (checked on the CPU oracle
    while this test was written)."""
    before = blob_subject()
    torch.manual_seed(3)
    after = blob_transform()(before)
    warped = after.landmarks.data.cpu().numpy().astype(np.float64)
    assert np.abs(warped - LANDMARKS).max() > 1.5  # the landmarks really moved
    centroids = blob_centroids(after.t1.data[0].cpu().numpy().astype(np.float64), warped)
    distance = np.sqrt(((centroids - warped) ** 2).sum(axis=1))
    print("centroid to landmark:", distance)
    assert distance.max() <= 0.5


# -- no annotations, no work ------------------------------------------------------------------------------------------------
def test_a_batch_without_annotations_takes_none_of_the_new_paths(hip, monkeypatch):
    from torchio_amd.transforms import _annotations

    def plain_batch():
        subjects = [tio.Subject(t1=_subject(seed=40 + index).t1.new_like(data=_subject(seed=40 + index).t1.data)) for index in range(3)]
        for subject in subjects:
            subject.t1.points.clear()
        return tio.SubjectsBatch.from_subjects(subjects)

    calls = []
    real = hip.warp_points
    monkeypatch.setattr(hip, "warp_points", lambda *args, **kwargs: calls.append(1) or real(*args, **kwargs))
    torch.manual_seed(8)
    out = _pipeline(True)(plain_batch())
    assert not calls and not out.has_annotations
    # the same call with the annotation code switched off altogether: the same bits
    with monkeypatch.context() as patch:
        patch.setattr(_annotations, "track", lambda batch, images: None)
        patch.setattr(tio.SubjectsBatch, "has_annotations", property(lambda self: False))
        torch.manual_seed(8)
        off = _pipeline(True)(plain_batch())
    assert torch.equal(out.images["t1"].data.view(torch.int32), off.images["t1"].data.view(torch.int32))
    assert [a.data.tolist() for a in out.images["t1"].affines] == [a.data.tolist() for a in off.images["t1"].affines]
    assert [t.name for t in out.applied_transforms] == [t.name for t in off.applied_transforms]
    # and annotations change nothing about the images
    annotated = tio.SubjectsBatch.from_subjects([_subject(seed=40 + index) for index in range(3)])
    torch.manual_seed(8)
    with_points = _pipeline(True)(annotated)
    assert calls and torch.equal(with_points.images["t1"].data.view(torch.int32), out.images["t1"].data.view(torch.int32))
    assert copy.deepcopy(with_points).points[0]["landmarks"].data.is_cuda
