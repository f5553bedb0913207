"""CPU: ``Points``, ``BoundingBoxes`` and ``BoundingBoxFormat`` — the data model and how ``Subject``, ``Image`` and the batch
containers carry it.  The reference's own annotation tests run as well, unmodified, through the aliasing of
``scripts/run_reference_tests.py`` (skipped where the reference tree is absent)."""
from __future__ import annotations

import copy
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import annotation_cases as cases
import torchio_amd as tio
from torchio_amd.data.axes import axes_type
from torchio_amd.data.axes import get_axis_mapping
from torchio_amd.data.axes import validate_axes
from torchio_amd.data.bboxes import Representation
from torchio_amd.data.points import axes_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBLIQUE = tio.AffineMatrix(cases.IN_AFFINE)


def _points(n=6, seed=0, **kwargs):
    return tio.Points(torch.from_numpy(np.random.default_rng(seed).uniform(-5, 30, (n, 3)).astype(np.float32)), **kwargs)


# -- validation ------------------------------------------------------------------------------------------------------------
def test_validation_messages():
    with pytest.raises(ValueError, match=r"Points must have shape \(N, 3\), got \(4, 2\)"):
        tio.Points(torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"BoundingBoxes must have shape \(N, 6\), got \(2, 3\)"):
        tio.BoundingBoxes(torch.zeros(2, 3), format=tio.BoundingBoxFormat.IJKIJK)
    with pytest.raises(ValueError, match="Expected 2 labels, got 3"):
        tio.BoundingBoxes(torch.zeros(2, 6), format=tio.BoundingBoxFormat.IJKIJK, labels=torch.zeros(3))
    with pytest.raises(ValueError, match="Axis string must be 3 characters, got 2: 'RA'"):
        tio.Points(torch.zeros(1, 3), axes="RA")
    with pytest.raises(ValueError, match="Invalid axis string 'RLS'"):
        validate_axes("RLS")
    with pytest.raises(ValueError, match="Cannot compute axis mapping between different types: 'IJK' \\(voxel\\) and 'RAS' \\(anatomical\\)"):
        get_axis_mapping("IJK", "RAS")
    with pytest.raises(TypeError, match="Expected Points for key 'a', got Tensor"):
        tio.ScalarImage(torch.zeros(1, 2, 2, 2), points={"a": torch.zeros(1, 3)})
    with pytest.raises(TypeError, match="Expected BoundingBoxes for key 'b', got Points"):
        tio.ScalarImage(torch.zeros(1, 2, 2, 2), bounding_boxes={"b": _points()})
    with pytest.raises(ValueError):
        Representation("corner")
    assert validate_axes("KJI") == "KJI" and axes_type("IJK").value == "voxel" and axes_type("LPI").value == "anatomical"
    assert get_axis_mapping("RAS", "SPL") == ((2, 1, 0), (False, True, True))
    assert get_axis_mapping("IJK", "KIJ") == ((2, 0, 1), (False, False, False))
    assert tio.BoundingBoxFormat("IJK", "corners") == tio.BoundingBoxFormat.IJKIJK != tio.BoundingBoxFormat.IJKWHD
    assert repr(tio.BoundingBoxFormat("RAS", "center_size")) == "BoundingBoxFormat(axes='RAS', representation='center_size')"
    assert repr(_points(4, axes="LPS")) == "Points(num_points=4, axes='LPS')" and len(_points(4)) == 4


# -- conversions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [("KJI", "IJK"), ("LPS", "IJK"), ("SAR", "JKI", "LPI", "IJK"), ("RAS", "LPI", "IJK")])
def test_to_axes_round_trips_under_an_oblique_affine(route):
    points = _points(affine=OBLIQUE)
    moved = points
    for axes in route:
        moved = moved.to_axes(axes)
        assert moved.axes == axes and moved is not points
        # every convention names the same voxels: the float64 matrix of the convention, applied to the IJK coordinates
        expected = cases.apply34(axes_matrix(axes, OBLIQUE), points.data.numpy().astype(np.float64))
        assert np.abs(moved.data.numpy() - expected).max() <= 4 * np.spacing(np.float32(np.abs(expected).max())) * len(route)
    torch.testing.assert_close(moved.data, points.data, rtol=0, atol=2e-5)
    torch.testing.assert_close(points.to_world(), OBLIQUE.apply(points.data).float())
    world_axes = "".join(OBLIQUE.orientation)
    torch.testing.assert_close(points.to_axes(world_axes).data, points.to_world())


def test_to_format_round_trips():
    corners = torch.tensor([[1.0, 2.0, 3.0, 4.0, 6.0, 9.0], [0.0, -2.0, 5.0, 2.5, 3.0, 5.5]])
    boxes = tio.BoundingBoxes(corners, format=tio.BoundingBoxFormat.IJKIJK, labels=torch.tensor([3, 7]), affine=OBLIQUE, metadata={"k": 1})
    size = boxes.to_format(tio.BoundingBoxFormat.IJKWHD)
    torch.testing.assert_close(size.data, torch.tensor([[2.5, 4.0, 6.0, 3.0, 4.0, 6.0], [1.25, 0.5, 5.25, 2.5, 5.0, 0.5]]))
    torch.testing.assert_close(size.to_format(tio.BoundingBoxFormat.IJKIJK).data, corners)
    permuted = boxes.to_format(tio.BoundingBoxFormat("KIJ", "center_size"))
    torch.testing.assert_close(permuted.data[:, :3], size.data[:, [2, 0, 1]])
    torch.testing.assert_close(permuted.to_format(boxes.format).data, corners)
    assert torch.equal(permuted.labels, boxes.labels) and permuted.labels is not boxes.labels and permuted.metadata == {"k": 1}
    # through the affine the box becomes the hull of its two corners; an axis-aligned affine brings it back exactly
    aligned = tio.AffineMatrix(np.diag([-2.0, 0.5, 3.0, 1.0]) + np.array([[0, 0, 0, 4.0], [0, 0, 0, -1.0], [0, 0, 0, 2.0], [0, 0, 0, 0]]))
    axis_boxes = tio.BoundingBoxes(corners, format=tio.BoundingBoxFormat.IJKIJK, affine=aligned)
    world = axis_boxes.to_format(tio.BoundingBoxFormat("RAS"))
    assert bool((world.data[:, :3] <= world.data[:, 3:]).all())
    torch.testing.assert_close(world.to_format(tio.BoundingBoxFormat("LPS")).to_format(tio.BoundingBoxFormat.IJKIJK).data, corners)
    assert repr(world) == "BoundingBoxes(num_boxes=2, axes='RAS', representation='corners')" and len(world) == 2


def test_copies_are_independent():
    points = _points(affine=OBLIQUE, metadata={"names": ["a"]})
    boxes = tio.BoundingBoxes(torch.rand(3, 6), format=tio.BoundingBoxFormat.IJKWHD, labels=torch.arange(3), affine=OBLIQUE)
    for original in (points, boxes):
        clone = copy.deepcopy(original)
        assert torch.equal(clone.data, original.data) and clone.data.data_ptr() != original.data.data_ptr()
        assert clone.affine == original.affine and clone.affine is not original.affine
        clone.data.add_(1.0)
        clone.affine.data[0, 3] += 1.0
        assert not torch.equal(clone.data, original.data) and clone.affine != original.affine
    assert copy.deepcopy(boxes).labels is not boxes.labels
    like = points.new_like(data=torch.zeros(2, 3))
    assert like.axes == points.axes and like.metadata == points.metadata and like.affine == points.affine and like.affine is not points.affine
    assert boxes.new_like(data=torch.zeros(1, 6)).labels is None and boxes.new_like(data=torch.zeros(1, 6), affine=np.eye(4)).affine == tio.AffineMatrix()
    assert points.to(torch.float64) is points and points.data.dtype == torch.float64


# -- containers -------------------------------------------------------------------------------------------------------------
def _subject(n_points: int, seed: int):
    image = tio.ScalarImage(
        torch.zeros(1, 4, 5, 6), affine=OBLIQUE.clone(), points={"tips": _points(n_points + 1, seed + 1)},
        bounding_boxes={"cells": tio.BoundingBoxes(torch.rand(2, 6), format=tio.BoundingBoxFormat.IJKIJK)},
    )
    return tio.Subject(
        t1=image, seg=tio.LabelMap(torch.zeros(1, 4, 5, 6, dtype=torch.int16)), landmarks=_points(n_points, seed, axes="RAS"),
        lesions=tio.BoundingBoxes(torch.rand(1, 6), format=tio.BoundingBoxFormat.IJKWHD, labels=torch.tensor([seed])), age=seed,
    )


def test_subject_carries_annotations():
    subject = _subject(3, 0)
    assert set(subject.points) == {"landmarks"} and set(subject.bounding_boxes) == {"lesions"}
    assert subject.landmarks is subject["landmarks"] and "lesions" in subject and subject.age == 0
    assert set(subject.all_points()) == {"landmarks", ("t1", "tips")} and set(subject.all_bounding_boxes()) == {"lesions", ("t1", "cells")}
    assert list(subject) == ["t1", "seg", "landmarks", "lesions"] and len(subject) == 4
    clone = copy.deepcopy(subject)
    assert clone.landmarks is not subject.landmarks and torch.equal(clone.landmarks.data, subject.landmarks.data)
    assert clone.t1.points["tips"] is not subject.t1.points["tips"]
    assert subject.to(torch.float64) is subject and subject.landmarks.data.dtype == subject.t1.points["tips"].data.dtype == torch.float64
    assert tio.Subject(landmarks=_points()).points  # annotations alone make a subject


def test_image_keeps_annotations_through_new_like_deepcopy_and_slicing():
    image = _subject(2, 0).t1
    for other in (image.new_like(data=torch.ones(1, 2, 2, 2)), copy.deepcopy(image), image[:, 1:3]):
        assert type(other) is tio.ScalarImage and set(other.points) == {"tips"} and set(other.bounding_boxes) == {"cells"}
        assert other.points["tips"] is not image.points["tips"] and torch.equal(other.points["tips"].data, image.points["tips"].data)
    assert "points={tips}" in repr(image) and "bboxes={cells}" in repr(image)


def test_batches_carry_annotations_per_element_with_their_history():
    subjects = [_subject(n, seed) for seed, n in enumerate((0, 1, 5))]
    for index, subject in enumerate(subjects):
        subject.applied_transforms = [tio.AppliedTransform(name="Flip", params={"axes": (index % 3,)})]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    assert batch.has_annotations and [len(p["landmarks"]) for p in batch.points] == [0, 1, 5]  # lists, never stacked
    assert [len(p["tips"]) for p in batch.images["t1"].points] == [1, 2, 6] and batch.images["seg"].points is None
    batch.set_per_element_history([s.applied_transforms for s in subjects])
    clone = copy.deepcopy(batch)
    assert clone.points[2]["landmarks"] is not batch.points[2]["landmarks"]
    assert batch.to(torch.float64) is batch and batch.points[2]["landmarks"].data.dtype == torch.float64
    for index, (before, after) in enumerate(zip(subjects, clone.unbatch(), strict=True)):
        assert torch.equal(after.landmarks.data, before.landmarks.data) and after.landmarks.axes == "RAS"
        assert torch.equal(after.lesions.labels, before.lesions.labels) and after.lesions.format == tio.BoundingBoxFormat.IJKWHD
        assert torch.equal(after.t1.points["tips"].data, before.t1.points["tips"].data)
        assert set(after.t1.bounding_boxes) == {"cells"} and not after.seg.points and after.age == index
        assert [t.params for t in after.applied_transforms] == [{"axes": (index % 3,)}]
    images = tio.ImagesBatch.from_images([s.t1 for s in subjects])
    assert [len(image.points["tips"]) for image in images.unbatch()] == [1, 2, 6]
    plain = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(torch.zeros(1, 2, 2, 2)))])
    assert not plain.has_annotations and plain.points is None and plain.images["t1"].points is None


def test_engine_refuses_host_points_and_gradients():
    from torchio_amd import ops

    engine = ops.hip_engine()
    block = torch.from_numpy(cases.Map(np.eye(4)).block()[None])
    with pytest.raises(ops.EngineError, match="move the data"):
        engine.warp_points(torch.zeros(2, 3), [0, 2], block)
    if torch.cuda.is_available():
        with pytest.raises(ops.EngineError, match="no backward"):
            engine.warp_points(torch.zeros(2, 3, device="cuda", requires_grad=True), [0, 2], block)


# -- the reference's own tests -----------------------------------------------------------------------------------------------
def _runner():
    spec = importlib.util.spec_from_file_location("run_reference_tests", os.path.join(ROOT, "scripts", "run_reference_tests.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


REFERENCE_FILES = {
    # file -> (pytest -k selection or None, tests that pass)
    "test_points.py": (None, 33),
    "test_bboxes.py": (None, 48),
    "test_axes.py": (None, 32),
    "test_image_annotations.py": (None, 24),
    # the annotation tests of test_subject.py; its spatial slicing of a whole Subject is not part of this package
    "test_subject.py": ("WithPoints or WithBoundingBoxes or Mixed", 10),
}


@pytest.mark.reference
@pytest.mark.parametrize("name", list(REFERENCE_FILES))
def test_reference_annotation_tests_pass_on_the_mirror(name, tmp_path):
    runner = _runner()
    path = os.path.join(runner.REFERENCE_TESTS, name)
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    selection, expected = REFERENCE_FILES[name]
    code = (
        "import sys, pytest; sys.path.insert(0, sys.argv[1]); import run_reference_tests as r; r.install_alias();"
        "sys.exit(pytest.main(['-p', 'no:cacheprovider', '-q', '--rootdir=' + sys.argv[3], '-W', 'ignore', sys.argv[2], *sys.argv[4:]]))"
    )
    extra = [] if selection is None else ["-k", selection]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    result = subprocess.run(
        [sys.executable, "-c", code, os.path.join(ROOT, "scripts"), path, str(tmp_path), *extra],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120,
    )
    tail = result.stdout.strip().splitlines()[-1] if result.stdout.strip() else result.stderr[-400:]
    counts = {key: int(value) for value, key in re.findall(r"(\d+) (passed|failed|error|errors)", tail)}
    assert result.returncode == 0 and counts == {"passed": expected}, result.stdout[-2000:] + result.stderr[-1000:]
