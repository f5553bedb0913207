"""CPU: the float64 numpy reference of the annotation tests (``annotation_cases.py``) on its own, before the GPU tests lean on it.

* ``s_ref`` against the sampling coordinates of committed golden ``Spatial`` vectors.  The fixtures hold images, not grids, so
  the coordinates are recovered: the golden case's transform, seeded as the case is (the drawn parameters are asserted to be
  the recorded ones), resamples three coordinate ramps on the CPU oracle — which the same fixtures pin bit for bit
  (``test_golden_oracle.py``).  Trilinear interpolation reproduces a ramp, so wherever the sample lies inside the field of
  view the output voxel ``o`` of ramp ``c`` holds ``s(o)_c``.
* with a zero field ``s_ref`` is ``M`` alone, whichever way the field is composed;
* ``s_ref(solve_ref(p)) = p`` to 1e-9, with every point reported converged, in both regimes and both compositions.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import annotation_cases as cases
import torchio_amd as tio
from golden_cases import build_transform
from golden_cases import load_cases
from parity_harness import use_engine

GOLDEN = {case["name"]: case for case in load_cases()}
RECOVERABLE = ["affine", "elastic", "spatial_fused", "spatial_elastic_first_batch_p", "spatial_target_and_affine", "resample_2mm"]
SEEDS = {"gentle": 11, "half_folding": 11}  # regime (b): checked below — the float64 reference converges on every point


def _ramps(shape) -> torch.Tensor:
    axes = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in shape], indexing="ij")
    return torch.stack(axes)


@pytest.mark.parametrize("name", RECOVERABLE)
def test_s_ref_is_the_sampling_grid_of_the_golden_vectors(name, oracle):
    case = GOLDEN[name]
    subjects = [
        tio.Subject(
            t1=tio.ScalarImage(_ramps(item["t1"].shape[1:]), affine=tio.AffineMatrix(item["affine"])),
            seg=tio.LabelMap(item["seg"].clone(), affine=tio.AffineMatrix(item.get("seg_affine", item["affine"]))),
        )
        for item in case["inputs"]
    ]
    data = subjects[0] if len(subjects) == 1 else tio.SubjectsBatch.from_subjects(subjects)
    torch.manual_seed(case["seed"])
    with use_engine(oracle):
        out = build_transform(case)(data)
    history = [{"name": t.name, "params": t.params} for t in out.applied_transforms]
    assert history == case["expected"]["history"]  # the golden vector's own parameters
    outs = [out] if isinstance(out, tio.Subject) else out.unbatch()
    params = history[-1]["params"] if history else None
    checked = 0
    for index, (before, after) in enumerate(zip(subjects, outs, strict=True)):
        if params is None:
            continue
        in_shape, out_shape = before.t1.spatial_shape, after.t1.spatial_shape
        first = subjects[0].t1  # the launch reads the first element's grid (spatial.py:1110-1135)
        m = cases.spatial_maps(params, first.affine, out_shape, after.t1.affine, len(subjects))[index]
        if m is None:
            assert torch.equal(after.t1.data, before.t1.data)
            continue
        o = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_shape], indexing="ij"), axis=-1).reshape(-1, 3)
        s, _ = cases.s_ref(m, o)
        inside = np.all((s >= 0.01) & (s <= np.asarray(in_shape) - 1.01), axis=1)
        assert inside.sum() > 0.2 * inside.size
        sampled = after.t1.data.numpy().reshape(3, -1).T.astype(np.float64)
        # float32 mapping, float32 interpolation weights: a few units of the coordinate's last place, not more
        assert np.abs(sampled[inside] - s[inside]).max() <= 2e-4
        checked += 1
    assert checked > 0


@pytest.mark.parametrize("affine_first", [True, False])
def test_zero_field_is_the_matrix_alone(affine_first):
    m = cases.Map(cases.voxel_matrix(3), cases.OUT_SHAPE, cases.IN_SPACING, cases.OUT_SPACING, affine_first, np.zeros((*cases.GRID, 3), np.float32))
    plain = cases.Map(cases.voxel_matrix(3))
    rng = np.random.default_rng(0)
    o = rng.uniform(-20, 40, (500, 3))
    s, jacobian = cases.s_ref(m, o)
    expected, _ = cases.s_ref(plain, o)
    assert np.array_equal(s, expected) if affine_first else np.abs(s - expected).max() <= 1e-12
    assert np.abs(jacobian - m.matrix[:3, :3]).max() <= 1e-15
    solved, status = cases.solve_ref(m, expected)
    assert not status.any() and np.abs(solved - o).max() <= 1e-9


def test_jacobian_is_the_derivative_and_within_its_bound():
    m = cases.elastic_map("half_folding", True, SEEDS["half_folding"])
    rng = np.random.default_rng(1)
    o = rng.uniform(0.3, 0.7, (200, 3)) * (np.asarray(cases.OUT_SHAPE) - 1.0)
    _, jacobian = cases.s_ref(m, o)
    h = 1e-6
    for axis in range(3):
        step = np.zeros(3)
        step[axis] = h
        numeric = (cases.s_ref(m, o + step)[0] - cases.s_ref(m, o - step)[0]) / (2 * h)
        smooth = np.abs(numeric - jacobian[:, :, axis]).max(axis=1) < 1e-5  # (a step across a cell face is not a derivative)
        assert smooth.mean() > 0.95
    assert np.abs(jacobian).sum(axis=2).max() <= cases.jacobian_bound(m) * (1 + 1e-12)


@pytest.mark.parametrize("affine_first", [True, False])
@pytest.mark.parametrize("regime", ["gentle", "half_folding"])
def test_solve_ref_inverts_s_ref(regime, affine_first):
    m = cases.elastic_map(regime, affine_first, SEEDS[regime])
    p = cases.points_for(m, 2000, seed=5).astype(np.float64)
    o, status = cases.solve_ref(m, p)
    assert not status.any(), f"{int(status.sum())} of {status.size} points did not converge"
    assert np.abs(cases.s_ref(m, o)[0] - p).max() <= 1e-9


def test_points_outside_the_field_of_view_stay_defined():
    m = cases.elastic_map("gentle", True, SEEDS["gentle"])
    far = np.array([[-500.0, 0.0, 0.0], [0.0, 900.0, 0.0], [3.0, 4.0, -700.0], [1e4, -1e4, 1e4]])
    o, status = cases.solve_ref(m, far)
    assert not status.any() and np.isfinite(o).all()
    assert np.abs(cases.s_ref(m, o)[0] - far).max() <= cases.TOLERANCE
