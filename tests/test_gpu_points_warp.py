"""GPU: ``tio_points_warp`` (``Engine.warp_points``) against the float64 numpy reference of ``annotation_cases.py``.

Shapes: a non-cubic output grid (11, 24, 17) over an input of (13, 19, 23), a (5, 7, 6) control grid, spacings (0.8, 1.0, 2.5)
in and (1.2, 0.9, 2.0) out, oblique affines on both sides, both compositions of affine and field; a batch of three elements
with 0, 1 and 257 points (an empty element, a block boundary), every third point outside the field of view.

Bars.  Affine only: at most one float32 ulp from ``float32(Minv64 @ p64)``, the product written out term by term so that no
BLAS picks the order of the sum; the kernel adds in that order with every operation rounded on its own, so the float64 values
are the same and equality is asserted as well.  With a field: ``max|s_ref(o_gpu) - p| <= 1e-6 + 4 spacing(float32(max|coord|)) Jn``, ``Jn``
the bound on the Jacobian's infinity norm from ``M`` and the control field's finite differences
(``annotation_cases.jacobian_bound``): the rounding of the float32 output carried through ``s``, times four, over the
solver's stop.  Two regimes: (a) at most 1/8 of a coarse cell per axis — ``I + grad d`` strictly diagonally dominant, the map
injective, every status 0; (b) half the reference's folding bound, control fields of seeds 11 and 15, on which the float64
reference converges for every point (asserted here as well) — status 0 and the bar.  Nothing at or beyond folding.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import annotation_cases as cases

pytestmark = pytest.mark.gpu

#: control-field seeds per batch element; regime (b) needs fields on which the float64 reference converges everywhere
FIELD_SEEDS = (15, 15, 11)


def _ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def _inverse_times(m: cases.Map, points: np.ndarray) -> np.ndarray:
    """``float32(Minv64 @ p64)``, the product written out term by term so that no BLAS chooses the order of the sum."""
    p, inverse = points.astype(np.float64), m.inverse
    rows = [((inverse[r, 0] * p[:, 0] + inverse[r, 1] * p[:, 1]) + inverse[r, 2] * p[:, 2]) + inverse[r, 3] for r in range(3)]
    return np.stack(rows, axis=1).astype(np.float32)


def test_affine_only_is_the_float64_inverse_rounded_once(hip):
    maps = [cases.Map(cases.voxel_matrix(seed), cases.OUT_SHAPE) for seed in (1, 2, 3)]
    points, offsets, blocks, control = cases.ragged(maps)
    assert control is None
    out, status = cases.warp_on_gpu(hip, points, offsets, blocks, control)
    assert out.shape == points.shape and out.dtype == np.float32 and not status.any()
    for index, m in enumerate(maps):
        lo, hi = offsets[index], offsets[index + 1]
        expected = _inverse_times(m, points[lo:hi])
        ulps = _ulps(out[lo:hi], expected)
        print(f"element {index}: {hi - lo} points, {int((out[lo:hi] != expected).sum())} values differ, max {ulps.max() if ulps.size else 0.0} ulp")
        assert (ulps <= 1.0).all()
        assert np.array_equal(out[lo:hi], expected)


@pytest.mark.parametrize("affine_first", [True, False], ids=["affine_first", "elastic_first"])
@pytest.mark.parametrize("regime", ["gentle", "half_folding"])
def test_elastic_solve_meets_the_bar(hip, regime, affine_first):
    maps = [cases.elastic_map(regime, affine_first, seed) for seed in FIELD_SEEDS]
    points, offsets, blocks, control = cases.ragged(maps)
    out, status = cases.warp_on_gpu(hip, points, offsets, blocks, control)
    assert not status.any(), f"{int((status != 0).sum())} points not converged"
    assert np.isfinite(out).all()
    for index, m in enumerate(maps):
        lo, hi = offsets[index], offsets[index + 1]
        if hi == lo:
            continue
        p = points[lo:hi].astype(np.float64)
        o_ref, status_ref = cases.solve_ref(m, p)
        assert not status_ref.any()  # the float64 reference converges on every point of this case
        outside = np.any((o_ref < 0) | (o_ref > np.asarray(m.out_shape) - 1.0), axis=1)
        residual = np.abs(cases.s_ref(m, out[lo:hi].astype(np.float64))[0] - p).max()
        bar = cases.elastic_bar(m, out[lo:hi])
        print(f"{regime} element {index}: {hi - lo} points ({int(outside.sum())} outside), residual {residual:.3g}, bar {bar:.3g}, "
              f"|o_gpu - o_ref| {np.abs(out[lo:hi] - o_ref).max():.3g}")
        if hi - lo >= 3:
            assert outside.sum() >= (hi - lo) // 3  # a third of the points lie outside the field of view
        assert residual <= bar


def test_elements_with_and_without_a_field_share_one_launch(hip):
    field_map = cases.elastic_map("gentle", True, 11)
    plain = cases.Map(cases.voxel_matrix(4), cases.OUT_SHAPE)
    maps = [plain, field_map, plain, field_map]
    counts = (300, 5, 0, 513)
    points, offsets, blocks, control = cases.ragged(maps, counts)
    assert blocks[0, 37] == -1 and blocks[1, 37] == 0 and blocks[3, 37] == field_map.field.size
    out, status = cases.warp_on_gpu(hip, points, offsets, blocks, control)
    assert not status.any()
    for index, m in enumerate(maps):
        lo, hi = offsets[index], offsets[index + 1]
        if hi == lo:
            continue
        p = points[lo:hi].astype(np.float64)
        assert np.abs(cases.s_ref(m, out[lo:hi].astype(np.float64))[0] - p).max() <= cases.elastic_bar(m, out[lo:hi])
    # the same call without the status output stores the same points
    assert np.array_equal(cases.warp_on_gpu(hip, points, offsets, blocks, control, return_status=False), out)


def test_a_block_that_names_control_points_outside_the_buffer_reads_nothing(hip):
    m = cases.elastic_map("gentle", True, 11)
    points, offsets, blocks, control = cases.ragged([m], (40,))
    blocks[0, 37] = 6.0  # the grid no longer fits the buffer
    out, status = cases.warp_on_gpu(hip, points, offsets, blocks, control)
    assert (status == 2).all()
    assert (_ulps(out, _inverse_times(m, points)) <= 1.0).all()


def test_empty_batches_and_bad_arguments(hip):
    from torchio_amd.ops import EngineError

    empty = hip.warp_points(torch.empty((0, 3), device="cuda"), [0, 0, 0], torch.from_numpy(np.stack([cases.Map(np.eye(4)).block()] * 2)))
    assert empty.shape == (0, 3) and empty.is_cuda
    points = torch.zeros((4, 3), device="cuda")
    block = torch.from_numpy(cases.Map(np.eye(4)).block()[None])
    with pytest.raises(EngineError, match="offsets"):
        hip.warp_points(points, [0, 3], block)  # does not span the points
    with pytest.raises(ValueError):
        hip.warp_points(points, [0, 4], block.float())
    with pytest.raises(TypeError):
        hip.warp_points(points.double(), [0, 4], block)
