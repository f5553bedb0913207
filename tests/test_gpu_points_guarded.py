"""GPU: ``Engine.warp_points`` (``tio_points_warp``) between ``0xFF`` guards (``guarded_memory.py``): the points, the control
points and the parameter blocks carved 16-byte aligned (skew 0) and one element off (skew 1: the float32 buffers 4 bytes
off), the tensors ``ops.py`` allocates carved through the shim.  After each call: the guards are intact, no output element
was left unwritten, and the result is the unguarded call's."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import annotation_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu


def _case(kind: str):
    if kind == "affine":
        maps = [cases.Map(cases.voxel_matrix(seed), cases.OUT_SHAPE) for seed in (1, 2, 3)]
    else:
        maps = [cases.elastic_map("half_folding", kind == "affine_first", seed) for seed in (15, 15, 11)]
    points, offsets, blocks, control = cases.ragged(maps)
    return torch.from_numpy(points), torch.from_numpy(offsets), torch.from_numpy(blocks), None if control is None else torch.from_numpy(control)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("kind", ["affine", "affine_first", "elastic_first"])
def test_device_inputs(hip, kind, skew):
    points, offsets, blocks, control = _case(kind)
    arena = Arena()
    with guarded_engine_allocations(arena):
        carved = [None if t is None else carve_like(t, arena, "cuda", skew) for t in (points, blocks, control)]
        out, status = hip.warp_points(carved[0], offsets, carved[1], carved[2], return_status=True)
    # the engine carves the moved points and the status
    assert len(arena.carves) == sum(t is not None for t in carved) + 2
    arena.check_guards()
    plain, plain_status = hip.warp_points(points.cuda(), offsets, blocks.cuda(), None if control is None else control.cuda(), return_status=True)
    assert arena.owns(out) and arena.owns(status)
    assert_written(out)
    assert_written(status)
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32)) and torch.equal(status, plain_status)
    assert not bool(status.any())


@pytest.mark.parametrize("skew", [0, 1])
def test_host_parameters_go_through_one_staging_copy(hip, skew):
    points, offsets, blocks, control = _case("affine_first")
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = hip.warp_points(carve_like(points, arena, "cuda", skew), offsets, blocks, control)
    # the points; the engine carves the pinned staging block's source and the moved points
    assert len(arena.carves) == 3
    arena.check_guards()
    assert arena.owns(out)
    assert_written(out)
    plain = hip.warp_points(points.cuda(), offsets, blocks.cuda(), control.cuda())
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    assert np.isfinite(out.cpu().numpy()).all()
