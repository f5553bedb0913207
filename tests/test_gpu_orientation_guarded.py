"""GPU: ``tio_permute3d`` between ``0xFF`` guards (``guarded_memory.py``), input and output shifted off 16-byte alignment by
0, 1 and 3 elements.  After each call the guards are intact, every output element was written, and the result is the
ATen sequence's.  This is the test that sees an edge tile reading or writing past its row."""
from __future__ import annotations

import pytest
import torch

import orientation_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations
from torchio_amd import ops

pytestmark = pytest.mark.gpu

SKEWS = (0, 1, 3)
MASKS = (0, 5, 7)  # none, the two outer axes, all three: a flip reverses the direction an edge tile is walked in
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


@pytest.mark.parametrize("shape", cases.PERMUTE_SHAPES, ids=ids)
def test_permute3d_stays_inside_its_buffers(hip, shape):
    for dtype in cases.PERMUTE_DTYPES:
        plain = cases.distinct((2, 2, *shape), dtype, "cuda")
        for perm in cases.PERMUTATIONS:
            for mask in MASKS:
                expected = cases.aten_permute(plain, perm, mask)
                flips = [axis for axis in range(3) if mask & (1 << axis)]
                for skew in SKEWS:
                    # through the engine: the input skewed, the output carved by the engine's own allocation
                    arena = Arena()
                    with guarded_engine_allocations(arena):
                        out = hip.permute3d(carve_like(plain, arena, "cuda", skew), perm, flips)
                    assert len(arena.carves) == 2 and arena.owns(out)
                    arena.check_guards()
                    assert_written(out)
                    assert torch.equal(out, expected), (dtype, perm, mask, skew)
                    # the entry point itself: input and output both skewed
                    arena = Arena()
                    x = carve_like(plain, arena, "cuda", skew)
                    y = arena.carve(expected.shape, dtype, "cuda", skew)
                    hip._call("permute3d", x, ops._ptr(x), ops._ptr(y), ops.dtype_code(dtype), 2, 2, ops._i32x3(shape), ops._i32x3(perm), mask,
                              hip._stream(x))
                    arena.check_guards()
                    assert_written(y)
                    assert torch.equal(y, expected), (dtype, perm, mask, skew)
