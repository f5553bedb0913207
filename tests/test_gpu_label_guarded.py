"""GPU: the four label-map engine methods between ``0xFF`` guards (``guarded_memory.py``): the input carved 16-byte aligned
(skew 0) and one element off (skew 1), every output and scratch tensor of ``ops.py`` carved through the shim.  After each
call: the guards are intact, no output element was left unwritten, and the result is the unguarded call's."""
from __future__ import annotations

import pytest
import torch

import label_cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
DTYPES = [torch.uint8, torch.int16, torch.int32, torch.float32]  # the 8-bit table, the 16-bit table, the search; never a canary value


def _guarded(call, data, skew, carves):
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = call(carve_like(data, arena, "cuda", skew))
    assert len(arena.carves) == 1 + carves and arena.owns(out)
    arena.check_guards()
    assert_written(out)
    assert torch.equal(out, call(data.cuda()))
    return out


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_remap(hip, shape, dtype, skew):
    data = label_cases.label_field(shape, 0).to(dtype)
    mapping = {0: 2, 2: 0, 3: 5}
    out = _guarded(lambda x: hip.label_remap(x, mapping), data, skew, 2 if dtype == torch.int16 else 1)
    assert torch.equal(out.cpu(), label_cases.remap(data, mapping))
    _guarded(lambda x: hip.label_remap(x, mapping, default=1), data, skew, 2 if dtype == torch.int16 else 1)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_one_hot(hip, shape, dtype, skew):
    data = label_cases.label_field(shape, 1).to(dtype)
    out = _guarded(lambda x: hip.label_one_hot(x, 5), data, skew, 2)  # the output and the status word
    assert torch.equal(out.cpu(), label_cases.one_hot(data, 5))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_contour(hip, shape, dtype, skew):
    data = label_cases.label_field(shape, 2).to(dtype)
    out = _guarded(hip.label_contour, data, skew, 1)
    assert torch.equal(out.cpu(), label_cases.contour(data))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("fully_connected", [True, False], ids=["26", "6"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_keep_largest_component(hip, shape, dtype, fully_connected, skew):
    data = label_cases.label_field(shape, 0).to(dtype)
    labels = [0, 1, 3]
    out = _guarded(lambda x: hip.keep_largest_component(x, labels, background=2, fully_connected=fully_connected), data, skew, 2)
    assert torch.equal(out.cpu(), label_cases.keep_largest(data, labels, 2, fully_connected))
