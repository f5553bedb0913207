"""GPU: the intensity-statistics engine methods between ``0xFF`` guards (``guarded_memory.py``): the input — and the mask —
carved 16-byte aligned (skew 0) and one element off (skew 1), every output and scratch tensor of ``ops.py`` carved through
the shim.  After each call: the guards are intact, no output element was left unwritten, and the result is the unguarded
call's."""
from __future__ import annotations

import pytest
import torch

import intensity_stats_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
DTYPES = [torch.float32, torch.float64, torch.int16, torch.uint8]  # 4-, 8-, 2- and 1-byte elements
FRACTIONS = [0.005, 0.995]


def _data(shape, dtype):
    generator = torch.Generator().manual_seed(len(shape) + shape[-1])
    if dtype.is_floating_point:
        return (torch.randn(shape, generator=generator) * 40 + 20).to(dtype)
    return torch.randint(0, 200, shape, generator=generator).to(dtype)  # (never 255: the canary of uint8)


def _mask(shape):
    return cases.label_cases.label_field((1, 1, *shape[2:]), 4)[0].to(torch.int16)  # (1, I, J, K), values 0..3


def _guarded(call, inputs, skew, engine_carves, tensor_result=True):
    """``call(*inputs)`` with every input carved at ``skew`` and the engine's allocations carved; returns the result."""
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = call(*[carve_like(tensor, arena, "cuda", skew) for tensor in inputs])
    assert len(arena.carves) == len(inputs) + engine_carves
    arena.check_guards()
    plain = call(*[tensor.cuda() for tensor in inputs])
    if tensor_result:
        assert arena.owns(out)
        assert_written(out)
        assert out.dtype == plain.dtype and torch.equal(out, plain)
    else:
        assert out == plain or all(a == b or (a != a and b != b) for a, b in zip(out, plain, strict=True))
    return out


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_moments(hip, shape, dtype, skew):
    data, mask = _data(shape, dtype), _mask(shape)
    count, mean, std = _guarded(hip.intensity_moments, [data], skew, 2, tensor_result=False)  # the record and the workspace
    assert count == data[0].numel() and mean == mean
    count, _, _ = _guarded(hip.intensity_moments, [data, mask], skew, 2, tensor_result=False)
    assert count == int(mask.bool().sum())


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiles(hip, shape, dtype, skew):
    data, mask = _data(shape, dtype), _mask(shape)
    values = _guarded(lambda x: hip.intensity_quantiles(x, FRACTIONS), [data], skew, 2, tensor_result=False)
    assert values == [cases.compute_quantile(cases.inside_values(data[0], None), q) for q in FRACTIONS]
    inside = cases.inside_values(data[0], mask)
    values, count = _guarded(lambda x, m: hip.intensity_quantiles(x, FRACTIONS, m, return_count=True), [data, mask], skew, 2, tensor_result=False)
    assert count == inside.numel()
    if count:
        assert values == [cases.compute_quantile(inside, q) for q in FRACTIONS]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map(hip, shape, dtype, skew):
    data = _data(shape, dtype)
    out = _guarded(lambda x: hip.intensity_map(x, "rescale_clip", in_min=-3.5, in_max=91.25, in_range=94.75, out_min=-1.0, out_range=2.0), [data], skew, 1)
    assert torch.equal(out.cpu(), cases.normalize(data, -3.5, 91.25, -1.0, 1.0))
    low = torch.tensor([0.1, -0.3][: shape[0]])
    span = torch.tensor([0.6, 0.0][: shape[0]])
    _guarded(lambda x, a, b: hip.intensity_map(x, "rescale", in_min=-3.5, in_range=94.75, out_min=a, out_range=b), [data, low, span], skew, 1)
    _guarded(lambda x: hip.intensity_map(x, "sub_div", in_min=20.5, in_range=40.25), [data], skew, 1)
    _guarded(lambda x: hip.intensity_map(x, "mul_add", in_min=20.5, in_range=40.25), [data], skew, 1)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES + [torch.float16], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clamp(hip, shape, dtype, skew):
    data = _data(shape, dtype)
    out = _guarded(lambda x: hip.clamp(x, 10.5, 60.25), [data], skew, 1)
    assert cases.same(out.cpu(), cases.clamp(data, 10.5, 60.25))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES + [torch.float16], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_where(hip, shape, dtype, skew):
    data, mask = _data(shape, dtype), _mask(shape)
    out = _guarded(lambda x, m: hip.mask_where(x, m, -7.5), [data, mask], skew, 1)
    assert cases.same(out.cpu(), cases.mask_where(data, mask, -7.5))
