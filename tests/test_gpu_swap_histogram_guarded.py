"""GPU: ``swap_patches``, ``intensity_multi_quantiles`` and ``histogram_standardize`` between ``0xFF`` guards
(``guarded_memory.py``): the input — and the mask — carved 16-byte aligned (skew 0) and one element off (skew 1), every output
and scratch tensor of ``ops.py`` carved through the shim.  After each call: the guards are intact, no output element was left
unwritten, and the result is the unguarded call's."""
from __future__ import annotations

import pytest
import torch

import swap_histogram_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
DTYPES = [torch.float32, torch.float64, torch.int16, torch.uint8]  # 4-, 8-, 2- and 1-byte elements
OVERLAP_SHAPE, OVERLAP_PATCH = (2, 2, 5, 6, 7), (3, 4, 4)  # every pair of patches overlaps


def _data(shape, dtype):
    generator = torch.Generator().manual_seed(len(shape) + shape[-1])
    if dtype.is_floating_point:
        return (torch.randn(shape, generator=generator) * 40 + 20).to(dtype)
    return torch.randint(0, 200, shape, generator=generator).to(dtype)  # (never 255: the canary of uint8)


def _mask(shape):
    return cases.label_cases.label_field((1, 1, *shape[2:]), 4)[0].to(torch.int16)  # (1, I, J, K), values 0..3


def _guarded(call, inputs, skew, engine_carves):
    """``call(*inputs)`` with every input carved at ``skew`` and the engine's allocations carved; returns the results."""
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = call(*[carve_like(tensor, arena, "cuda", skew) for tensor in inputs])
    assert len(arena.carves) == len(inputs) + engine_carves
    arena.check_guards()
    plain = call(*[tensor.cuda() for tensor in inputs])
    outs, plains = (out, plain) if isinstance(out, tuple) else ((out,), (plain,))
    for got, expected in zip(outs, plains, strict=True):
        assert arena.owns(got)
        assert_written(got)
        assert got.dtype == expected.dtype and torch.equal(got, expected)
    return out


def _patch_for(shape):
    return tuple(max(1, (s + 1) // 2) for s in shape[2:])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES + [OVERLAP_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_swap_patches(hip, shape, dtype, skew):
    data = _data(shape, dtype)
    patch = OVERLAP_PATCH if shape == OVERLAP_SHAPE else _patch_for(shape)
    shared = cases.random_locations(shape[2:], patch, 9, 1)
    out = _guarded(lambda x: hip.swap_patches(x, shared, patch), [data], skew, 1)
    assert torch.equal(out.cpu(), cases.swap_sequential(data, shared, patch))
    per_element = [cases.random_locations(shape[2:], patch, 5, 2), []][: shape[0]]
    out = _guarded(lambda x: hip.swap_patches(x, per_element, patch), [data], skew, 1)
    assert torch.equal(out.cpu(), cases.swap_sequential(data, per_element, patch))
    _guarded(lambda x: hip.swap_patches(x, [], patch), [data], skew, 1)  # the plain copy


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_multi_quantiles(hip, shape, dtype, skew):
    data, mask = _data(shape, dtype), _mask(shape)
    values, counts = _guarded(lambda x: hip.intensity_multi_quantiles(x, cases.DEFAULT_QUANTILES), [data], skew, 3)  # values, counts, workspace
    for b in range(shape[0]):
        assert cases.same_bits64(values[b].cpu().numpy(), cases.percentiles(data[b], cases.DEFAULT_QUANTILES))
    assert counts.tolist() == [data[0].numel()] * shape[0]
    if int(mask.bool().sum()):  # (nothing inside: NaN, which the written-check takes for the canary)
        values, counts = _guarded(lambda x, m: hip.intensity_multi_quantiles(x, cases.DEFAULT_QUANTILES, m), [data, mask], skew, 3)
        assert counts.tolist() == [int(mask.bool().sum())] * shape[0]
        for b in range(shape[0]):
            assert cases.same_bits64(values[b].cpu().numpy(), cases.percentiles(cases.inside_values(data[b], mask), cases.DEFAULT_QUANTILES))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int16, torch.float16], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_standardize(hip, shape, dtype, skew):
    data = _data(shape, dtype)
    landmarks = cases.landmarks_for(cases.DEFAULT_QUANTILES) + 10.0  # (no result near -1, the canary of int16)
    # values, counts, workspace of the selection; the output and the table
    out = _guarded(lambda x: hip.histogram_standardize(x, landmarks, cases.DEFAULT_QUANTILES), [data], skew, 5)
    assert cases.same(out.cpu(), cases.standardize(data, landmarks, cases.DEFAULT_QUANTILES))
