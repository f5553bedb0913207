"""GPU: ``Engine.channel_scatter``, ``Engine.channel_project`` and ``tio.PCA`` between ``0xFF`` guards (``guarded_memory.py``):
the inputs carved 16-byte aligned (skew 0) and one element off (skew 1), every tensor ``ops.py`` allocates carved through the
shim.  After each call: the guards are intact, no output element was left unwritten, and the result is the unguarded call's."""
from __future__ import annotations

import pytest
import torch

import pca_cases as cases
import torchio_amd as tio
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 17, 3, 5, 67), (1, 3, 1, 1, 3), (1, 1, 1, 1, 1)]
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


def _data(shape):
    return cases.make_input(shape[1], shape[2:], seed=shape[-1], batch=shape[0])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _guarded(call, inputs, skew, engine_carves):
    """``call(*inputs)`` with every input carved at ``skew`` and the engine's allocations carved: its outputs (a tuple)."""
    arena = Arena()
    with guarded_engine_allocations(arena):
        outs = call(*[carve_like(tensor, arena, "cuda", skew) for tensor in inputs])
    assert len(arena.carves) == len(inputs) + engine_carves
    arena.check_guards()
    plain = call(*[tensor.cuda() for tensor in inputs])
    for out, expected in zip(outs, plain, strict=True):
        assert arena.owns(out)
        assert_written(out)
        assert _same_bits(out, expected)
    return outs


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_channel_scatter(hip, shape, skew):
    # the engine carves the means, the scatter matrices and the workspace of per-chunk partials
    mean, scatter = _guarded(lambda x: hip.channel_scatter(x), [_data(shape)], skew, 3)
    assert mean.shape == shape[:2] and scatter.shape == (shape[0], shape[1], shape[1])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_channel_project(hip, shape, clip, skew):
    batch, channels = shape[:2]
    components = min(channels, 3)
    generator = torch.Generator().manual_seed(channels)
    center = torch.randn(batch, channels, generator=generator)
    weights = torch.randn(batch, components, channels, generator=generator)
    offset = torch.randn(batch, components, generator=generator)
    (out,) = _guarded(lambda x, m, w, o: (hip.channel_project(x, m, w, o, clip=clip),), [_data(shape), center, weights, offset], skew, 1)
    assert out.shape == (batch, components, *shape[2:])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_transform(hip, shape, skew):
    components = min(shape[1], 3)

    def call(x):
        batch = cases.batch_of(tio, torch.zeros(shape), "cuda")
        batch.images["emb"].data = x  # the carved tensor itself is what the kernels read
        return (tio.PCA(num_components=components, normalize=shape[2:] != (1, 1, 1))(batch).images["emb"].data,)

    # the engine carves the means, the scatter matrices, the workspace and the result
    (out,) = _guarded(call, [_data(shape)], skew, 4)
    assert out.shape == (shape[0], components, *shape[2:])
