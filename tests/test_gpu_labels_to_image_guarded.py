"""GPU: ``Engine.labels_to_image`` in both modes between ``0xFF`` guards (``guarded_memory.py``): the inputs carved 16-byte
aligned (skew 0) and one element off (skew 1), every tensor ``ops.py`` allocates carved through the shim.  After each call:
the guards are intact, no output element was left unwritten, and the result is the unguarded call's."""
from __future__ import annotations

import pytest
import torch

import labels_to_image_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
DTYPES = [torch.float32, torch.float64, torch.int16, torch.uint8]  # 4-, 8-, 2- and 1-byte elements
VALUES, KEYS = [0, 1, 2, 3, 20], [0, 1, 3, 20]  # (never the canary: 255, -1 or NaN); 2 has no key
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


def _labels(shape, dtype):
    return torch.stack([cases.label_volume(shape[2:], VALUES, shift) for shift in range(shape[0])]).to(dtype)


def _parameters(batch, batched):
    means, stds = [0.5, 0.25, 0.75, 1.5], [0.1, 0.2, 0.05, 0.3]
    return ([means] * batch, [stds[::-1]] * batch) if batched else (means, stds)


def _guarded(call, inputs, skew, engine_carves):
    """``call(*inputs)`` with every input carved at ``skew`` and the engine's allocations carved; returns the result."""
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = call(*[carve_like(tensor, arena, "cuda", skew) for tensor in inputs])
    assert len(arena.carves) == len(inputs) + engine_carves
    arena.check_guards()
    plain = call(*[tensor.cuda() for tensor in inputs])
    assert arena.owns(out)
    assert_written(out)
    assert out.dtype == plain.dtype and torch.equal(out.view(torch.int32), plain.view(torch.int32))
    return out


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_mode(hip, shape, dtype, batched, skew):
    means, stds = _parameters(shape[0], batched)
    # the engine carves its output and the staging block of the one packed upload
    out = _guarded(lambda x: hip.labels_to_image(x, KEYS, means, stds, seed=17), [_labels(shape, dtype)], skew, 2)
    assert out.shape == (shape[0], 1, *shape[2:])
    assert torch.equal(out == 0, (_labels(shape, dtype)[:, :1] == 2).cuda())


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_label_mode(hip, shape, dtype, batched, skew):
    means, stds = _parameters(shape[0], batched)
    labels = _labels(shape, dtype)
    base = torch.randn(shape[0], 1, *shape[2:], generator=torch.Generator().manual_seed(shape[-1]))
    # out=None: the engine carves the output (and clears it) and the staging block
    fresh = _guarded(lambda x, z: hip.labels_to_image(x, KEYS, means, stds, base=z, base_key=3), [labels, base], skew, 2)
    assert torch.equal(fresh != 0, (labels == 20).cuda())
    # the caller's own output, carved and skewed like the inputs: only the voxels of the label change
    held = torch.full(base.shape, 9.0)
    out = _guarded(lambda x, z, o: hip.labels_to_image(x, KEYS, means, stds, base=z, base_key=1, out=o), [labels, base, held], skew, 1)
    assert torch.equal(out != 9.0, (labels == 1).cuda())
