"""GPU: ``Engine.centre_draw`` (``tio_centre_law_sums``, ``tio_centre_draw``) and ``Engine.patch_gather``
(``tio_patch_gather``) between ``0xFF`` guards (``guarded_memory.py``): the inputs carved 16-byte aligned (skew 0) and one
element off (skew 1), the tensors ``ops.py`` allocates carved through the shim.  After each call: the guards are intact, every
output element was written, the inputs are unchanged, and the result is the unguarded call's."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import patch_feed_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_untouched
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPE = (40, 33, 31)  # 19 whole segments and a short one
DRAWS = 63  # 189 corner words: three words of padding in front of the record


def _sources():
    values = np.random.default_rng(0).integers(0, 4, SHAPE)
    return {
        "map_float32": (torch.from_numpy(values.astype(np.float32)), None, values.astype(np.float32)),
        "map_uint8": (torch.from_numpy(values.astype(np.uint8)), None, values.astype(np.float32)),
        "labels_int16": (torch.from_numpy(values.astype(np.int16)), [(1, 2.0), (3, 1.0), (1, 0.5)], cases.label_weights(values, [(1, 2.0), (3, 1.0), (1, 0.5)])),
        "labels_int16_no_table": (torch.from_numpy(values.astype(np.int16)), [], cases.label_weights(values, [])),
    }


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("own_stream", [False, True], ids=["uniforms", "own_stream"])
@pytest.mark.parametrize("kind", ["map_float32", "map_uint8", "labels_int16", "labels_int16_no_table"])
def test_centre_draw(hip, kind, own_stream, skew):
    source, table, weights = _sources()[kind]
    patch = (5, 4, 3)
    uniforms = None if own_stream else torch.from_numpy(np.random.default_rng(1).random(DRAWS))
    arena = Arena()
    with guarded_engine_allocations(arena):
        carved_source = carve_like(source, arena, "cuda", skew)
        carved_uniforms = None if uniforms is None else carve_like(uniforms, arena, "cuda", skew)
        draw = hip.centre_draw(carved_source, patch, DRAWS, label_table=table, seed=99, uniforms=carved_uniforms, return_uniforms=True)
        torch.cuda.synchronize()
    # the engine carves the prefix sums, the packed corners + record, the centres and the uniforms used
    assert len(arena.carves) == (1 if own_stream else 2) + 4
    arena.check_guards()
    for tensor in (draw.prefix, draw.packed, draw.centres, draw.uniforms):
        assert arena.owns(tensor)
    for tensor in (draw.prefix, draw.centres, draw.uniforms, draw.corners):
        assert_written(tensor)
    assert draw.prefix.numel() == -(-source.numel() // cases.SEGMENT)
    assert_untouched(draw.packed[3 * DRAWS : draw.packed.numel() - 4])  # the padding in front of the record
    record = draw.record.cpu()
    flat = cases.masked_weights(weights, patch)
    assert float(record[:2].view(torch.float64)) == flat.sum() and record[2:].tolist() == [0, 0]
    assert torch.equal(carved_source, source.cuda()) and (uniforms is None or torch.equal(carved_uniforms, uniforms.cuda()))
    used = draw.uniforms.cpu().numpy()
    assert np.array_equal(used, cases.centre_uniforms(99, DRAWS) if own_stream else uniforms.numpy())
    expected, _, _ = cases.draw_reference(flat, used)
    assert np.array_equal(draw.centres.cpu().numpy(), expected)
    plain = hip.centre_draw(source.cuda(), patch, DRAWS, label_table=table, seed=99, uniforms=None if uniforms is None else uniforms.cuda())
    assert torch.equal(plain.centres, draw.centres) and torch.equal(plain.corners, draw.corners) and torch.equal(plain.prefix, draw.prefix)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32, torch.float64])
@pytest.mark.parametrize("shape,patch", [((2, 13, 11, 10), (5, 4, 3)), ((1, 9, 8, 37), (3, 2, 17)), ((2, 13, 11, 10), (13, 11, 10))])
def test_patch_gather(hip, shape, patch, dtype, skew):
    count = int(np.prod(shape))
    volume = (torch.arange(count, dtype=torch.int64).reshape(shape) % 251).to(dtype)
    limit = np.array(shape[1:]) - np.array(patch)
    corners = np.random.default_rng(2).integers(0, limit + 1, (7, 3)).astype(np.int32)
    corners[0], corners[1], corners[2] = 0, limit, (-3, 40, 1)  # the last one is clamped by the kernel
    arena = Arena()
    with guarded_engine_allocations(arena):
        carved_volume = carve_like(volume, arena, "cuda", skew)
        carved_corners = carve_like(torch.from_numpy(corners), arena, "cuda", skew)
        out = hip.patch_gather(carved_volume, carved_corners, patch)
        torch.cuda.synchronize()
    assert len(arena.carves) == 3  # the engine carves the patches
    arena.check_guards()
    assert arena.owns(out)
    assert_written(out)
    assert torch.equal(carved_volume, volume.cuda()) and torch.equal(carved_corners.cpu(), torch.from_numpy(corners))
    clamped = np.clip(corners, 0, limit)
    expected = torch.stack([volume[:, i : i + patch[0], j : j + patch[1], k : k + patch[2]] for i, j, k in clamped.tolist()])
    assert torch.equal(out.cpu(), expected)
    assert torch.equal(out, hip.patch_gather(volume.cuda(), torch.from_numpy(corners), patch))
