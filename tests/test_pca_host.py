"""``tio.PCA`` without a GPU: the export, the constructor and channel-count errors, the plan and workspace arithmetic of
``tio_channel_scatter`` (host only, nothing is enqueued), and the fixture's own consistency with ``exact_pca``."""
from __future__ import annotations

import ctypes
import os

import pytest
import torch

import pca_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_golden.pt")


def test_pca_is_exported():
    from torchio_amd import transforms

    assert tio.PCA is transforms.PCA and "PCA" in tio.__all__ and "PCA" in transforms.__all__
    assert issubclass(tio.PCA, tio.IntensityTransform)


def test_invalid_num_components_raises():
    with pytest.raises(ValueError, match="num_components must be >= 1, got 0"):
        tio.PCA(num_components=0)


def test_too_few_channels_raises_before_the_engine_is_touched():
    batch = cases.batch_of(tio, torch.rand(2, 2, 4, 4, 4))  # on the CPU: the engine would refuse it
    with pytest.raises(ValueError, match="Image has 2 channels but num_components=5"):
        tio.PCA(num_components=5)(batch)


def test_make_params_is_empty():
    assert tio.PCA().make_params(cases.batch_of(tio, torch.rand(1, 3, 2, 2, 2))) == {}


def test_engine_methods_refuse_cpu_tensors():
    from torchio_amd import ops

    engine = ops.Engine(_lib.load()[1], "cuda", "hip")
    with pytest.raises(ops.EngineError, match="runs on cuda tensors"):
        engine.channel_scatter(torch.rand(1, 3, 2, 2, 2))
    with pytest.raises(ops.EngineError, match="runs on cuda tensors"):
        engine.channel_project(torch.rand(1, 3, 2, 2, 2), torch.zeros(1, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2), clip=True)


@pytest.mark.parametrize("batch", [1, 2, 16])
@pytest.mark.parametrize("channels", [1, 3, 16, 17, 40, 70, 128, 1024])
@pytest.mark.parametrize("voxels", [1, 3, 210, 1003, 40_000, 128**3])
def test_scatter_plan_and_workspace_are_consistent(batch, channels, voxels):
    _, functions = _lib.load()
    plan = (ctypes.c_int32 * 4)()
    assert functions["channel_scatter_plan"](batch, channels, voxels, plan) == 0
    chunks, chunk_voxels, pairs_per_block, grid = plan
    tiles = (channels + 15) // 16
    assert chunks >= 1 and chunk_voxels % 16 == 0
    assert chunks * chunk_voxels >= voxels > (chunks - 1) * chunk_voxels  # the chunks cover the voxels, none is empty
    assert 1 <= pairs_per_block <= 8  # 8 tiles of 4 doubles: 64 accumulator registers per lane
    pairs = tiles * (tiles + 1) // 2
    assert grid % (chunks * batch) == 0
    groups = grid // (chunks * batch)
    assert -(-pairs // pairs_per_block) <= groups <= pairs  # every upper tile pair belongs to a block
    assert functions["channel_scatter_workspace_bytes"](batch, channels, voxels) >= chunks * batch * (16 * tiles) ** 2 * 8


def test_scatter_argument_errors_return_minus_one_and_name_the_entry_point():
    _, functions = _lib.load()
    plan = (ctypes.c_int32 * 4)()
    buffer = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buffer))
    for arguments in ((1, 0, 10), (1, _abi.PCA_MAX_CHANNELS + 1, 10), (1, 3, 0), (-1, 3, 10)):
        assert functions["channel_scatter_plan"](*arguments, plan) == -1
        assert b"tio_channel_scatter_plan" in functions["last_error"]()
        assert functions["channel_scatter_workspace_bytes"](*arguments) == -1
        assert b"tio_channel_scatter_workspace_bytes" in functions["last_error"]()
    assert functions["channel_scatter_plan"](1, 3, 10, None) == -1
    # the compute entry points validate on the host before any launch
    assert functions["channel_scatter"](None, 1, 3, 10, p, p, p, 4096, None) == -1
    assert b"tio_channel_scatter: null" in functions["last_error"]()
    assert functions["channel_scatter"](p, 1, 2000, 10, p, p, p, 4096, None) == -1
    assert functions["channel_scatter"](p, 1, 3, 10, p, p, p, 8, None) == -1
    assert b"workspace" in functions["last_error"]()
    assert functions["channel_project"](p, 1, 3, 10, p, p, p, 4, 0, p, None) == -1
    assert b"tio_channel_project" in functions["last_error"]() and b"components" in functions["last_error"]()
    assert functions["channel_project"](p, 1, 3, 10, p, None, p, 2, 0, p, None) == -1
    assert b"tio_channel_project: null" in functions["last_error"]()
    assert functions["channel_project"](p, 1, 3, 10, p, p, p, 2, 0, p, None) == -1
    assert b"overlaps" in functions["last_error"]()


def test_header_declares_no_dtype_parameter_for_the_pca_entry_points():
    import re

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tio_hip.h")
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = dict(re.findall(r"\btio_(channel_(?:scatter|project)[a-z0-9_]*)\s*\(([^;{}]*)\)\s*;", text))
    assert sorted(declared) == ["channel_project", "channel_scatter", "channel_scatter_plan", "channel_scatter_workspace_bytes"]
    assert not any("dtype" in arguments for arguments in declared.values())


def test_fixture_agrees_with_exact_pca_within_its_recorded_deviation():
    golden = torch.load(GOLDEN)
    assert golden["seed"] == cases.GOLDEN_SEED and set(golden["cases"]) == set(cases.GOLDEN_CASES)
    for name, entry in golden["cases"].items():
        builder, arguments = cases.GOLDEN_CASES[name]
        assert torch.equal(entry["input"], cases.make_input(**builder)), name
        assert entry["dev_ref"] <= 2e-6, name
        for b in range(entry["input"].shape[0]):
            exact = cases.exact_pca(entry["input"][b], **arguments)
            excess = cases.flip_excess(entry["out"][b].numpy(), exact["out"], entry["dev_ref"])
            assert (excess <= 0).all(), (name, b, excess)


def test_exact_pca_sign_convention_and_scaling():
    data = cases.make_input(5, (4, 5, 6), seed=11)[0]
    exact = cases.exact_pca(data, 2, clip=False)
    loadings = exact["weights"] / abs(exact["weights"]).max(axis=1, keepdims=True)
    assert (loadings.max(axis=1) == 1.0).all()  # the entry of largest magnitude is the positive one
    projected = (exact["out"].reshape(2, -1) - 0.5) * 4.6
    assert abs(projected[0].std(ddof=1) - 1.0) < 1e-12 and abs(projected[1].std(ddof=1) - 1.0) < 1e-12  # whitened, normalised
    assert abs(projected.mean(axis=1)).max() < 1e-12
