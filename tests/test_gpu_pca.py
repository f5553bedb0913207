"""GPU: ``tio_channel_scatter`` against float64 numpy, ``tio.PCA`` against ``exact_pca`` (``pca_cases.py``) and against the
reference's recorded outputs, ``tio_channel_project`` alone, and the reference's own five PCA tests on device batches.

Bars.  Scatter: ``|dS_ij| <= 1e-9 sqrt(S_ii S_jj)`` — float64 accumulation of exact products costs at most ``V 2^-53``, about
1e-11 at 1e5 voxels, times ``1 + d^2`` with ``d = |mean - pivot| / deviation``, a handful for a pivot drawn from the data; an
unpivoted ``sum x x^T - V mean mean^T`` misses it by orders of magnitude on the offset case.  Mean: ``1e-12 max(|mean|,
deviation)``.  Transform: ``(C + 4) 2^-24 (sum_c |W_kc| |x_c - mean_c| + |o_k|)`` per voxel and component, the float32
rounding of a ``C``-term centred dot product, computed in float64 from ``exact_pca``'s own weights.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import pca_cases as cases
import torchio_amd as tio
from torchio_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_golden.pt")
CHANNELS = [1, 3, 16, 17, 40, 70]  # one tile, its edge, two tiles' edge, three tiles (two pair groups), five tiles
VOXELS = {1: (1, 1, 1), 3: (1, 3, 1), 210: (5, 6, 7), 1003: (17, 1, 59)}


def _plan(batch, channels, voxels):
    plan = (ctypes.c_int32 * 4)()
    assert _lib.load()[1]["channel_scatter_plan"](batch, channels, voxels, plan) == 0
    return tuple(plan)


def _assert_scatter(hip, data):
    """``Engine.channel_scatter`` of float32 ``(B, C, I, J, K)`` host ``data`` within the bars, twice with the same bits."""
    device = data.cuda()
    mean, scatter = hip.channel_scatter(device)
    again_mean, again_scatter = hip.channel_scatter(device)
    batch, channels = data.shape[:2]
    assert mean.dtype == scatter.dtype == torch.float64
    assert mean.shape == (batch, channels) and scatter.shape == (batch, channels, channels)
    assert torch.equal(mean.view(torch.int64), again_mean.view(torch.int64))
    assert torch.equal(scatter.view(torch.int64), again_scatter.view(torch.int64))
    assert torch.equal(scatter.view(torch.int64), scatter.transpose(1, 2).contiguous().view(torch.int64))  # symmetric bit for bit
    expected_mean, expected_scatter = cases.scatter_reference(data)
    mean, scatter = mean.cpu().numpy(), scatter.cpu().numpy()
    diagonal = np.sqrt(np.einsum("bii->bi", expected_scatter))
    voxels = data[0, 0].numel()
    deviation = diagonal / np.sqrt(max(voxels - 1, 1))
    scatter_error = np.abs(scatter - expected_scatter) - 1e-9 * diagonal[:, :, None] * diagonal[:, None, :]
    mean_error = np.abs(mean - expected_mean) - 1e-12 * np.maximum(np.abs(expected_mean), deviation)
    print(f"scatter {tuple(data.shape)}: worst |dS| / sqrt(S_ii S_jj) = "
          f"{np.max(np.abs(scatter - expected_scatter) / np.maximum(diagonal[:, :, None] * diagonal[:, None, :], 1e-300)):.3e}, "
          f"worst |dmean| / max(|mean|, deviation) = {np.max(np.abs(mean - expected_mean) / np.maximum(np.maximum(np.abs(expected_mean), deviation), 1e-300)):.3e}")
    assert scatter_error.max() <= 0, np.unravel_index(scatter_error.argmax(), scatter_error.shape)
    assert mean_error.max() <= 0, np.unravel_index(mean_error.argmax(), mean_error.shape)


@pytest.mark.parametrize("voxels", list(VOXELS))
@pytest.mark.parametrize("channels", CHANNELS)
def test_scatter_against_float64_numpy(hip, channels, voxels):
    _assert_scatter(hip, cases.make_input(channels, VOXELS[voxels], seed=channels + voxels, batch=2))


def test_scatter_over_several_chunks_and_tile_pair_groups(hip):
    channels, voxels = 40, 40_003  # (an odd count: the last chunk ends inside a step)
    chunks, chunk_voxels, pairs_per_block, grid = _plan(1, channels, voxels)
    assert chunks >= 3 and grid // chunks >= 2 and chunks * chunk_voxels >= voxels, (chunks, chunk_voxels, pairs_per_block, grid)
    _assert_scatter(hip, cases.make_input(channels, (1, 13, 3077), seed=77))


def test_scatter_with_means_ten_thousand_deviations_up(hip):
    generator = torch.Generator().manual_seed(8)
    data = (1000.0 + 0.1 * torch.randn(2, 17, 17, 1, 59, dtype=torch.float64, generator=generator)).to(torch.float32)
    _assert_scatter(hip, data)


def test_scatter_of_an_unaligned_view(hip):
    """The base pointer one, two and three elements off a 16-byte boundary."""
    data = cases.make_input(17, VOXELS[1003], seed=5, batch=2)
    for skew in (1, 2, 3):
        holder = torch.empty(data.numel() + 4, dtype=torch.float32, device="cuda")
        view = holder[skew : skew + data.numel()].view(data.shape)
        view.copy_(data)
        assert view.data_ptr() % 16 == 4 * skew
        mean, scatter = hip.channel_scatter(view)
        base_mean, base_scatter = hip.channel_scatter(data.cuda())
        assert torch.equal(mean, base_mean) and torch.equal(scatter, base_scatter)


ARGUMENTS = [dict(whiten=w, normalize=n, clip=c) for w in (True, False) for n in (True, False) for c in (True, False)]


def _assert_transform(data, arguments):
    """``tio.PCA(**arguments)`` on the device batch of ``data`` (any dtype) against ``exact_pca``, per voxel and component."""
    out = tio.PCA(**arguments)(cases.batch_of(tio, data, "cuda")).images["emb"].data
    components = arguments.get("num_components", 3)
    assert out.dtype == torch.float32 and out.device.type == "cuda" and out.shape == (data.shape[0], components, *data.shape[2:])
    out = out.cpu().numpy().astype(np.float64)
    for b in range(data.shape[0]):
        exact = cases.exact_pca(data[b], **arguments)
        bound = cases.rounding_bound(exact)
        excess = np.abs(out[b] - exact["out"]) - bound
        print(f"PCA {tuple(data.shape)} {data.dtype} {arguments}: worst |out - exact| / bound = {np.max(np.abs(out[b] - exact['out']) / bound):.3f}")
        assert excess.max() <= 0, (arguments, b, np.unravel_index(excess.argmax(), excess.shape), float(excess.max()))
    if arguments.get("clip", True):
        assert out.min() >= 0.0 and out.max() <= 1.0
    return out


@pytest.mark.parametrize("channels,components", [(c, q) for c in CHANNELS for q in (1, 3, 5) if q <= c])
def test_transform_against_exact_pca(hip, channels, components):
    data = cases.make_input(channels, (5, 6, 7), seed=10 * channels + components, batch=2)
    for arguments in ARGUMENTS:
        _assert_transform(data, dict(num_components=components, **arguments))
    _assert_transform(data, dict(num_components=components, values_range=(-1.0, 3.0), clip=False))
    _assert_transform(data, dict(num_components=components, values_range=(-1.0, 3.0)))


@pytest.mark.parametrize("dtype", [torch.int16, torch.float64], ids=str)
def test_transform_of_other_dtypes_is_the_transform_of_their_float32_values(hip, dtype):
    data = cases.make_input(17, (5, 6, 7), seed=3, batch=2).to(torch.float64)
    data = (100.0 * data).round().to(torch.int16) if dtype == torch.int16 else data + 1e-9 * torch.arange(data.numel()).reshape(data.shape)
    assert data.dtype == dtype
    for clip in (True, False):
        out = _assert_transform(data, dict(num_components=3, clip=clip))
        same = tio.PCA(num_components=3, clip=clip)(cases.batch_of(tio, data.to(torch.float32), "cuda")).images["emb"].data
        assert np.array_equal(out, same.cpu().numpy().astype(np.float64))


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES))
def test_transform_against_the_reference_fixture(hip, golden, name):
    entry = golden["cases"][name]
    _, arguments = cases.GOLDEN_CASES[name]
    out, next_rand = cases.run_case(tio, name, entry["input"], "cuda")
    assert torch.equal(next_rand, entry["next_rand"])  # the generator is where the reference leaves it
    out = out.cpu().numpy().astype(np.float64)
    for b in range(entry["input"].shape[0]):
        exact = cases.exact_pca(entry["input"][b], **arguments)
        excess = cases.flip_excess(out[b], entry["out"][b].numpy(), cases.rounding_bound(exact) + entry["dev_ref"])
        assert (excess <= 0).all(), (name, b, excess)


def _projection_inputs(channels, components, shape=(1, 3, 5, 67), seed=0):
    generator = torch.Generator().manual_seed(seed)
    data = torch.randn(shape[0], channels, *shape[1:], generator=generator)
    center = torch.randn(shape[0], channels, generator=generator)
    weights = torch.randn(shape[0], components, channels, generator=generator)
    offset = torch.randn(shape[0], components, generator=generator)
    return data.cuda(), center.cuda(), weights.cuda(), offset.cuda()


@pytest.mark.parametrize("clip", [False, True])
def test_project_keeps_a_nan_voxel_nan_in_every_component_and_changes_nothing_else(hip, clip):
    data, center, weights, offset = _projection_inputs(5, 3)
    weights[0, 1, 2] = 0.0  # (a zero weight does not hide the NaN: 0 * NaN)
    clean = hip.channel_project(data, center, weights, offset, clip=clip)
    data[0, 2, 1, 3, 40] = float("nan")
    out = hip.channel_project(data, center, weights, offset, clip=clip)
    assert bool(torch.isnan(out[0, :, 1, 3, 40]).all())
    out[0, :, 1, 3, 40] = clean[0, :, 1, 3, 40]
    assert torch.equal(out, clean)


def test_project_in_two_component_groups_is_the_two_groups_on_their_own(hip):
    data, center, weights, offset = _projection_inputs(12, 9, shape=(2, 3, 5, 67))
    whole = hip.channel_project(data, center, weights, offset, clip=False)
    first = hip.channel_project(data, center, weights[:, :8].contiguous(), offset[:, :8].contiguous(), clip=False)
    last = hip.channel_project(data, center, weights[:, 8:].contiguous(), offset[:, 8:].contiguous(), clip=False)
    assert torch.equal(whole, torch.cat([first, last], dim=1))
    expected = torch.einsum("bkc,bcxyz->bkxyz", weights.double(), (data - center[:, :, None, None, None]).double())
    expected = expected + offset.double()[:, :, None, None, None]
    magnitude = torch.einsum("bkc,bcxyz->bkxyz", weights.double().abs(), (data - center[:, :, None, None, None]).double().abs())
    bound = (12 + 4) * 2.0**-24 * (magnitude + offset.double().abs()[:, :, None, None, None])
    assert bool(((whole.double() - expected).abs() <= bound).all())


# -- the reference's own tests (tests/test_pca.py), on device batches -------------------------------------------------------
def test_reduces_channels(hip):
    result = tio.PCA(num_components=3)(cases.batch_of(tio, torch.rand(1, 8, 10, 10, 10), "cuda"))
    assert result.images["emb"].data.shape[1] == 3


def test_output_range(hip):
    result = tio.PCA(num_components=3, clip=True)(cases.batch_of(tio, torch.randn(1, 16, 10, 10, 10), "cuda"))
    assert result.images["emb"].data.min() >= 0.0
    assert result.images["emb"].data.max() <= 1.0


def test_too_few_channels_raises(hip):
    with pytest.raises(ValueError, match="channels"):
        tio.PCA(num_components=5)(cases.batch_of(tio, torch.rand(1, 2, 10, 10, 10), "cuda"))


def test_invalid_num_components_raises(hip):
    with pytest.raises(ValueError, match="num_components"):
        tio.PCA(num_components=0)


def test_no_whitening(hip):
    result = tio.PCA(num_components=3, whiten=False, normalize=False)(cases.batch_of(tio, torch.randn(1, 8, 10, 10, 10), "cuda"))
    assert result.images["emb"].data.shape[1] == 3


def test_history_and_untouched_input(hip):
    batch = cases.batch_of(tio, cases.make_input(4, (3, 4, 5), seed=1, batch=2), "cuda")
    before = batch.images["emb"].data.clone()
    out = tio.PCA(num_components=2)(batch)
    assert out.applied_transforms[-1].name == "PCA" and out.applied_transforms[-1].params == {}
    assert torch.equal(batch.images["emb"].data, before)


def test_one_voxel(hip):
    """``.std()`` of one value is NaN (the reference's ``first_std``); without it the centred voxel lands on ``-lo / (hi - lo)``."""
    data = torch.rand(2, 4, 1, 1, 1)
    out = tio.PCA(num_components=3, normalize=True)(cases.batch_of(tio, data, "cuda")).images["emb"].data
    assert out.shape == (2, 3, 1, 1, 1) and bool(torch.isnan(out).all())
    out = tio.PCA(num_components=3, normalize=False)(cases.batch_of(tio, data, "cuda")).images["emb"].data
    assert torch.equal(out.cpu(), torch.full((2, 3, 1, 1, 1), 0.5))
