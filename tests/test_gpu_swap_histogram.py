"""GPU: ``tio_swap_patches``, ``tio_intensity_multi_quantiles``, ``tio_histogram_standardize`` and the two classes against the
torch-CPU restatements of ``swap_histogram_cases.py`` (which the host tests hold against the reference's own outputs) and the
golden file.  Everything is compared bit for bit: Swap moves elements, the percentiles are compared as float64 bits with
``np.percentile``, the map is a sequence of separately rounded float32 operations.

Shapes: the volumes of the issue's Swap geometries (all pairs overlapping; K = 67, no multiple of anything); for the
selection one voxel, two, 101 (every default percentile on a data value), 4020 in two channels (one block, a ragged tail)
and 103917 (26 blocks).
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import swap_histogram_cases as cases
import torchio_amd as tio
from torchio_amd import ops
from torchio_amd.transforms import histogram_standardization as module

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swap_histogram_golden.pt")
Q = cases.DEFAULT_QUANTILES


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


# -- Swap: the engine against the sequential loop ---------------------------------------------------------------------------
def _check_swap(hip, data, locations, patch):
    on_device = data.cuda()
    before = on_device.clone()
    out = hip.swap_patches(on_device, locations, patch)
    assert torch.equal(on_device, before), "the input is unchanged"
    expected = cases.swap_sequential(data, locations, patch)
    assert out.dtype == data.dtype and out.shape == data.shape
    assert torch.equal(out.cpu().view(torch.uint8), expected.view(torch.uint8))
    return out


OVERLAPPING = cases.random_locations((5, 6, 7), (3, 4, 4), 30, 1)
SWAP_GEOMETRIES = {
    "all_pairs_overlap": ((1, 1, 5, 6, 7), (3, 4, 4), OVERLAPPING),
    "forty_swaps_heavy_overlap": ((1, 1, 9, 10, 67), (3, 4, 5), cases.random_locations((9, 10, 67), (3, 4, 5), 40, 2)),
    "a_equals_b": ((1, 1, 5, 6, 7), (3, 4, 4), [((1, 1, 2), (1, 1, 2)), ((0, 2, 3), (0, 2, 3)), ((1, 1, 2), (2, 2, 3))]),
    "no_swaps": ((2, 1, 5, 6, 7), (3, 4, 4), []),
    "three_hundred_swaps": ((1, 1, 9, 10, 67), (2, 3, 9), cases.random_locations((9, 10, 67), (2, 3, 9), 300, 3)),
    "patch_is_the_volume": ((1, 2, 5, 6, 7), (5, 6, 7), [((0, 0, 0), (0, 0, 0))] * 3),
    "one_voxel_patches": ((1, 1, 5, 6, 7), (1, 1, 1), cases.random_locations((5, 6, 7), (1, 1, 1), 50, 4)),
    "two_channels": ((1, 2, 9, 10, 67), (3, 4, 5), cases.random_locations((9, 10, 67), (3, 4, 5), 12, 5)),
    "two_elements_shared": ((2, 1, 9, 10, 67), (3, 4, 5), cases.random_locations((9, 10, 67), (3, 4, 5), 12, 6)),
    "per_instance_7_0_3": ((3, 2, 5, 6, 7), (3, 4, 4), [cases.random_locations((5, 6, 7), (3, 4, 4), 7, 7), [], cases.random_locations((5, 6, 7), (3, 4, 4), 3, 8)]),
    "per_instance_all_empty": ((2, 1, 5, 6, 7), (3, 4, 4), [[], []]),
}


@pytest.mark.parametrize("name", list(SWAP_GEOMETRIES))
def test_swap_is_the_sequential_loop(hip, name):
    shape, patch, locations = SWAP_GEOMETRIES[name]
    _check_swap(hip, cases.randn(shape, 11), locations, patch)


def test_swap_geometries_overlap_as_intended():
    assert all(all(abs(a[d] - b[d]) < (3, 4, 4)[d] for d in range(3)) for a, b in OVERLAPPING)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.float64], ids=str)
def test_swap_moves_elements_of_every_size(hip, dtype):
    shape, patch, locations = SWAP_GEOMETRIES["forty_swaps_heavy_overlap"]
    data = cases.typed(shape, 12, dtype)
    _check_swap(hip, data, locations, patch)
    _check_swap(hip, cases.typed((3, 2, 5, 6, 7), 13, dtype), SWAP_GEOMETRIES["per_instance_7_0_3"][2], (3, 4, 4))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32, torch.float64], ids=str)
def test_swap_one_element_off_a_vector_boundary(hip, dtype):
    shape, patch, locations = SWAP_GEOMETRIES["two_channels"]
    data = cases.typed(shape, 14, dtype)
    flat = torch.cat([data.reshape(-1)[:1], data.reshape(-1)]).cuda()[1:].view(shape)
    assert flat.data_ptr() % 16 == data.element_size()
    out = hip.swap_patches(flat, locations, patch)
    assert torch.equal(out.cpu(), cases.swap_sequential(data, locations, patch))


def test_swap_refusals(hip):
    data = cases.randn((1, 1, 5, 6, 7), 15).cuda()
    with pytest.raises(ValueError, match="cannot be larger"):
        hip.swap_patches(data, [], (3, 7, 4))
    with pytest.raises(ValueError, match="outside"):
        hip.swap_patches(data, [((0, 0, 0), (3, 2, 3))], (3, 4, 4))
    with pytest.raises(ValueError, match="outside"):
        hip.swap_patches(data, [((0, -1, 0), (1, 1, 1))], (3, 4, 4))
    with pytest.raises(ValueError, match="location lists"):
        hip.swap_patches(data, [[], []], (3, 4, 4))
    with pytest.raises(ops.EngineError, match="runs on cuda tensors"):
        hip.swap_patches(data.cpu(), [], (3, 4, 4))
    with pytest.raises(ops.EngineError, match="no backward"):
        hip.swap_patches(data.clone().requires_grad_(), [], (3, 4, 4))
    origins = torch.zeros(6, dtype=torch.int32, device="cuda")
    counts = torch.ones(1, dtype=torch.int32, device="cuda")
    status = hip._fn["swap_patches"](data.data_ptr(), data.data_ptr(), 4, 1, 1, ops._i32x3((5, 6, 7)), ops._i32x3((3, 4, 4)), origins.data_ptr(),
                                     counts.data_ptr(), 1, 1, None)
    assert status == -1 and b"overlaps" in hip._fn["last_error"]()  # y aliasing x: refused, nothing launched


# -- the percentiles of every element against np.percentile -------------------------------------------------------------------
def _check_percentiles(hip, data, mask, quantiles=Q):
    values, counts = hip.intensity_multi_quantiles(data.cuda(), quantiles, None if mask is None else mask.cuda())
    assert values.dtype == torch.float64 and values.shape == (data.shape[0], len(quantiles)) and values.is_cuda
    assert counts.dtype == torch.int64 and counts.shape == (data.shape[0],) and counts.is_cuda
    values, counts = values.cpu().numpy(), counts.tolist()
    for b in range(data.shape[0]):
        inside = cases.inside_values(data[b], mask)
        expected = cases.percentiles(inside, quantiles)
        print(b, inside.numel(), values[b], expected)
        assert counts[b] == inside.numel()
        assert cases.same_bits64(values[b], expected), (b, values[b], expected)


@pytest.mark.parametrize("name", list(cases.selection_inputs()))
def test_percentiles_are_numpys(hip, name):
    _check_percentiles(hip, *cases.selection_inputs()[name])


def test_percentile_inputs_are_what_they_claim():
    inputs = cases.selection_inputs()
    n = inputs["ranks_on_data_values"][0].numel()
    assert n == 101 and all(float((100.0 * q) / 100.0 * (n - 1)).is_integer() for q in Q)
    assert int(inputs["a_few_nans"][0].isnan().sum()) == 4 and int(inputs["mask_no_voxel"][1].bool().sum()) == 0
    assert inputs["many_blocks"][0].numel() == 103917 and inputs["small"][0].numel() == 4020 and inputs["two_elements"][0].shape[0] == 2


@pytest.mark.parametrize("dtype", cases.ALL_DTYPES, ids=str)
def test_percentiles_read_every_dtype(hip, dtype):
    data = cases.typed((2, *cases.SMALL[1:]), 8, dtype)
    _check_percentiles(hip, data, None)
    _check_percentiles(hip, data, cases.selection_inputs()["mask_one_channel_int16"][1])


def test_percentiles_other_fractions(hip):
    data = cases.selection_inputs()["two_elements"][0]
    _check_percentiles(hip, data, None, [0.0, 1.0])
    _check_percentiles(hip, data, None, [0.5])
    _check_percentiles(hip, data, None, [k / 31 for k in range(32)])
    _check_percentiles(hip, data, None, cases.WIDE_QUANTILES)
    with pytest.raises(ValueError, match="fractions"):
        hip.intensity_multi_quantiles(data.cuda(), [0.5] * 33)
    with pytest.raises(ValueError, match="0 <= q <= 1"):
        hip.intensity_multi_quantiles(data.cuda(), [0.5, 1.5])


# -- the transform against the restatement ------------------------------------------------------------------------------------
def _check_standardize(hip, data, quantiles=Q):
    landmarks = cases.landmarks_for(quantiles)
    out = hip.histogram_standardize(data.cuda(), landmarks, quantiles)
    expected = cases.standardize(data, landmarks, quantiles)
    assert out.dtype == data.dtype and cases.same(out.cpu(), expected)
    return out.cpu()


STANDARDIZE_INPUTS = ["one_voxel_volume", "two_voxels", "ranks_on_data_values", "small", "many_blocks", "all_equal", "half_exact_zeros", "duplicates",
                      "last_digit_only", "two_elements"]


@pytest.mark.parametrize("name", STANDARDIZE_INPUTS)
def test_standardize_is_the_restatement(hip, name):
    _check_standardize(hip, cases.selection_inputs()[name][0])
    _check_standardize(hip, cases.selection_inputs()[name][0], cases.WIDE_QUANTILES)


def test_standardize_flat_segments():
    """What the inputs are for: all segments flat, leading flat segments, a segment narrower than 1e-5 but not empty."""
    inputs = cases.selection_inputs()
    widths = np.diff(cases.percentiles(inputs["half_exact_zeros"][0], Q))
    assert np.any(widths == 0) and widths[0] > 0 and widths[-1] > 0  # flat in the middle
    found = cases.percentiles(_leading_zeros(), Q)
    assert found[0] == found[5] == 0.0 and found[-1] > 0.0
    assert np.all(np.diff(cases.percentiles(inputs["all_equal"][0], Q)) == 0)
    widths = np.diff(cases.percentiles(inputs["last_digit_only"][0], Q).astype(np.float32))
    assert np.all(widths > 0)
    close = _close_percentiles()
    widths = np.diff(cases.percentiles(close, Q).astype(np.float32))
    assert np.any((widths > 0) & (widths < 1e-5)) and np.any(widths > 1e-5)


def _leading_zeros():
    """Half exact zeros and nothing below them: the leading segments are flat."""
    return cases.selection_inputs()["half_exact_zeros"][0].abs()


def _close_percentiles():
    """4020 values around 1e-3 spaced 2^-33 apart (adjacent percentiles a few 1e-6 apart), then a wide upper tail."""
    data = (1e-3 + torch.randperm(4020, generator=torch.Generator().manual_seed(21)).double() * 2.0**-33).float()
    data[data > torch.quantile(data, 0.85)] += 5.0
    return data.view(cases.SMALL)


def test_standardize_close_percentiles_and_leading_flat_segments(hip):
    _check_standardize(hip, _close_percentiles())
    _check_standardize(hip, _leading_zeros())


def test_standardize_infinities_and_nan(hip):
    data = cases.selection_inputs()["small"][0].clone()
    data.view(-1)[[5, 700]] = float("inf")
    data.view(-1)[[6, 4000]] = -float("inf")
    out = _check_standardize(hip, data)
    assert bool(out.view(-1)[5].isinf()) and int(out.isnan().sum()) == 0
    data.view(-1)[99] = float("nan")
    assert bool(_check_standardize(hip, data).isnan().all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int16, torch.int32], ids=str)
def test_standardize_keeps_the_dtype(hip, dtype):
    base = cases.randn((2, 2, 5, 6, 67), 22, 40.0, 20.0)  # results stay within about [-40, 140]: in range for every dtype here
    data = base.to(dtype) if dtype.is_floating_point else base.round().to(dtype)
    _check_standardize(hip, data)


def test_standardize_builds_a_table_per_element(hip):
    data = cases.selection_inputs()["two_elements"][0]
    out = _check_standardize(hip, data)
    alone = [_check_standardize(hip, data[b : b + 1]) for b in range(2)]
    assert torch.equal(out[0], alone[0][0]) and torch.equal(out[1], alone[1][0])
    swapped = _check_standardize(hip, data.flip(0))
    assert torch.equal(swapped[0], out[1]) and not torch.equal(swapped[0], out[0])


def test_standardize_enqueues_without_synchronising(hip, monkeypatch):
    """No read-back in ``Engine.histogram_standardize``: under ``set_sync_debug_mode("error")`` a synchronising call raises; and,
    whatever that mode catches on this build, no tensor is taken to the host."""
    data = cases.selection_inputs()["small"][0].cuda()
    landmarks = cases.landmarks_for(Q).cuda()
    hip.histogram_standardize(data, landmarks, Q)  # (loads everything once)
    torch.cuda.synchronize()

    def refuse(*args, **kwargs):
        raise AssertionError("a tensor was read back")

    with monkeypatch.context() as patch:
        for name in ("cpu", "item", "tolist", "numpy"):
            patch.setattr(torch.Tensor, name, refuse)
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = hip.histogram_standardize(data, landmarks, Q)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert cases.same(out.cpu(), cases.standardize(data.cpu(), landmarks.cpu(), Q))


# -- the classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SWAP_CASES))
def test_swap_golden_cases(golden, name):
    out, params, history_name, messages = cases.run_case(tio, name, "cuda")
    entry = golden[name]
    assert params == entry["params"] and history_name == entry["name"] == "Swap" and messages == entry["warnings"]
    for key, expected in entry["out"].items():
        assert out.images[key].data.is_cuda and cases.same(out.images[key].data.cpu(), expected)


@pytest.mark.parametrize("name", list(cases.HISTOGRAM_CASES))
def test_histogram_standardization_golden_cases(golden, name):
    out, params, history_name, messages = cases.run_case(tio, name, "cuda")
    entry = golden[name]
    assert params == entry["params"] == {} and history_name == entry["name"] and messages == entry["warnings"] == []
    for key, expected in entry["out"].items():
        assert cases.same(out.images[key].data.cpu(), expected)


@pytest.mark.parametrize("name", list(cases.LANDMARK_CASES))
def test_landmark_training_golden_cases(golden, name):
    landmarks = cases.run_case(tio, name, "cuda")
    assert landmarks.dtype == torch.float32 and landmarks.device.type == "cpu" and torch.equal(landmarks, golden[name]["landmarks"])


def test_landmark_training_takes_host_images_and_custom_quantiles(hip):
    images = [tio.ScalarImage(image) for image in cases.training_images()]
    quantiles = [0.05, 0.5, 0.95]
    got = module.compute_histogram_landmarks(images, quantiles=quantiles, cutoff=(0.05, 0.95))
    assert torch.equal(got, cases.train_landmarks(cases.training_images(), quantiles))


def test_swap_in_a_compose_equals_stepwise(hip):
    image = cases.golden_image(2, (9, 10, 13))
    batch = cases._batch(tio, {"t1": (tio.ScalarImage, image)}, "cuda")
    swap, affine = tio.Swap(patch_size=3, num_iterations=7), tio.Affine(degrees=10.0)
    torch.manual_seed(5)
    composed = tio.Compose([swap, affine])(batch)
    torch.manual_seed(5)
    stepwise = affine(swap(batch))
    assert torch.equal(composed.images["t1"].data, stepwise.images["t1"].data)
    names = [record.name for record in composed.applied_transforms]
    assert "Swap" in names and composed.applied_transforms[names.index("Swap")].params == stepwise.applied_transforms[0].params
    assert len(stepwise.applied_transforms[0].params["locations"]) == 2
