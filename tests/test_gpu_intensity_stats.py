"""GPU: the intensity-statistics kernels and the four classes against the torch-CPU restatements of
``intensity_stats_cases.py`` (which the host tests hold against the reference's own outputs) and the golden file.

Selection, quantiles, the elementwise maps, Clamp and Mask are compared bit for bit; the moments within one float32 ulp of a
float64 evaluation — half an ulp for the single rounding plus the float64 accumulation error, which stays below a quarter
ulp under the three conditions the test asserts on its own inputs (n <= 2^17, |mean| >= 2^-10 mean|x|, |mean| <= 2^10 std).

Shapes: one voxel, two, 4020 elements in two channels (one block, a ragged tail), 103917 (26 blocks, a ragged tail); for the
elementwise kernels sizes that are no multiple of any vector group and two batch elements.
"""
from __future__ import annotations

import math
import os

import pytest
import torch

import intensity_stats_cases as cases
import torchio_amd as tio

pytestmark = pytest.mark.gpu

ONE, TWO, SMALL, BLOCKS = (1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (2, 2, 5, 6, 67), (1, 1, 33, 47, 67)
FRACTIONS = [0.0, 0.005, 0.5, 0.995, 1.0]
ALL_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]
MAP_SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intensity_stats_golden.pt")


def _ids(shape):
    return "x".join(map(str, shape))


def _randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def _typed(shape, seed, dtype):
    """Values every dtype holds differently: integers across the dtype's range (int64 beyond 2^24, where ``.float()``
    rounds), floats with a fraction (float64 with more bits than float32 keeps)."""
    generator = torch.Generator().manual_seed(seed)
    if dtype == torch.float64:
        return torch.randn(shape, generator=generator, dtype=torch.float64) * 50 + 10
    if dtype.is_floating_point:
        return (torch.randn(shape, generator=generator) * 50 + 10).to(dtype)
    if dtype == torch.int64:
        return torch.randint(-(2**40), 2**40, shape, generator=generator)
    info = torch.iinfo(dtype)
    return torch.randint(max(info.min, -40000), min(info.max, 40000) + 1, shape, generator=generator).to(dtype)


# -- selection -----------------------------------------------------------------------------------------------------------
def _selection_inputs():
    """name -> (data, mask): each a CPU tensor (mask may be None)."""
    n_small = 2 * 5 * 6 * 67
    half = _randn(BLOCKS, 3)
    half.view(-1)[: half.numel() // 2] = 0.0
    half.view(-1)[1::3] = 0.0
    steps = (1.0 + torch.randperm(n_small, generator=torch.Generator().manual_seed(4)).double() * 2.0**-23).float().view(1, *SMALL[1:])
    special = _randn(SMALL, 5)
    flat = special.view(-1)
    flat[:12] = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 1e-40, -1e-42, 1.4e-45, -1.4e-45, 3.4e38, -3.4e38, float("inf"), -0.0])
    nans = _randn(SMALL, 6)
    nans.view(-1)[[0, 17, 1000, 4019]] = float("nan")
    labels = cases.label_cases.label_field((1, 1, *SMALL[2:]), 1)[0].to(torch.int16)  # (1, I, J, K), values 0..3
    per_channel = torch.stack([labels[0] == 1, labels[0] >= 2])  # (2, I, J, K) bool
    one_voxel = torch.zeros(1, *SMALL[2:], dtype=torch.uint8)
    one_voxel[0, 3, 4, 50] = 9
    signed_zero = torch.where(labels > 1, 0.5, -0.0)  # float32 mask: -0.0 is outside, as `.bool()` has it
    small = _randn(SMALL, 1, 30.0, 5.0)
    return {
        "one_voxel_volume": (_randn(ONE, 0), None),
        "two_voxels": (_randn(TWO, 0), None),
        "small": (small, None),
        "many_blocks": (_randn(BLOCKS, 2, 100.0), None),
        "all_equal": (torch.full(SMALL, 3.25), None),
        "half_exact_zeros": (half, None),
        "duplicates": (torch.randint(0, 5, BLOCKS, generator=torch.Generator().manual_seed(7)).float(), None),
        "last_digit_only": (steps, None),
        "negatives_denormals_infinities": (special, None),
        "a_few_nans": (nans, None),
        "mask_one_voxel": (small, one_voxel),
        "mask_no_voxel": (small, torch.zeros(1, *SMALL[2:], dtype=torch.int16)),
        "mask_every_voxel": (small, torch.full((2, *SMALL[2:]), -3, dtype=torch.int8)),
        "mask_one_channel_int16": (small, labels),
        "mask_per_channel_bool": (small, per_channel),
        "mask_float_signed_zero": (small, signed_zero),
    }


SELECTION = _selection_inputs()


def _same_scalar(got: torch.Tensor, expected: torch.Tensor) -> bool:
    return bool(got == expected) or (bool(got.isnan()) and bool(expected.isnan()))


def _check_selection(hip, data, mask):
    values = cases.inside_values(data[0], mask)
    found = hip._order_statistics(data.cuda(), FRACTIONS, None if mask is None else mask.cuda())
    assert len(found) == len(FRACTIONS)
    for q, (lower, upper, count) in zip(FRACTIONS, found, strict=True):
        assert count == values.numel()
        if count == 0:
            assert bool(lower.isnan()) and bool(upper.isnan())
            continue
        expected_lower, expected_upper = cases.order_statistics(values, q)
        assert lower.dtype == torch.float32 and _same_scalar(lower, expected_lower) and _same_scalar(upper, expected_upper), (q, lower, expected_lower, upper, expected_upper)


@pytest.mark.parametrize("name", list(SELECTION))
def test_selection_is_kthvalue(hip, name):
    _check_selection(hip, *SELECTION[name])


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
def test_selection_reads_every_dtype(hip, dtype):
    data = _typed(SMALL, 8, dtype)
    _check_selection(hip, data, None)
    _check_selection(hip, data, SELECTION["mask_one_channel_int16"][1])


def test_selection_off_a_vector_boundary(hip):
    data = SELECTION["small"][0]
    flat = torch.cat([data.reshape(-1)[:1], data.reshape(-1)]).cuda()[1:].view(data.shape)  # one element off its allocation
    assert flat.data_ptr() % 16 == 4
    values = cases.inside_values(data[0], None)
    for q, (lower, upper, count) in zip(FRACTIONS, hip._order_statistics(flat, FRACTIONS), strict=True):
        expected = cases.order_statistics(values, q)
        assert count == values.numel() and bool(lower == expected[0]) and bool(upper == expected[1])


@pytest.mark.parametrize("name", ["two_voxels", "small", "many_blocks", "half_exact_zeros", "duplicates", "last_digit_only", "mask_one_channel_int16",
                                  "mask_per_channel_bool", "mask_one_voxel"])
def test_quantiles_are_the_reference_s(hip, name):
    data, mask = SELECTION[name]
    values = cases.inside_values(data[0], mask)
    fractions = [0.0, 0.005, 0.25, 0.5, 1.0 / 3.0, 0.995, 1.0]
    got = hip.intensity_quantiles(data.cuda(), fractions, None if mask is None else mask.cuda())
    assert got == [cases.compute_quantile(values, q) for q in fractions]


def test_quantiles_of_an_empty_mask_and_bad_fractions(hip):
    data, mask = SELECTION["mask_no_voxel"]
    values, count = hip.intensity_quantiles(data.cuda(), [0.1, 0.9], mask.cuda(), return_count=True)
    assert count == 0 and all(math.isnan(v) for v in values)
    with pytest.raises(ValueError, match="no element inside"):
        hip.intensity_quantiles(data.cuda(), [0.5], mask.cuda())
    with pytest.raises(ValueError, match="0 <= q <= 1"):
        hip.intensity_quantiles(data.cuda(), [1.5])
    with pytest.raises(ValueError, match="does not broadcast"):
        hip.intensity_quantiles(data.cuda(), [0.5], torch.zeros(3, *SMALL[2:], device="cuda"))


# -- moments -------------------------------------------------------------------------------------------------------------
MOMENT_INPUTS = {"normal_100_40": (40.0, 100.0), "normal_1000_3": (3.0, 1000.0), "uniform_0_1": None}


def _moment_data(kind, shape):
    seed = {TWO: 3, SMALL: 5, BLOCKS: 5}[shape]
    if MOMENT_INPUTS[kind] is None:
        return torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    return _randn(shape, seed, *MOMENT_INPUTS[kind])


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("shape", [TWO, SMALL, BLOCKS], ids=_ids)
@pytest.mark.parametrize("kind", list(MOMENT_INPUTS))
def test_moments_within_one_ulp_of_float64(hip, kind, shape, masked):
    data = _moment_data(kind, shape)
    mask = None
    if masked:
        mask = cases.label_cases.label_field((1, 1, *shape[2:]), 2)[0].to(torch.int16) if shape != TWO else torch.ones(1, 1, 1, 2, dtype=torch.int16)
    values = cases.inside_values(data[0], mask).double()
    exact_mean, exact_std = float(values.mean()), float(values.std())
    # the conditions under which float64 accumulation stays below a quarter of a float32 ulp
    assert 2 <= values.numel() <= 2**17
    assert abs(exact_mean) >= 2.0**-10 * float(values.abs().mean()) and abs(exact_mean) <= 2.0**10 * exact_std
    count, mean, std = hip.intensity_moments(data.cuda(), None if mask is None else mask.cuda())
    print(f"{kind} {shape} masked={masked}: mean off by {cases.ulps_off(mean, exact_mean):.3f} ulp, std by {cases.ulps_off(std, exact_std):.3f} ulp")
    assert count == values.numel()
    assert cases.ulps_off(mean, exact_mean) <= 1.0 and cases.ulps_off(std, exact_std) <= 1.0
    assert hip.intensity_moments(data.cuda(), None if mask is None else mask.cuda()) == (count, mean, std)  # the same bits again


def test_moments_edge_counts_and_dtypes(hip):
    data = SELECTION["small"][0]
    count, mean, std = hip.intensity_moments(data.cuda(), SELECTION["mask_one_voxel"][1].cuda())
    assert count == 2 and not math.isnan(std)  # the voxel, in both channels
    count, mean, std = hip.intensity_moments(_randn(ONE, 1, 1.0, 7.0).cuda())
    assert count == 1 and mean == float(_randn(ONE, 1, 1.0, 7.0)) and math.isnan(std)  # torch.std of one value
    count, mean, std = hip.intensity_moments(data.cuda(), SELECTION["mask_no_voxel"][1].cuda())
    assert count == 0 and math.isnan(mean) and math.isnan(std)
    count, mean, std = hip.intensity_moments(torch.full(SMALL, 3.25).cuda())
    assert (count, mean, std) == (4020, 3.25, 0.0)
    per_channel = SELECTION["mask_per_channel_bool"][1]
    for dtype in ALL_DTYPES:
        typed = _typed(SMALL, 9, dtype)
        values = cases.inside_values(typed[0], per_channel).double()
        count, mean, std = hip.intensity_moments(typed.cuda(), per_channel.cuda())
        assert count == values.numel() and cases.ulps_off(mean, float(values.mean())) <= 1.0 and cases.ulps_off(std, float(values.std())) <= 1.0, dtype


def _same_float(got: float, expected: float) -> bool:
    return got == expected or (math.isnan(got) and math.isnan(expected))


@pytest.mark.parametrize("shape", [SMALL, BLOCKS], ids=_ids)
@pytest.mark.parametrize("planted", [[float("nan")], [float("inf")], [-float("inf")], [float("inf"), float("inf")], [float("inf"), -float("inf")],
                                     [float("inf"), float("nan")]], ids=["nan", "inf", "-inf", "inf_inf", "inf_-inf", "inf_nan"])
def test_moments_of_non_finite_values_are_torch_s(hip, shape, planted):
    """``torch.mean`` / ``torch.std`` of values with a NaN or an infinity: a NaN deviation, a mean of NaN or of the infinity.  The
    planted values sit at a thread's first element (index 0), inside a vector and in the ragged tail."""
    data = _randn(shape, 13, 40.0, 100.0)
    flat = data[0].view(-1)
    for value, index in zip(planted, (0, flat.numel() - 1), strict=False):
        flat[index] = value
    flat[flat.numel() // 2 + 1] = planted[0]
    values = data[0].reshape(-1)
    count, mean, std = hip.intensity_moments(data.cuda())
    assert count == values.numel() and _same_float(mean, float(values.mean())) and _same_float(std, float(values.std())), (mean, std)
    assert math.isnan(std)
    labels = cases.label_cases.label_field((1, 1, *shape[2:]), 2)[0].to(torch.int16)
    labels.view(-1)[0] = 1  # the planted first element is inside
    inside = cases.inside_values(data[0], labels)
    count, mean, std = hip.intensity_moments(data.cuda(), labels.cuda())
    assert count == inside.numel() and _same_float(mean, float(inside.mean())) and _same_float(std, float(inside.std())), (mean, std)


def test_standardize_of_an_image_with_a_nan_is_all_nan_like_the_reference_s(hip):
    image = cases.golden_image().clone()
    image[0, 1, 2, 3, 4] = float("nan")
    out = tio.Standardize()(_batch(image))  # no "deviation is zero" error: `nan == 0` is false (standardize.py:91)
    mean, std = out.applied_transforms[-1].params["stats"]["t1"]
    assert math.isnan(mean) and math.isnan(std) and bool(out.images["t1"].data.isnan().all())


def test_engine_methods_refuse_autograd_and_host_tensors(hip):
    leaf = torch.zeros(1, 1, 2, 2, 2, device="cuda", requires_grad=True)
    for call in (hip.intensity_moments, lambda x: hip.intensity_quantiles(x, [0.5]), lambda x: hip.intensity_map(x, "sub_div", in_min=0.0, in_range=1.0),
                 lambda x: hip.clamp(x, 0.0), lambda x: hip.mask_where(x, torch.ones(1, 2, 2, 2, device="cuda"), 0.0)):
        with pytest.raises(tio.ops.EngineError, match="no backward"):
            call(leaf)
        with pytest.raises(tio.ops.EngineError, match="tensor on cpu"):
            call(torch.zeros(1, 1, 2, 2, 2))


# -- map, clamp, mask ----------------------------------------------------------------------------------------------------
def _with_specials(data):
    if data.dtype.is_floating_point and data.numel() > 8:
        data.view(-1)[[1, 5, 7]] = torch.tensor([float("nan"), float("inf"), -float("inf")], dtype=data.dtype)
    return data


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=_ids)
def test_map_every_mode_scalar_and_per_element(hip, shape, dtype):
    data = _with_specials(_typed(shape, 10, dtype))
    on_device = data.cuda()
    in_min, in_max = -17.3, 61.9
    in_range = in_max - in_min
    for out_min, out_max in ((-1.0, 1.0), (0.1, 254.7)):
        got = hip.intensity_map(on_device, "rescale_clip", in_min=in_min, in_max=in_max, in_range=in_range, out_min=out_min, out_range=out_max - out_min)
        assert cases.same(got.cpu(), cases.normalize(data, in_min, in_max, out_min, out_max))
        got = hip.intensity_map(on_device, "rescale", in_min=in_min, in_range=in_range, out_min=out_min, out_range=out_max - out_min)
        assert cases.same(got.cpu(), cases.normalize_inverse(data, in_min, in_max, out_min, out_max))
    lows, highs = [0.1, -0.3][: shape[0]], [0.7, 0.9][: shape[0]]
    low_t = torch.tensor(lows, dtype=torch.float32)
    span_t = torch.tensor(highs, dtype=torch.float32) - low_t
    got = hip.intensity_map(on_device, "rescale_clip", in_min=in_min, in_max=in_max, in_range=in_range, out_min=low_t.cuda(), out_range=span_t.cuda())
    assert cases.same(got.cpu(), cases.normalize(data, in_min, in_max, lows, highs))
    highs = [0.1, 0.9][: shape[0]]  # element 0: out_min == out_max, it stays
    span_t = torch.tensor(highs, dtype=torch.float32) - low_t
    got = hip.intensity_map(on_device, "rescale", in_min=in_min, in_range=in_range, out_min=low_t.cuda(), out_range=span_t.cuda())
    assert cases.same(got.cpu(), cases.normalize_inverse(data, in_min, in_max, lows, highs))
    mean, std = 20.897739410400391, 40.169807434082031
    assert cases.same(hip.intensity_map(on_device, "sub_div", in_min=mean, in_range=std).cpu(), cases.standardize(data, mean, std))
    assert cases.same(hip.intensity_map(on_device, "mul_add", in_min=mean, in_range=std).cpu(), cases.standardize_inverse(data, mean, std))


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=_ids)
def test_clamp_is_torch_clamp(hip, shape, dtype):
    data = _with_specials(_typed(shape, 11, dtype))
    for out_min, out_max in ((0.1, None), (None, 61.3), (-17.25, 40.5), (3.0, 3.0)):
        got = hip.clamp(data.cuda(), out_min, out_max)
        assert cases.same(got.cpu(), cases.clamp(data, out_min, out_max)), (out_min, out_max)
    with pytest.raises(RuntimeError, match="At least one"):
        hip.clamp(data.cuda())


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
@pytest.mark.parametrize("shape", MAP_SHAPES + [(2, 2, 3, 5, 67)], ids=_ids)
def test_mask_where_is_torch_where(hip, shape, dtype):
    data = _with_specials(_typed(shape, 12, dtype))
    labels = cases.label_cases.label_field((1, 1, *shape[2:]), 3)[0].to(torch.int16)  # (1, I, J, K)
    masks = [labels, labels > 1, torch.where(labels > 0, 2.5, -0.0), torch.cat([labels == 1, labels != 2])[: shape[1]]]
    for mask in masks:
        for outside in (0.0, -7.3):
            got = hip.mask_where(data.cuda(), mask.cuda(), outside)
            assert cases.same(got.cpu(), cases.mask_where(data, mask, outside)), (mask.dtype, outside)


# -- the classes ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c[0] != "Standardize"])
def test_golden_cases_bit_for_bit(hip, golden, name):
    entry = golden["cases"][name]
    out, params, history_name = cases.run_case(tio, name, "cuda")
    assert history_name == entry["name"] and params == entry["params"]
    assert torch.equal(out.images["t1"].data.cpu(), entry["out"]) and torch.equal(out.images["seg"].data.cpu(), golden["labels"])
    if "restored" in entry:
        assert torch.equal(tio.apply_inverse_transform(out).images["t1"].data.cpu(), entry["restored"])


@pytest.mark.parametrize("name", ["standardize_plain", "standardize_masked"])
def test_golden_standardize(hip, golden, name):
    entry = golden["cases"][name]
    out, params, history_name = cases.run_case(tio, name, "cuda")
    assert history_name == "Standardize" and list(params) == ["stats"] and list(params["stats"]) == ["t1"]
    mean, std = params["stats"]["t1"]
    golden_mean, golden_std = entry["params"]["stats"]["t1"]
    # each within one float32 ulp of the float64 value, so within two of each other
    assert cases.ulps_off(mean, golden_mean) <= 2.0 and cases.ulps_off(std, golden_std) <= 2.0
    data = out.images["t1"].data.cpu()
    assert torch.equal(data, cases.standardize(cases.golden_image(), mean, std))
    assert torch.allclose(data, entry["out"], rtol=0, atol=1e-5)
    if "restored" in entry:
        assert torch.equal(tio.apply_inverse_transform(out).images["t1"].data.cpu(), cases.standardize_inverse(data, mean, std))


def test_zero_range_element_stays_in_the_inverse(hip, golden):
    subjects = [tio.Subject(t1=tio.ScalarImage(cases.golden_image()[b].clone())) for b in range(2)]
    batch = tio.SubjectsBatch.from_subjects(subjects).to("cuda")
    batch.applied_transforms.append(tio.AppliedTransform("Normalize", dict(cases.ZERO_RANGE_INVERSE)))
    assert torch.equal(tio.apply_inverse_transform(batch).images["t1"].data.cpu(), golden["zero_range_restored"])


def _batch(image, labels=None, **more):
    subjects = []
    for b in range(image.shape[0]):
        entries = {"t1": tio.ScalarImage(image[b].clone())}
        if labels is not None:
            entries["seg"] = tio.LabelMap(labels[b].clone())
        entries.update({key: tio.ScalarImage(value[b].clone()) for key, value in more.items()})
        subjects.append(tio.Subject(**entries))
    return tio.SubjectsBatch.from_subjects(subjects).to("cuda")


def test_warnings_and_the_zero_deviation_error(hip):
    image, labels = cases.golden_image(), cases.golden_labels()
    constant = torch.full_like(image, 4.0)
    with pytest.warns(RuntimeWarning, match='Cannot rescale "t1": input range is zero'):
        out = tio.Normalize()(_batch(constant))
    assert torch.equal(out.images["t1"].data.cpu(), constant)  # skipped
    with pytest.raises(RuntimeError, match='Standard deviation is zero for masked values in "t1"'):
        tio.Standardize()(_batch(constant))
    nothing = torch.zeros_like(labels)
    with pytest.warns(RuntimeWarning, match='Cannot compute percentiles for "t1": mask is empty'):
        out = tio.Normalize(masking_method="seg", per_instance=False)(_batch(image, nothing))
    low, high = cases.percentile_range(image[0], None, 0.0, 100.0)
    assert out.applied_transforms[-1].params["in_ranges"] == {"t1": (low, high)}
    assert torch.equal(out.images["t1"].data.cpu(), cases.normalize(image, low, high, -1.0, 1.0))
    with pytest.warns(RuntimeWarning, match='Mask is empty for "t1". Using all voxels'):
        out = tio.Standardize(masking_method="seg")(_batch(image, nothing))
    mean, std = out.applied_transforms[-1].params["stats"]["t1"]
    assert cases.ulps_off(mean, float(image[0].double().mean())) <= 1.0 and cases.ulps_off(std, float(image[0].double().std())) <= 1.0


def test_include_exclude_and_label_maps_pass(hip):
    image, labels = cases.golden_image(), cases.golden_labels()
    other = image * 0.5 - 3.0
    out = tio.Clamp(out_min=0.0, include=["t1"])(_batch(image, labels, t2=other))
    assert torch.equal(out.images["t1"].data.cpu(), image.clamp(min=0.0)) and torch.equal(out.images["t2"].data.cpu(), other)
    assert out.applied_transforms[-1].include == ["t1"] and torch.equal(out.images["seg"].data.cpu(), labels)
    out = tio.Standardize(exclude=["t1"])(_batch(image, labels, t2=other))
    assert list(out.applied_transforms[-1].params["stats"]) == ["t2"] and torch.equal(out.images["t1"].data.cpu(), image)
    assert not torch.equal(out.images["t2"].data.cpu(), other) and out.images["seg"].data.dtype == torch.int16
    out = tio.Mask(masking_method=cases.above_twenty, outside_value=1.5, exclude=["t2"])(_batch(image, labels, t2=other))
    assert torch.equal(out.images["t1"].data.cpu(), torch.where(cases.above_twenty(image[0]).expand_as(image), image, 1.5))
    assert torch.equal(out.images["t2"].data.cpu(), other)


def test_integer_images_become_float32(hip):
    image = torch.randint(-1000, 2000, cases.GOLDEN_SHAPE, generator=torch.Generator().manual_seed(1), dtype=torch.int16)
    out = tio.Clamp(out_min=-100.5, out_max=900)(_batch(image))
    assert cases.same(out.images["t1"].data.cpu(), image.clamp(min=-100.5, max=900))
    out = tio.Normalize(in_min=-1000.0, in_max=1000.0, out_min=0.0, out_max=1.0, per_instance=False)(_batch(image))
    assert torch.equal(out.images["t1"].data.cpu(), cases.normalize(image, -1000.0, 1000.0, 0.0, 1.0))
    out = tio.Normalize(percentile_low=0.5, percentile_high=99.5, per_instance=False)(_batch(image))
    low, high = cases.percentile_range(image[0], None, 0.5, 99.5)
    assert out.applied_transforms[-1].params["in_ranges"] == {"t1": (low, high)}


def test_compose_with_normalize_in_front_of_affine_and_behind_it(hip):
    image, labels = cases.golden_image(), cases.golden_labels()

    def affine():
        return tio.Affine(degrees=(-20, 20), translation=(-2, 2))

    def normalize():
        return tio.Normalize(percentile_low=1.0, percentile_high=99.0, per_instance=False)

    for order in ("front", "behind"):
        first, second = (normalize, affine) if order == "front" else (affine, normalize)
        torch.manual_seed(31)
        composed = tio.Compose([first(), second()])(_batch(image, labels))
        torch.manual_seed(31)
        halfway = first()(_batch(image, labels))
        stepwise = second()(halfway)
        assert [record.name for record in composed.applied_transforms] == [type(first()).__name__, type(second()).__name__]
        assert [record.params for record in composed.applied_transforms] == [record.params for record in stepwise.applied_transforms]
        assert torch.equal(composed.images["t1"].data, stepwise.images["t1"].data) and torch.equal(composed.images["seg"].data, stepwise.images["seg"].data)
        if order == "behind":
            # the input range was read from what the resampling wrote, not from the input: parameters are not drawn ahead
            expected = tuple(hip.intensity_quantiles(halfway.images["t1"].data, [0.01, 0.99]))
            assert composed.applied_transforms[-1].params["in_ranges"]["t1"] == expected
            assert expected != tuple(hip.intensity_quantiles(_batch(image).images["t1"].data, [0.01, 0.99]))
            assert float(composed.images["t1"].data.min()) == -1.0 and float(composed.images["t1"].data.max()) == 1.0
