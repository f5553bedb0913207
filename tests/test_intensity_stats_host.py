"""Normalize / Standardize / Clamp / Mask without a GPU: argument checks of the new entry points (nothing is launched), the
four classes' constructors / parameters / inverses / errors raised before any compute, and the golden file (the reference's
own outputs, ``tests/golden/make_golden_intensity_stats.py``) against the torch-CPU restatements of
``intensity_stats_cases.py`` that the GPU tests compare the engine with."""
from __future__ import annotations

import ctypes
import json
import os

import pytest
import torch

import intensity_stats_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.transforms import normalize as normalize_module

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intensity_stats_golden.pt")
SOME = ctypes.c_void_p(4096)  # a non-null, 16-byte aligned pointer no check dereferences
OTHER = ctypes.c_void_p(8192)
NEW = ("intensity_stats_workspace_bytes", "intensity_moments", "intensity_quantiles", "intensity_map", "intensity_clamp", "intensity_mask")


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def test_entry_points_are_hip_only_and_the_abi_number_stays(fn):
    assert _abi.ABI_VERSION >= 17 and fn["abi_version"]() == _abi.ABI_VERSION  # (these entry points: since 17)
    for name in NEW:
        assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
    assert (_abi.MAP_RESCALE_CLIP, _abi.MAP_RESCALE, _abi.MAP_SUB_DIV, _abi.MAP_MUL_ADD) == (0, 1, 2, 3)


def test_workspace_size(fn):
    size = fn["intensity_stats_workspace_bytes"]()
    assert size >= 4 * 2048 * 8 and size >= 1024 * 24 and size < (1 << 20)  # four 64-bit histograms; the moments' partials


@pytest.mark.parametrize("name", ["intensity_moments", "intensity_quantiles"])
def test_statistics_refuse_bad_arguments(fn, name):
    call = fn[name]
    size = fn["intensity_stats_workspace_bytes"]()
    fractions = (ctypes.c_double * 2)(0.25, 0.75)
    extra = (fractions, 2) if name == "intensity_quantiles" else ()

    def run(x=SOME, dtype=_abi.F32, channels=2, spatial=64, mask=None, mask_dtype=0, mask_channels=0, record=OTHER, workspace=SOME, nbytes=size, extra=extra):
        return call(x, dtype, channels, spatial, mask, mask_dtype, mask_channels, *extra, record, workspace, nbytes, None)

    assert run(x=None) == -1 and b"null" in fn["last_error"]()
    assert run(record=None) == -1 and b"null" in fn["last_error"]()
    assert run(workspace=None) == -1
    assert run(channels=-1) == -1 and b"negative" in fn["last_error"]()
    assert run(spatial=-5) == -1 and b"negative" in fn["last_error"]()
    assert run(dtype=9) == -2 and run(dtype=-1) == -2 and b"dtype" in fn["last_error"]()
    assert run(mask=SOME, mask_dtype=33, mask_channels=1) == -2
    assert run(mask=SOME, mask_dtype=_abi.U8, mask_channels=3) == -1 and b"mask channels" in fn["last_error"]()
    assert run(mask=SOME, mask_dtype=_abi.I16, mask_channels=0) == -1
    assert run(nbytes=size - 1) == -1 and b"too small" in fn["last_error"]()
    assert run(workspace=ctypes.c_void_p(4100)) == -1 and b"aligned" in fn["last_error"]()
    assert run(channels=4, spatial=1 << 39) == -5
    if name == "intensity_quantiles":
        for bad in (-0.001, 1.0001, float("nan"), float("inf")):
            assert run(extra=((ctypes.c_double * 2)(0.5, bad), 2)) == -1 and b"outside [0, 1]" in fn["last_error"]()
        assert run(extra=(None, 1)) == -1
        assert run(extra=(fractions, 0)) == -1 and run(extra=(fractions, 3)) == -1 and b"fractions" in fn["last_error"]()


def test_map_refuses_bad_arguments(fn):
    call = fn["intensity_map"]

    def run(x=SOME, y=OTHER, dtype=_abi.I16, batch=2, per_element=64, mode=_abi.MAP_RESCALE_CLIP, low=None, span=None):
        return call(x, y, dtype, batch, per_element, mode, 0.0, 1.0, 1.0, 0.0, 1.0, low, span, None)

    assert run(x=None) == -1 and b"null" in fn["last_error"]()
    assert run(y=None) == -1
    assert run(batch=-1) == -1 and run(per_element=-1) == -1 and b"negative" in fn["last_error"]()
    assert run(dtype=12) == -2
    assert run(mode=4) == -1 and run(mode=-1) == -1 and b"mode" in fn["last_error"]()
    assert run(low=SOME) == -1 and run(span=SOME) == -1 and b"together" in fn["last_error"]()
    assert run(mode=_abi.MAP_SUB_DIV, low=SOME, span=SOME) == -1 and run(mode=_abi.MAP_MUL_ADD, low=SOME, span=SOME) == -1
    assert run(batch=8, per_element=1 << 38) == -5
    assert run(x=None, y=None, batch=0) == 0 and run(x=None, y=None, per_element=0) == 0  # nothing to do


def test_clamp_refuses_bad_arguments(fn):
    call = fn["intensity_clamp"]
    assert call(None, OTHER, _abi.F32, 8, 1, 0.0, 0, 0.0, None) == -1 and b"null" in fn["last_error"]()
    assert call(SOME, None, _abi.F32, 8, 1, 0.0, 0, 0.0, None) == -1
    assert call(SOME, OTHER, _abi.F32, -8, 1, 0.0, 0, 0.0, None) == -1 and b"negative" in fn["last_error"]()
    assert call(SOME, OTHER, _abi.F32, 8, 0, 0.0, 0, 0.0, None) == -1 and b"at least one" in fn["last_error"]()
    assert call(SOME, OTHER, _abi.F32, 8, 1, float("nan"), 0, 0.0, None) == -1 and b"NaN" in fn["last_error"]()
    assert call(SOME, OTHER, 9, 8, 1, 0.0, 0, 0.0, None) == -2
    assert call(None, None, _abi.F32, 0, 1, 0.0, 0, 0.0, None) == 0


def test_mask_refuses_bad_arguments(fn):
    call = fn["intensity_mask"]
    assert call(None, OTHER, _abi.F32, 8, SOME, _abi.U8, 4, 0.0, None) == -1 and b"null" in fn["last_error"]()
    assert call(SOME, OTHER, _abi.F32, 8, None, _abi.U8, 4, 0.0, None) == -1
    assert call(SOME, OTHER, _abi.F32, -8, SOME, _abi.U8, 4, 0.0, None) == -1 and b"negative" in fn["last_error"]()
    assert call(SOME, OTHER, _abi.F32, 8, SOME, _abi.U8, 3, 0.0, None) == -1 and b"multiple" in fn["last_error"]()
    assert call(SOME, OTHER, _abi.F32, 8, SOME, _abi.U8, 0, 0.0, None) == -1
    assert call(SOME, OTHER, 10, 8, SOME, _abi.U8, 4, 0.0, None) == -2 and call(SOME, OTHER, _abi.F32, 8, SOME, -2, 4, 0.0, None) == -2
    assert call(None, None, _abi.F32, 0, None, _abi.U8, 0, 0.0, None) == 0


# -- classes ---------------------------------------------------------------------------------------------------------------
def _batch():
    image = tio.ScalarImage(torch.zeros(1, 2, 2, 2))
    seg = tio.LabelMap(torch.zeros(1, 2, 2, 2, dtype=torch.int16))
    return tio.SubjectsBatch.from_subjects([tio.Subject(t1=image, seg=seg, other=tio.ScalarImage(torch.zeros(1, 2, 2, 2)))])


def test_classes_aliases_and_exports():
    assert tio.RescaleIntensity is tio.Normalize and tio.ZNormalization is tio.Standardize
    for name in ("Normalize", "Standardize", "Clamp", "Mask", "RescaleIntensity", "ZNormalization"):
        assert name in tio.__all__ and name in tio.transforms.__all__ and getattr(tio.transforms, name) is getattr(tio, name)
    for name in ("Normalize", "_RescaleInverse", "Standardize", "_StandardizeInverse", "Clamp", "Mask"):
        assert name in tio.transforms.transform._TRANSFORM_REGISTRY  # history replay finds the classes by name
    for cls in (tio.Normalize, tio.Standardize, tio.Clamp, tio.Mask):
        assert issubclass(cls, tio.IntensityTransform)


def test_constructors_and_defaults():
    normalize = tio.Normalize()
    assert normalize.out_min.is_constant(-1.0) and normalize.out_max.is_constant(1.0) and normalize.in_min is None and normalize.in_max is None
    assert normalize.percentile_low.is_constant(0.0) and normalize.percentile_high.is_constant(100.0) and normalize.masking_method is None
    assert normalize.supports_per_instance_params and normalize.invertible and not normalize.draws_ahead
    ranged = tio.Normalize(out_min=(-1, 0), out_max=tio.Choice([1.0, 2.0]), in_min=-1000, in_max=(900, 1100), percentile_low=0.5, p=0.3)
    assert ranged.out_min._ranges[0] == (-1.0, 0.0) and ranged.in_min.is_constant(-1000.0) and ranged.in_max._ranges[0] == (900.0, 1100.0) and ranged.p == 0.3
    with pytest.raises(TypeError):
        tio.Normalize(0.0, 1.0)  # keyword-only, as in the reference
    standardize = tio.Standardize(masking_method="seg")
    assert standardize.masking_method == "seg" and standardize.invertible
    assert not standardize.supports_per_instance_params and not standardize.draws_ahead
    clamp = tio.Clamp(out_min=-1000, out_max=1000)
    assert (clamp.out_min, clamp.out_max) == (-1000, 1000) and not clamp.invertible and not clamp.supports_per_instance_params
    assert clamp.make_params(_batch()) == {"out_min": -1000, "out_max": 1000} and tio.Clamp().make_params(_batch()) == {"out_min": None, "out_max": None}
    tio.Clamp(out_min=2.0, out_max=2.0)
    with pytest.raises(ValueError, match=r"out_min \(3\) must be <= out_max \(2\)"):
        tio.Clamp(out_min=3, out_max=2)
    mask = tio.Mask()
    assert mask.masking_method == "brain" and mask.outside_value == 0.0 and mask.labels is None and not mask.invertible
    assert tio.Mask(masking_method="seg", labels=[1, 2], outside_value=-7).make_params(_batch()) == {}
    with pytest.raises(ValueError, match="Probability"):
        tio.Standardize(p=1.5)


def test_explicit_input_range_needs_no_voxel_values():
    """With ``in_min`` and ``in_max`` the parameters are drawn without a look at the data — no engine, no GPU."""
    batch = _batch()
    torch.manual_seed(3)
    params = tio.Normalize(in_min=-100.0, in_max=(50.0, 60.0), out_min=(0.0, 0.5), per_instance=False).make_params(batch)
    torch.manual_seed(3)
    expected_out_min = torch.empty(1).uniform_(0.0, 0.5).item()
    assert set(params) == {"out_min", "out_max", "in_min", "in_max"} and json.dumps(params)
    assert params["in_min"] == -100.0 and 50.0 <= params["in_max"] <= 60.0 and params["out_max"] == 1.0
    assert params["out_min"] == pytest.approx(expected_out_min, abs=1e-6)  # the first draw of make_params


def test_inverses_carry_the_parameters():
    params = {"out_min": [0.0, 0.5], "out_max": [1.0, 0.5], "in_ranges": {"t1": (2.0, 9.0)}, "_batch_size": 2, "_batched_keys": ["out_min", "out_max"]}
    undo = tio.Normalize().inverse(params)
    assert type(undo).__name__ == "_RescaleInverse" and undo.copy is False and undo.make_params(_batch()) == {}
    assert (undo._out_min, undo._out_max, undo._in_min, undo._in_max, undo._in_ranges) == ([0.0, 0.5], [1.0, 0.5], None, None, {"t1": (2.0, 9.0)})
    undo = tio.Standardize().inverse({"stats": {"t1": (3.0, 2.0)}})
    assert type(undo).__name__ == "_StandardizeInverse" and undo._stats == {"t1": (3.0, 2.0)} and undo.copy is False
    history = [tio.AppliedTransform("Clamp", {"out_min": 0.0, "out_max": None}), tio.AppliedTransform("Standardize", {"stats": {"t1": (3.0, 2.0)}}),
               tio.AppliedTransform("Mask", {}), tio.AppliedTransform("Normalize", {"out_min": 0.0, "out_max": 1.0, "in_min": 0.0, "in_max": 2.0})]
    replay = tio.get_inverse_transform(history, warn=False)
    assert [type(t).__name__ for t in replay.transforms] == ["_RescaleInverse", "_StandardizeInverse"]


@pytest.mark.parametrize("make", [lambda m: tio.Normalize(masking_method=m), lambda m: tio.Standardize(masking_method=m), lambda m: tio.Mask(masking_method=m)],
                         ids=["Normalize", "Standardize", "Mask"])
def test_masking_key_errors_come_before_any_compute(make):
    batch = _batch()
    with pytest.raises(KeyError, match='"brain" not found in batch images'):
        transform = make("brain")
        transform.apply_transform(batch, transform.make_params(batch))
    with pytest.raises(TypeError, match="must refer to a LabelMap"):
        transform = make("other")
        transform.apply_transform(batch, transform.make_params(batch))
    with pytest.raises(TypeError, match="masking_method must be"):
        transform = make(5)
        transform.apply_transform(batch, transform.make_params(batch))


def test_only_scalar_images_are_selected():
    batch = _batch()
    assert list(tio.Clamp(out_min=0)._get_images(batch)) == ["t1", "other"]
    assert list(tio.Standardize(exclude=["other"])._get_images(batch)) == ["t1"]
    assert list(tio.Normalize(include=["seg", "other"])._get_images(batch)) == ["other"]


def test_per_instance_output_range_is_subtracted_in_float32(monkeypatch):
    monkeypatch.setattr(normalize_module.ops, "h2d", lambda tensor, device: tensor)
    low, span = normalize_module._out_min_and_range([0.1, -0.3], [0.7, 0.9], torch.zeros(2, 1, 1, 1, 1))
    expected = torch.tensor([0.7, 0.9], dtype=torch.float32) - torch.tensor([0.1, -0.3], dtype=torch.float32)
    assert torch.equal(low, torch.tensor([0.1, -0.3])) and torch.equal(span, expected) and span.dtype == torch.float32
    assert normalize_module._out_min_and_range(0.1, 0.7, torch.zeros(1)) == (0.1, 0.7 - 0.1)


# -- the golden file (the reference's outputs) against the restatements -------------------------------------------------------
def test_golden_inputs_are_the_generators(golden):
    assert tuple(golden["shape"]) == cases.GOLDEN_SHAPE and golden["seed"] == cases.GOLDEN_SEED
    assert torch.equal(golden["image"], cases.golden_image()) and torch.equal(golden["labels"], cases.golden_labels())
    assert set(golden["cases"]) == set(cases.CASES) and os.path.getsize(GOLDEN) < 200 * 1024
    assert len(torch.unique(golden["labels"][0])) == 4


def _normalize_mask(name):
    method = cases.CASES[name][1].get("masking_method")
    if method is None:
        return None
    return cases.golden_labels()[0] if method == "seg" else method(cases.golden_image()[0])


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c[0] == "Normalize"])
def test_golden_normalize(golden, name):
    entry, arguments = golden["cases"][name], cases.CASES[name][1]
    params, image = entry["params"], cases.golden_image()
    assert entry["name"] == "Normalize"
    if "in_min" in arguments:
        in_min, in_max = params["in_min"], params["in_max"]
        assert (in_min, in_max) == (arguments["in_min"], arguments["in_max"]) and "in_ranges" not in params
    else:
        low, high = arguments.get("percentile_low", 0.0), arguments.get("percentile_high", 100.0)
        if isinstance(low, tuple):  # drawn: the range recorded must be some percentile range of the draw's interval
            in_min, in_max = params["in_ranges"]["t1"]
            assert cases.percentile_range(image[0], None, low[0], high)[0] <= in_min <= cases.percentile_range(image[0], None, low[1], high)[0]
        else:
            in_min, in_max = cases.percentile_range(image[0], _normalize_mask(name), low, high)
            assert params["in_ranges"] == {"t1": (in_min, in_max)}
    per_instance = arguments.get("per_instance", True)
    assert isinstance(params["out_min"], list) == per_instance and ("_batched_keys" in params) == per_instance
    assert torch.equal(entry["out"], cases.normalize(image, in_min, in_max, params["out_min"], params["out_max"]))
    if "restored" in entry:
        assert torch.equal(entry["restored"], cases.normalize_inverse(entry["out"], in_min, in_max, params["out_min"], params["out_max"]))


def test_golden_zero_range_inverse(golden):
    params = cases.ZERO_RANGE_INVERSE
    image = cases.golden_image()
    expected = cases.normalize_inverse(image, *params["in_ranges"]["t1"], params["out_min"], params["out_max"])
    assert torch.equal(golden["zero_range_restored"], expected)
    assert torch.equal(expected[1], image[1]) and not torch.equal(expected[0], image[0])  # out_min == out_max: that element stays


@pytest.mark.parametrize("name", ["standardize_plain", "standardize_masked"])
def test_golden_standardize(golden, name):
    entry = golden["cases"][name]
    image = cases.golden_image()
    mask = cases.golden_labels()[0] if name == "standardize_masked" else None
    values = cases.inside_values(image[0], mask)
    mean, std = entry["params"]["stats"]["t1"]
    assert entry["name"] == "Standardize" and (mean, std) == (float(values.mean().item()), float(values.std().item()))
    # the reference's float32 statistics lie within one float32 ulp of the float64 ones
    assert cases.ulps_off(mean, float(values.double().mean())) <= 1.0 and cases.ulps_off(std, float(values.double().std())) <= 1.0
    assert torch.equal(entry["out"], cases.standardize(image, mean, std))
    if "restored" in entry:
        assert torch.equal(entry["restored"], cases.standardize_inverse(entry["out"], mean, std))


def test_golden_clamp_and_mask(golden):
    image, labels = cases.golden_image(), cases.golden_labels()
    entries = golden["cases"]
    assert entries["clamp_one_bound"]["params"] == {"out_min": 0.0, "out_max": None}
    assert torch.equal(entries["clamp_one_bound"]["out"], cases.clamp(image, 0.0, None)) and bool((entries["clamp_one_bound"]["out"] >= 0).all())
    assert torch.equal(entries["clamp_both_bounds"]["out"], cases.clamp(image, -10.0, 50.5))
    assert torch.equal(entries["mask_by_key"]["out"], cases.mask_where(image, cases.label_mask(labels[0]), 0.0))
    expected = cases.mask_where(image, cases.label_mask(labels[0], [1, 3]), -7)
    assert torch.equal(entries["mask_labels"]["out"], expected) and bool((expected == -7).any())
    # the mask of element 0 applies to element 1 too (mask.py:91), both channels
    assert torch.equal(expected[1] == -7, (~cases.label_mask(labels[0], [1, 3])).expand_as(image[1]) | (image[1] == -7))


def test_quantile_restatement_is_torch_quantile():
    values = cases.golden_image().reshape(-1)
    for q in (0.0, 0.005, 0.37, 0.5, 0.995, 1.0):
        assert cases.compute_quantile(values, q) == pytest.approx(float(torch.quantile(values, q)), rel=1e-5)  # (torch.quantile ranks in float32)
        lower, upper = cases.order_statistics(values, q)
        assert float(lower) <= cases.compute_quantile(values, q) <= float(upper)
