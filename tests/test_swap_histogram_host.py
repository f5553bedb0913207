"""Swap / HistogramStandardization without a GPU: argument checks of the new entry points (nothing is launched), the draw order
of ``Swap.make_params`` against the reference's recorded parameters, the classes' constructors / errors, and the golden file
(the reference's own outputs, ``tests/golden/make_golden_swap_histogram.py``) against the torch-CPU restatements of
``swap_histogram_cases.py`` that the GPU tests compare the engine with."""
from __future__ import annotations

import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import swap_histogram_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.transforms import histogram_standardization as module

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swap_histogram_golden.pt")
SOME = ctypes.c_void_p(4096)  # non-null, 16-byte aligned pointers no check dereferences
OTHER = ctypes.c_void_p(1 << 30)
NEW = ("swap_patches", "intensity_multi_quantiles_workspace_bytes", "intensity_multi_quantiles", "histogram_standardize")


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


def _i3(*values):
    return (ctypes.c_int32 * 3)(*values)


def test_entry_points_are_hip_only_and_the_abi_number_stays(fn):
    assert _abi.ABI_VERSION >= 17 and fn["abi_version"]() == _abi.ABI_VERSION  # (these entry points: since 17)
    for name in NEW:
        assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "tio_hip.h")).read()
    for name in NEW:
        assert f"tio_{name}(" in header
    for where in ("swap.py:195", "histogram_standardization.py:280", "histogram_standardization.py:276"):
        assert where in header  # each entry names the reference lines it replaces
    assert fn["intensity_stats_workspace_bytes"]() == 4 * 2048 * 8 + 256  # the single-element selection's, unchanged


def test_swap_refuses_bad_arguments(fn):
    call = fn["swap_patches"]

    def run(x=SOME, y=OTHER, size=4, batch=2, channels=1, shape=(5, 6, 7), patch=(3, 4, 4), origins=SOME, counts=SOME, lists=1, s_max=3):
        return call(x, y, size, batch, channels, _i3(*shape), _i3(*patch), origins, counts, lists, s_max, None)

    assert run(x=None) == -1 and b"null" in fn["last_error"]()
    assert run(y=None) == -1
    assert run(origins=None) == -1 and b"null" in fn["last_error"]()
    assert run(counts=None) == -1
    assert run(size=3) == -2 and run(size=16) == -2 and b"bytes" in fn["last_error"]()
    assert run(batch=-1) == -1 and run(shape=(5, -6, 7)) == -1 and run(s_max=-1) == -1
    assert run(patch=(3, 7, 4)) == -1 and b"cannot be larger" in fn["last_error"]()
    assert run(patch=(0, 4, 4)) == -1
    assert run(lists=3) == -1 and b"location lists" in fn["last_error"]()
    assert run(y=SOME) == -1 and b"overlaps" in fn["last_error"]()
    assert run(y=ctypes.c_void_p(4096 + 4 * 100)) == -1  # (the ranges overlap)
    assert run(x=ctypes.c_void_p(4098)) == -1 and b"aligned" in fn["last_error"]()
    assert run(batch=4, lists=4, shape=(1 << 14, 1 << 14, 1 << 14), patch=(1, 1, 1)) == -5 and b"2^40" in fn["last_error"]()
    assert run(shape=(1 << 30, 1 << 30, 4), patch=(1, 1, 1)) == -5
    assert run(x=None, y=None, batch=0, lists=1) == 0  # nothing to do


def test_multi_quantiles_refuse_bad_arguments(fn):
    call, size_of = fn["intensity_multi_quantiles"], fn["intensity_multi_quantiles_workspace_bytes"]
    assert size_of(2, 13) == 2 * ((2048 + 27 * 128) * 8 + 2048)  # per element: pass 1's histogram, 2 * 13 + 1 groups of 128 bins, the state
    assert size_of(1, 0) == 0 and size_of(1, 33) == 0 and size_of(-1, 2) == 0
    fractions = (ctypes.c_double * 13)(*cases.DEFAULT_QUANTILES)

    def run(x=SOME, dtype=_abi.F32, batch=2, channels=2, spatial=64, mask=None, mask_dtype=0, mask_channels=0, q=fractions, n_q=13, values=OTHER,
            counts=OTHER, workspace=SOME, nbytes=None):
        nbytes = size_of(batch, n_q) if nbytes is None else nbytes
        return call(x, dtype, batch, channels, spatial, mask, mask_dtype, mask_channels, q, n_q, values, counts, workspace, nbytes, None)

    assert run(x=None) == -1 and b"null" in fn["last_error"]()
    assert run(values=None) == -1 and run(counts=None) == -1 and run(workspace=None) == -1
    assert run(q=None) == -1 and run(n_q=0) == -1 and run(n_q=33) == -1 and b"fractions" in fn["last_error"]()
    assert run(q=(ctypes.c_double * 2)(0.5, 1.5), n_q=2) == -1 and b"outside [0, 1]" in fn["last_error"]()
    assert run(q=(ctypes.c_double * 2)(float("nan"), 0.5), n_q=2) == -1
    assert run(dtype=9) == -2 and run(mask=SOME, mask_dtype=40, mask_channels=1) == -2
    assert run(channels=-1) == -1 and run(spatial=-1) == -1 and run(batch=-1) == -1 and b"negative" in fn["last_error"]()
    assert run(mask=SOME, mask_dtype=_abi.U8, mask_channels=3) == -1 and b"mask channels" in fn["last_error"]()
    assert run(nbytes=size_of(2, 13) - 1) == -1 and b"too small" in fn["last_error"]()
    assert run(workspace=ctypes.c_void_p(4100)) == -1 and b"aligned" in fn["last_error"]()
    assert run(batch=8, channels=1, spatial=1 << 38) == -5


def test_histogram_standardize_refuses_bad_arguments(fn):
    call = fn["histogram_standardize"]

    def run(x=SOME, y=OTHER, dtype=_abi.I16, batch=2, per_element=64, percentiles=SOME, landmarks=SOME, n=13, table=SOME):
        return call(x, y, dtype, batch, per_element, percentiles, landmarks, n, table, None)

    for name in ("x", "y", "percentiles", "landmarks", "table"):
        assert run(**{name: None}) == -1 and b"null" in fn["last_error"]()
    assert run(dtype=11) == -2
    assert run(batch=-1) == -1 and run(per_element=-1) == -1
    assert run(n=1) == -1 and run(n=33) == -1 and b"landmarks" in fn["last_error"]()
    assert run(batch=8, per_element=1 << 38) == -5
    assert run(x=None, y=None, batch=0) == 0 and run(x=None, y=None, per_element=0) == 0


# -- Swap ----------------------------------------------------------------------------------------------------------------
def _swap_batch(name):
    arguments, image, labels, seed = cases.swap_inputs(name)
    images = {"t1": (tio.ScalarImage, image)}
    if labels is not None:
        images["seg"] = (tio.LabelMap, labels)
    return tio.Swap(**arguments), cases._batch(tio, images, "cpu"), seed


@pytest.mark.parametrize("name", list(cases.SWAP_CASES))
def test_swap_make_params_draws_in_the_reference_order(golden, name):
    """On a CPU batch, without an engine: the gate draw, then ``make_params`` — the recorded parameters of the reference."""
    transform, batch, seed = _swap_batch(name)
    torch.manual_seed(seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if not transform._per_instance_p_active(batch):
            torch.rand(1)  # the batch-wide gate of `forward`
        params = transform.make_params(batch)
    assert params == golden[name]["params"]
    assert [str(w.message) for w in caught] == golden[name]["warnings"]
    assert all(image.data.device.type == "cpu" for image in batch.images.values())


def test_swap_golden_geometry(golden):
    overlap = golden["swap_all_pairs_overlap"]["params"]["locations"]
    assert len(overlap) == 30 and all(all(abs(a[d] - b[d]) < (3, 4, 4)[d] for d in range(3)) for a, b in overlap)
    gated = golden["swap_gated"]["params"]
    assert gated["_batched_keys"] == ["locations"] and gated["_batch_size"] == 6
    assert [entry == [] for entry in gated["locations"]] == [not keep for keep in gated["_keep"]] and 0 < sum(gated["_keep"]) < 6
    assert all(a[1] == 0 and b[1] == 0 for pairs in golden["swap_patch_spans_an_axis"]["params"]["locations"] for a, b in pairs)
    lengths = [len(pairs) for pairs in golden["swap_iteration_range"]["params"]["locations"]]
    assert all(2 <= n <= 9 for n in lengths)
    assert [len(pairs) for pairs in golden["swap_default_per_instance"]["params"]["locations"]] == [100, 100]
    assert "_batched_keys" not in golden["swap_shared"]["params"]


@pytest.mark.parametrize("name", list(cases.SWAP_CASES))
def test_both_swap_restatements_reproduce_the_reference(golden, name):
    arguments, image, labels, _ = cases.swap_inputs(name)
    patch = tio.Swap(**arguments).patch_size
    locations = golden[name]["params"]["locations"]
    expected = golden[name]["out"]["t1"]
    assert cases.same(cases.swap_sequential(image, locations, patch), expected)
    assert cases.same(cases.swap_backward_trace(image, locations, patch), expected)
    if labels is not None:
        assert torch.equal(golden[name]["out"]["seg"], labels)


def test_swap_constructor_and_errors():
    swap = tio.Swap()
    assert swap.patch_size == (15, 15, 15) and not swap.invertible and swap.supports_per_instance_params and swap.supports_per_instance_p
    assert tio.Swap(patch_size=(2, 3, 4)).patch_size == (2, 3, 4)
    with pytest.raises(ValueError, match="non-negative"):
        tio.Swap(num_iterations=-1)
    batch = cases._batch(tio, {"t1": (tio.ScalarImage, torch.zeros(1, 1, 4, 5, 6))}, "cpu")
    with pytest.raises(ValueError, match=r"Patch size \(5, 5, 5\) cannot be larger than spatial shape \(4, 5, 6\)"):
        tio.Swap(patch_size=5).make_params(batch)
    assert tio.transforms.Swap is tio.Swap and "Swap" in tio.__all__ and "HistogramStandardization" in tio.__all__


# -- HistogramStandardization ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.HISTOGRAM_CASES))
def test_standardization_restatement_reproduces_the_reference(golden, name):
    arguments, image, other, landmarks, quantiles = cases.histogram_inputs(name)
    expected = golden[name]["out"]
    assert golden[name]["params"] == {} and golden[name]["name"] == "HistogramStandardization"
    assert expected["t1"].dtype == image.dtype
    assert cases.same(cases.standardize(image, landmarks, quantiles), expected["t1"])
    if "t2" in expected:
        assert torch.equal(expected["t2"], other)  # not included: untouched


@pytest.mark.parametrize("name", list(cases.LANDMARK_CASES))
def test_landmark_training_restatement_and_host_half(golden, name):
    entry = golden[name]
    trained = cases.train_landmarks(cases.training_images(), cases.DEFAULT_QUANTILES, cases.LANDMARK_CASES[name])
    assert torch.equal(trained, entry["landmarks"])
    database = entry["database"].numpy()
    assert torch.equal(torch.as_tensor(module._compute_average_mapping(database), dtype=torch.float32), entry["landmarks"])
    assert np.array_equal(module._compute_average_mapping(database), cases.average_landmarks(database))


def test_numpy_percentile_rule():
    """The rule the device finish restates, against numpy itself: the difference rounded to float32, the rest float64."""
    for seed, n in enumerate([2, 3, 101, 4020, 999]):
        values = np.sort(cases.randn((n,), seed, 10.0 ** (seed - 2)).numpy())
        expected = np.percentile(values, [100.0 * q for q in cases.DEFAULT_QUANTILES])
        got = []
        for q in cases.DEFAULT_QUANTILES:
            virtual = (100.0 * q) / 100.0 * (n - 1)
            lower = int(np.floor(virtual))
            gamma = virtual - lower
            a, b = values[lower], values[min(lower + 1, n - 1)]
            difference = np.float64(np.float32(b - a))
            got.append(np.float64(b) - difference * (1 - gamma) if gamma >= 0.5 else np.float64(a) + difference * gamma)
        assert expected.dtype == np.float64 and cases.same_bits64(got, expected)


def test_quantile_helpers_and_constants():
    assert module.DEFAULT_CUTOFF == (0.01, 0.99) and module.STANDARD_RANGE == (0.0, 100.0)
    assert module._build_quantiles((0.01, 0.99)) == cases.DEFAULT_QUANTILES
    assert module._build_quantiles((0.02, 0.98)) == cases.WIDE_QUANTILES
    module._validate_quantiles(cases.DEFAULT_QUANTILES, (0.01, 0.99))
    with pytest.raises(ValueError, match="Need at least 2 quantiles, got 1"):
        module._validate_quantiles((0.5,), (0.5, 0.5))
    with pytest.raises(ValueError, match=r"All quantiles must be in \[0, 1\]"):
        module._validate_quantiles((0.01, 1.5), (0.01, 1.5))
    with pytest.raises(ValueError, match="must be included in quantiles"):
        module._validate_quantiles((0.1, 0.9), (0.01, 0.99))
    with pytest.raises(ValueError, match="must be included in quantiles"):
        module.compute_histogram_landmarks([], quantiles=[0.1, 0.5, 0.9])
    with pytest.raises(TypeError, match="Image data must be a tensor or ndarray, got str"):
        module.compute_histogram_landmarks(["subject_a_t1.nii"])


def test_landmarks_are_loaded_from_tensors_and_files(tmp_path):
    landmarks = cases.landmarks_for(cases.DEFAULT_QUANTILES)
    assert torch.equal(tio.HistogramStandardization(landmarks.double()).landmarks, landmarks) and tio.HistogramStandardization(landmarks).landmarks.dtype == torch.float32
    np.save(tmp_path / "landmarks.npy", landmarks.double().numpy())
    torch.save(landmarks, tmp_path / "landmarks.pt")
    torch.save(landmarks, tmp_path / "landmarks.pth")
    torch.save({"landmarks": landmarks}, tmp_path / "wrong.pt")
    for name in ("landmarks.npy", "landmarks.pt", "landmarks.pth"):
        for path in (tmp_path / name, str(tmp_path / name)):
            loaded = tio.HistogramStandardization(path)
            assert torch.equal(loaded.landmarks, landmarks) and loaded.landmarks.dtype == torch.float32
    with pytest.raises(TypeError, match="Expected a Tensor in .*wrong.pt, got dict"):
        tio.HistogramStandardization(tmp_path / "wrong.pt")
    with pytest.raises(ValueError, match="Unsupported landmarks file extension: .txt"):
        tio.HistogramStandardization(tmp_path / "landmarks.txt")
    transform = tio.HistogramStandardization(landmarks, cutoff=(0.02, 0.98), include=["t1"])
    assert transform.cutoff == (0.02, 0.98) and transform.include == ["t1"] and not transform.invertible
    assert transform.make_params(None) == {}
    batch = cases._batch(tio, {"t1": (tio.ScalarImage, torch.zeros(1, 1, 2, 2, 2))}, "cpu")
    with pytest.raises(ValueError, match=r"Number of landmarks \(13\) does not match the number of quantile positions \(15\)"):
        transform.apply_transform(batch, {})  # raised at apply time, before any engine call
