"""LabelsToImage without a GPU: the entry point's place in the ABI, its argument checks (nothing is launched), the engine
method's own checks, constructor / ``repr`` / errors, and the draw order of ``make_params`` against the parameters the
unmodified reference recorded (``tests/golden/make_golden_labels_to_image.py``)."""
from __future__ import annotations

import ctypes
import os

import pytest
import torch

import labels_to_image_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd import ops
from torchio_amd.transforms.transform import _TRANSFORM_REGISTRY

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labels_to_image_golden.pt")
SOME = ctypes.c_void_p(4096)  # non-null, 16-byte aligned pointers no check dereferences
OTHER = ctypes.c_void_p(1 << 30)
THIRD = ctypes.c_void_p(1 << 31)


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


# -- the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_point_is_hip_only_and_the_abi_number_stays(fn):
    assert _abi.ABI_VERSION == 18 and fn["abi_version"]() == 18
    name = "labels_to_image"
    assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
    root = os.path.join(os.path.dirname(GOLDEN), "..", "..")
    header = open(os.path.join(root, "include", "tio_hip.h")).read()
    assert "int tio_labels_to_image(const void* labels, int32_t dtype, int32_t batch, int32_t channels, int64_t n_spatial," in header
    for where in ("labels_to_image.py:182-218 _generate_per_element", ":263-290 _generate_from_labels"):
        assert where in header  # the entry names the reference lines it replaces
    assert "tio_labels_to_image" not in open(os.path.join(root, "oracle", "tio_oracle.c")).read()  # no CPU counterpart


def test_entry_point_refuses_bad_arguments(fn):
    call = fn["labels_to_image"]

    def run(labels=SOME, dtype=_abi.I16, batch=2, channels=1, n=315, keys=OTHER, n_keys=3, mean=OTHER, std=OTHER, batched=0, out=THIRD, base=None,
            base_key=0):
        return call(labels, dtype, batch, channels, n, keys, n_keys, mean, std, batched, out, 7, base, base_key, None)

    def text():
        return fn["last_error"]()

    assert run(labels=None) == -1 and b"null labels or output" in text()
    assert run(out=None) == -1 and b"null labels or output" in text()
    for name in ("keys", "mean", "std"):
        assert run(**{name: None}) == -1 and b"null keys, means or deviations" in text()
    assert run(dtype=9) == -2 and b"unknown dtype 9" in text()
    assert run(dtype=-1) == -2
    for name in ("batch", "channels", "n", "n_keys"):
        assert run(**{name: -1}) == -1 and b"negative size" in text()
    assert run(n_keys=_abi.REMAP_MAX_PAIRS + 1) == -1 and b"beyond 65536" in text()
    assert run(base=OTHER, n_keys=0) == -1 and b"one-label mode without keys" in text()
    assert run(base=OTHER, base_key=3) == -1 and b"base_key 3 outside [0, 3)" in text()
    assert run(base=OTHER, base_key=-1) == -1 and b"base_key -1 outside" in text()
    assert run(batch=65536) == -5 and b"65535" in text()
    assert run(out=SOME) == -1 and b"overlaps" in text()
    assert run(out=ctypes.c_void_p(4096 + 2 * 2 * 315 - 4)) == -1 and b"overlaps" in text()  # the last label element
    assert run(labels=ctypes.c_void_p(4096 + 4 * 2 * 315 - 4), out=SOME) == -1 and b"overlaps" in text()  # the last output element
    assert run(base=THIRD, out=THIRD) == -1 and b"overlaps the draws" in text()
    assert run(base=ctypes.c_void_p((1 << 31) + 4 * 2 * 315 - 4)) == -1 and b"overlaps the draws" in text()  # the last output element
    assert run(base=ctypes.c_void_p((1 << 31) - 4 * 2 * 315 + 4)) == -1 and b"overlaps the draws" in text()  # the last draw
    assert run(channels=0) == -1 and b"without channels" in text()
    assert run(labels=ctypes.c_void_p(4097)) == -1 and b"not aligned" in text()
    assert run(out=ctypes.c_void_p((1 << 31) + 2)) == -1 and b"not aligned" in text()
    # nothing to do: OK whatever the pointers are
    assert run(labels=None, out=None, batch=0) == 0 and run(labels=None, out=None, keys=None, mean=None, std=None, n=0) == 0


def test_engine_refuses_bad_arguments_before_any_launch():
    """On host tensors: shape and list errors are ``ValueError``; a well-formed call is refused as a CPU tensor."""
    engine = ops.Engine(_lib.load()[1], "cuda", "hip")
    labels = torch.zeros(2, 1, 3, 4, 5, dtype=torch.int16)
    with pytest.raises(ValueError, match=r"labels_to_image: expected a \(B, C, I, J, K\) tensor"):
        engine.labels_to_image(labels[0], [0], [0.5], [0.1], seed=1)
    with pytest.raises(ValueError, match="either seed .* or base and base_key"):
        engine.labels_to_image(labels, [0], [0.5], [0.1])
    with pytest.raises(ValueError, match="either seed .* or base and base_key"):
        engine.labels_to_image(labels, [0], [0.5], [0.1], seed=1, base=torch.zeros(2, 1, 3, 4, 5), base_key=0)
    for keys in ([1, 0], [0, 0], [0, 2, 1]):
        with pytest.raises(ValueError, match="the keys must be strictly ascending"):
            engine.labels_to_image(labels, keys, [0.5] * len(keys), [0.1] * len(keys), seed=1)
    with pytest.raises(ValueError, match="the keys must be strictly ascending"):  # a tensor of keys is checked like a list
        engine.labels_to_image(labels, torch.tensor([0.0, 2.0, 1.0], dtype=torch.float64), [0.5] * 3, [0.1] * 3, seed=1)
    with pytest.raises(ValueError, match=r"means \(2,\) and stds \(1,\) for 2 keys and a batch of 2"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1], seed=1)
    with pytest.raises(ValueError, match=r"means \(3, 2\) and stds \(3, 2\) for 2 keys and a batch of 2"):
        engine.labels_to_image(labels, [0, 1], [[0.5, 0.5]] * 3, [[0.1, 0.1]] * 3, seed=1)
    with pytest.raises(ValueError, match=r"base_key 2 outside \[0, 2\)"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], base=torch.zeros(2, 1, 3, 4, 5), base_key=2)
    with pytest.raises(ValueError, match="base_key None outside"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], base=torch.zeros(2, 1, 3, 4, 5))
    with pytest.raises(ValueError, match=r"base must be float32 of shape \(2, 1, 3, 4, 5\)"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], base=torch.zeros(2, 1, 3, 4, 6), base_key=0)
    with pytest.raises(ValueError, match="out is reused in one-label mode only"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], seed=1, out=torch.zeros(2, 1, 3, 4, 5))
    with pytest.raises(ValueError, match="out must be contiguous float32"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], base=torch.zeros(2, 1, 3, 4, 5), base_key=0, out=torch.zeros(2, 1, 3, 4, 5).double())
    with pytest.raises(ops.EngineError, match="labels_to_image: tensor on cpu"):
        engine.labels_to_image(labels, [0, 1], [0.5, 0.5], [0.1, 0.1], seed=1)


# -- the transform -------------------------------------------------------------------------------------------------------
def _batch(**images):
    return tio.SubjectsBatch.from_subjects([tio.Subject(**images)])


def test_constructor_repr_errors_and_place_in_the_package():
    default = tio.LabelsToImage()
    assert default.label_key is None and default.image_key == "image_from_labels" and default.mean_ranges is None and default.std_ranges is None
    assert default.ignore_background is False and default.p == 1.0 and default.per_instance is True
    assert repr(default) == "LabelsToImage()"
    assert default.default_mean._original == (0.1, 0.9) and default.default_std._original == (0.01, 0.1)
    custom = tio.LabelsToImage("seg", image_key="synthetic", mean=[(0.8, 1.0), 0.3], std=[0.1], default_mean=0.5, ignore_background=True, p=0.5)
    assert repr(custom) == "LabelsToImage(label_key='seg', image_key='synthetic', default_mean=0.5, ignore_background=True, p=0.5)"
    assert len(custom.mean_ranges) == 2 and len(custom.std_ranges) == 1 and custom.mean_ranges[1].sample_1d() == 0.3
    assert tio.transforms.LabelsToImage is tio.LabelsToImage and "LabelsToImage" in tio.__all__ and "LabelsToImage" in tio.transforms.__all__
    assert _TRANSFORM_REGISTRY["LabelsToImage"] is tio.LabelsToImage  # history replay finds it by name
    assert default.supports_per_instance_params and not default.supports_per_instance_p and not default.draws_ahead and not default.invertible
    with pytest.raises(NotImplementedError, match="LabelsToImage is not invertible"):
        default.inverse({})
    with pytest.raises(TypeError):
        tio.LabelsToImage("seg", "synthetic")  # image_key is keyword-only, as in the reference

    scalar_only = _batch(t1=tio.ScalarImage(torch.zeros(1, 2, 2, 2)), t2=tio.ScalarImage(torch.zeros(1, 2, 2, 2)))
    with pytest.raises(KeyError, match="No LabelMap found in the subject"):
        default.make_params(scalar_only)
    with pytest.raises(KeyError) as info:
        tio.LabelsToImage("seg").make_params(scalar_only)
    assert info.value.args[0] == "Label key 'seg' not found. Available: ['t1', 't2']"
    with pytest.raises(KeyError, match="Label key 'seg' not found"):
        tio.LabelsToImage("seg").apply_transform(scalar_only, {"means": {}, "stds": {}})


@pytest.mark.parametrize("name", list(cases.CASES))
def test_make_params_draws_what_the_reference_drew(name, golden, oracle, monkeypatch):
    """Gate draw, then ``make_params``: the recorded dictionary, value for value, and the generator where the reference's
    stood.  (8- and 16-bit maps take their labels from ``Engine.unique_labels``: the CPU oracle's here.)"""
    monkeypatch.setattr(ops, "_ENGINE", oracle)
    entry = golden[name]
    assert entry["seed"] == cases.CASES[name][0] and torch.equal(entry["labels"], torch.stack(cases.CASES[name][1]()))
    params, after = cases.draw_case(tio, name)
    assert params == entry["params"] and after == entry["after_params"]
    per_element = "_batched_keys" in params
    assert per_element == (entry["labels"].shape[0] > 1 and "shared" not in name)
    if per_element:
        assert params["_batched_keys"] == ["means", "stds"] and params["_batch_size"] == len(params["means"]) == len(params["stds"])


def test_duplicate_int_keys_draw_twice_and_the_second_stays(golden):
    """1.2 and 1.7 both become key 1: five labels, four keys, and the generator moved on by five pairs of draws."""
    params = golden["non_integer_float32"]["params"]
    assert [sorted(m) for m in params["means"]] == [[0, 1, 2, 3]] * 2
    transform = tio.LabelsToImage()
    torch.manual_seed(3)
    means, stds = transform._sample_label_values([0, 1, 1, 2, 3])
    torch.manual_seed(3)
    pairs = [(transform.default_mean.sample_1d(), abs(transform.default_std.sample_1d())) for _ in range(5)]
    assert means == {0: pairs[0][0], 1: pairs[2][0], 2: pairs[3][0], 3: pairs[4][0]}
    assert stds == {0: pairs[0][1], 1: pairs[2][1], 2: pairs[3][1], 3: pairs[4][1]}


def test_ignore_background_draws_nothing_for_label_zero():
    transform = tio.LabelsToImage(ignore_background=True, mean=[(5.0, 6.0), (7.0, 8.0)])
    torch.manual_seed(4)
    means, stds = transform._sample_label_values([-1, 0, 2])
    torch.manual_seed(4)
    first = (transform.mean_ranges[0].sample_1d(), abs(transform.default_std.sample_1d()))
    third = (transform.default_mean.sample_1d(), abs(transform.default_std.sample_1d()))  # ranges go by INDEX: label 2 is index 2
    assert means == {-1: first[0], 0: 0.0, 2: third[0]} and stds == {-1: first[1], 0: 0.0, 2: third[1]}
