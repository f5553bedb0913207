"""The label-map transforms without a GPU: argument checks of the five new entry points (nothing is launched), the workspace
size, the six classes' constructors / parameters / inverses / history names, and the golden file (the reference's own
outputs, ``tests/golden/make_golden_labels.py``) against the torch-CPU restatements the GPU tests compare with."""
from __future__ import annotations

import ctypes
import json
import os

import pytest
import torch

import label_cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.transforms import labels as label_transforms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labels_golden.pt")
SOME = ctypes.c_void_p(4096)  # a non-null pointer no check dereferences


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def _shape(*values):
    return (ctypes.c_int32 * 3)(*values)


def test_abi_version_is_17(fn):
    assert _abi.ABI_VERSION >= 17 and fn["abi_version"]() == _abi.ABI_VERSION  # (these entry points: since 17)
    for name in ("label_remap", "label_one_hot", "label_contour", "keep_largest_component", "keep_largest_workspace_bytes"):
        assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES


def test_remap_refuses_bad_arguments(fn):
    remap = fn["label_remap"]
    assert remap(None, None, _abi.I32, 8, None, None, 0, 0, 0.0, None, None) == -1
    assert b"null" in fn["last_error"]()
    assert remap(SOME, SOME, _abi.I32, 8, None, None, 2, 0, 0.0, None, None) == -1  # pairs without keys
    assert remap(SOME, SOME, _abi.I16, 8, SOME, SOME, 2, 0, 0.0, None, None) == -1  # int16 without its table
    assert remap(SOME, SOME, _abi.I32, -1, SOME, SOME, 2, 0, 0.0, None, None) == -1
    assert b"negative" in fn["last_error"]()
    assert remap(SOME, SOME, _abi.I32, 8, SOME, SOME, -2, 0, 0.0, None, None) == -1
    assert remap(SOME, SOME, _abi.I32, 8, SOME, SOME, 65537, 0, 0.0, None, None) == -1
    assert b"n_pairs" in fn["last_error"]()
    assert remap(SOME, SOME, _abi.I32, 8, SOME, SOME, 2, 7, 0.0, None, None) == -1
    assert b"mode" in fn["last_error"]()
    assert remap(SOME, SOME, 99, 8, SOME, SOME, 2, 0, 0.0, None, None) == -2
    assert remap(None, None, _abi.I32, 0, None, None, 0, 0, 0.0, None, None) == 0  # nothing to do


def test_one_hot_refuses_bad_arguments(fn):
    one_hot = fn["label_one_hot"]
    assert one_hot(None, None, _abi.U8, 1, 8, 4, SOME, None) == -1
    assert b"null" in fn["last_error"]()
    assert one_hot(SOME, SOME, _abi.U8, 1, 8, 4, None, None) == -1
    assert one_hot(SOME, SOME, _abi.U8, -1, 8, 4, SOME, None) == -1
    assert one_hot(SOME, SOME, _abi.U8, 1, -8, 4, SOME, None) == -1
    assert one_hot(SOME, SOME, _abi.U8, 1, 8, -4, SOME, None) == -1
    assert b"negative" in fn["last_error"]()
    assert one_hot(SOME, SOME, 42, 1, 8, 4, SOME, None) == -2
    assert one_hot(None, None, _abi.U8, 0, 8, 4, SOME, None) == 0


def test_contour_refuses_bad_arguments(fn):
    contour = fn["label_contour"]
    assert contour(None, None, _abi.I16, 1, _shape(2, 2, 2), None) == -1
    assert b"null" in fn["last_error"]()
    assert contour(SOME, SOME, _abi.I16, 1, None, None) == -1
    assert contour(SOME, SOME, _abi.I16, -1, _shape(2, 2, 2), None) == -1
    assert contour(SOME, SOME, _abi.I16, 1, _shape(2, -2, 2), None) == -1
    assert b"negative" in fn["last_error"]()
    assert contour(SOME, SOME, -3, 1, _shape(2, 2, 2), None) == -2
    assert contour(None, None, _abi.I16, 1, _shape(2, 0, 2), None) == 0


def test_keep_largest_refuses_bad_arguments(fn):
    keep = fn["keep_largest_component"]
    shape = _shape(2, 3, 4)
    assert keep(None, None, _abi.I16, 1, shape, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert b"null" in fn["last_error"]()
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, None, 1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, SOME, 1, 0.0, 1, None, 1 << 20, None) == -1
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, None, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, -1, shape, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, SOME, -1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert b"negative" in fn["last_error"]()
    assert keep(SOME, SOME, _abi.I16, 1, shape, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -1
    assert b"alias" in fn["last_error"]()
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, SOME, 1, 0.0, 1, SOME, 16, None) == -1
    assert b"too small" in fn["last_error"]()
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, SOME, 1, 0.0, 1, ctypes.c_void_p(4100), 1 << 20, None) == -1
    assert b"aligned" in fn["last_error"]()
    for dtype in (_abi.F64, _abi.F16, _abi.BF16, 77):
        assert keep(SOME, ctypes.c_void_p(8192), dtype, 1, shape, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -2
    assert keep(SOME, ctypes.c_void_p(8192), _abi.I16, 1, shape, SOME, _abi.KEEP_LARGEST_MAX_LABELS + 1, 0.0, 1, SOME, 1 << 20, None) == -5
    assert keep(SOME, ctypes.c_void_p(8192), _abi.U8, 2, _shape(1024, 1024, 1024), SOME, 1, 0.0, 1, SOME, 1 << 20, None) == -5
    assert b"32-bit" in fn["last_error"]()
    assert keep(None, None, _abi.I16, 0, shape, SOME, 1, 0.0, 1, SOME, 1 << 20, None) == 0
    assert _abi.KEEP_LARGEST_MAX_LABELS >= 256


def test_workspace_bytes_grow_with_the_voxel_count(fn):
    size = fn["keep_largest_workspace_bytes"]
    assert size(1, None, 1) == -1 and size(-1, _shape(1, 1, 1), 1) == -1
    previous = 0
    for extent in (1, 2, 3, 5, 8, 13, 64, 65, 300, 512):
        now = size(1, _shape(extent, extent, extent), 4)
        assert now >= 8 * extent**3 and now >= previous  # a parent and a size per voxel
        previous = now
    assert size(2, _shape(8, 8, 8), 4) >= size(1, _shape(8, 8, 8), 4)
    assert size(1, _shape(8, 8, 8), 200) > size(1, _shape(8, 8, 8), 4)


def _batch():
    image = tio.ScalarImage(torch.zeros(1, 2, 2, 2))
    seg = tio.LabelMap(torch.zeros(1, 2, 2, 2, dtype=torch.int16))
    return tio.SubjectsBatch.from_subjects([tio.Subject(t1=image, seg=seg)])


def test_constructors_params_and_inverses():
    batch = _batch()
    remap = tio.RemapLabels({1: 2, 3: 4})
    params = remap.make_params(batch)
    assert params == {"remapping": {1: 2, 3: 4}} and json.dumps(params)
    assert remap.invertible and remap.inverse(params).remapping == {2: 1, 4: 3} and remap.inverse(params).copy is False
    remove = tio.RemoveLabels([3, 4], background_label=7)
    assert remove.labels == [3, 4] and remove.background_label == 7 and remove.make_params(batch) == {} and not remove.invertible
    with pytest.raises(TypeError):
        tio.RemoveLabels([1], 0)  # background_label is keyword-only, as in the reference
    sequential = tio.SequentialLabels()
    assert sequential.invertible
    undo = sequential.inverse({"remappings": {"seg": {0: 0, 5: 1}}})
    assert type(undo).__name__ == "_SequentialLabelsInverse" and undo._remappings == {"seg": {0: 0, 5: 1}} and undo.make_params(batch) == {}
    one_hot = tio.OneHot(num_classes=5)
    assert one_hot.make_params(batch) == {"num_classes": 5} and tio.OneHot().num_classes == -1
    assert one_hot.invertible and type(one_hot.inverse({})).__name__ == "_OneHotInverse"
    with pytest.raises(TypeError):
        tio.OneHot(5)
    contour = tio.Contour()
    assert contour.make_params(batch) == {} and not contour.invertible
    keep = tio.KeepLargestComponent()
    assert keep.labels is None and keep.background_label == 0 and keep.fully_connected is True and keep.make_params(batch) == {}
    keep = tio.KeepLargestComponent((1, 2), background_label=3, fully_connected=False, p=0.5)
    assert keep.labels == [1, 2] and keep.background_label == 3 and keep.fully_connected is False and keep.p == 0.5 and not keep.invertible
    for name in ("RemapLabels", "RemoveLabels", "SequentialLabels", "_SequentialLabelsInverse", "OneHot", "_OneHotInverse", "Contour",
                 "KeepLargestComponent"):
        assert name in tio.transforms.transform._TRANSFORM_REGISTRY  # history replay finds the classes by name
    for name in ("RemapLabels", "RemoveLabels", "SequentialLabels", "OneHot", "Contour", "KeepLargestComponent"):
        assert name in tio.__all__ and name in tio.transforms.__all__


def test_only_label_maps_are_selected():
    batch = _batch()
    assert list(tio.Contour()._label_maps(batch)) == ["seg"]
    assert list(tio.Contour(exclude=["seg"])._label_maps(batch)) == []


def test_inverse_from_history_names():
    history = [tio.AppliedTransform("RemapLabels", {"remapping": {1: 2}}), tio.AppliedTransform("KeepLargestComponent", {}),
               tio.AppliedTransform("OneHot", {"num_classes": -1})]
    undo = tio.get_inverse_transform(history, warn=False)
    assert [type(t).__name__ for t in undo.transforms] == ["_OneHotInverse", "RemapLabels"]
    assert undo.transforms[1].remapping == {2: 1}


def test_unrepresentable_values_are_refused():
    check = label_transforms._check_representable
    check(255, torch.uint8, "label")
    check(-128, torch.int8, "label")
    check(256.0, torch.bfloat16, "label")
    for value, dtype in ((256, torch.uint8), (-1, torch.uint8), (128, torch.int8), (40000, torch.int16), (1.5, torch.int32),
                         (257, torch.bfloat16), (2049, torch.float16), (float("nan"), torch.float32)):
        with pytest.raises(ValueError, match="cannot be represented"):
            check(value, dtype, "label")


def test_one_hot_inverse_runs_on_the_host_engine_free_path():
    """``_OneHotInverse`` is plain tensor algebra: it needs no engine."""
    data = label_cases.label_field((1, 1, 4, 5, 6), 0)
    batch = tio.SubjectsBatch.from_subjects([tio.Subject(seg=tio.LabelMap(label_cases.one_hot(data)[0]))])
    restored = label_transforms._OneHotInverse().apply_transform(batch, {})
    assert torch.equal(restored.images["seg"].data, data.float())


# -- the golden file (the reference's outputs) against the restatements ------------------------------------------------------
def test_golden_field_is_the_generator_s(golden):
    assert torch.equal(golden["field"].long(), label_cases.label_field(tuple(golden["shape"]), golden["seed"]))


def test_golden_remap_family(golden):
    field, sparse = golden["field"], golden["sparse"]
    assert golden["remap_params"] == {"remapping": {1: 2, 2: 1, 3: 7, 9: 4}}
    assert torch.equal(golden["remap"], label_cases.remap(field, {1: 2, 2: 1, 3: 7, 9: 4}))
    assert torch.equal(golden["remove"], label_cases.remap(field, {2: 6, 3: 6}))
    mapping = golden["sequential_params"]["remappings"]["seg"]
    assert mapping == {0: 0, 5: 1, 10: 2, 40: 3}
    assert torch.equal(golden["sequential"], label_cases.remap(sparse, mapping, default=0))
    assert torch.equal(golden["sequential"], field)


def test_golden_one_hot_and_contour(golden):
    field = golden["field"]
    assert torch.equal(golden["one_hot"].float(), label_cases.one_hot(field))
    assert torch.equal(golden["one_hot_6"].float(), label_cases.one_hot(field, 6)) and golden["one_hot_6"].shape[1] == 6
    assert torch.equal(golden["contour"].float(), label_cases.contour(field))
    assert bool((golden["contour"][:, :, 0] == 1).all())  # every face voxel is marked (the -1 padding is smaller)


@pytest.mark.parametrize("fully_connected", [True, False])
def test_golden_keep_largest(golden, fully_connected):
    field = golden["field"]
    assert not label_cases.has_tie(field, [1, 2, 3], fully_connected)
    assert torch.equal(golden[f"keep_largest_{int(fully_connected)}"], label_cases.keep_largest(field, [1, 2, 3], 0, fully_connected))
    if fully_connected:
        assert torch.equal(golden["keep_largest_label2_background5"], label_cases.keep_largest(field, [2], 5, True))


@pytest.mark.parametrize("shape", [(24, 20, 37), (5, 7, 66), (1, 9, 130)])
@pytest.mark.parametrize("fully_connected", [True, False])
def test_component_restatement_gives_scipy_s_partition(shape, fully_connected):
    import numpy as np
    from scipy import ndimage

    volume = label_cases.label_field((1, 1, *shape), 0)[0, 0]
    ours = label_cases.components(volume, fully_connected)
    structure = np.ones((3, 3, 3)) if fully_connected else ndimage.generate_binary_structure(3, 1)
    for value in range(4):
        numbered, count = ndimage.label((volume == value).numpy(), structure=structure)
        mask = volume == value
        pairs = torch.stack([ours[mask], torch.from_numpy(numbered.astype(np.int64))[mask]], dim=1)
        assert torch.unique(pairs, dim=0).shape[0] == count == torch.unique(ours[mask]).numel()  # a bijection between the numberings
