"""Reorient, Transpose, CropOrPad, EnsureShapeMultiple, ToReferenceSpace and CopyAffine without a GPU: the place of
``tio_permute3d`` in the ABI and its argument checks (nothing is launched), the engine method's own checks, and the host
logic of the six classes against what the unmodified reference recorded (``tests/golden/make_golden_orientation.py``).

``CropOrPad`` and ``EnsureShapeMultiple`` run on the CPU oracle engine (``tio_pad3d`` and a view).  The oracle has no
``permute3d``; for ``Reorient`` and ``Transpose`` a stand-in engine answers it with ``torch.flip`` / ``permute``, so that
parameters, affines and history are checked here and the kernel itself in ``tests/test_gpu_orientation.py``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import orientation_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd import ops
from torchio_amd.transforms.transform import _TRANSFORM_REGISTRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orientation_golden.pt")
SOME = ctypes.c_void_p(4096)  # non-null pointers no check dereferences
OTHER = ctypes.c_void_p(1 << 30)
AFFINE_BAR = cases.AFFINE_BAR
assert_same = cases.assert_same


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


class _TorchPermute:
    """The oracle engine plus ``permute3d`` as the reference's own tensor ops."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def permute3d(self, data, perm, flip_axes=()):
        return cases.aten_permute(data, list(perm), sum(1 << axis for axis in flip_axes))


@pytest.fixture()
def on_oracle(oracle, monkeypatch):
    monkeypatch.setattr(ops, "_ENGINE", _TorchPermute(oracle))


# -- the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_point_is_hip_only_and_the_abi_number_stays(fn):
    assert _abi.ABI_VERSION == 18 and fn["abi_version"]() == 18
    name = "permute3d"
    assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
    header = open(os.path.join(ROOT, "include", "tio_hip.h")).read()
    assert "int tio_permute3d(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels," in header
    assert "const int32_t in_shape[3], const int32_t perm[3], int32_t flip_mask, void* stream);" in header
    for where in ("reorient.py:63-91 _apply_reorientation", "transpose.py:44"):
        assert where in header  # the entry names the reference lines it replaces
    assert "tio_permute3d" not in open(os.path.join(ROOT, "oracle", "tio_oracle.c")).read()  # no CPU counterpart


def test_entry_point_refuses_bad_arguments(fn):
    call = fn["permute3d"]

    def run(x=SOME, y=OTHER, dtype=_abi.F32, batch=2, channels=2, shape=(3, 4, 5), perm=(2, 1, 0), mask=0):
        return call(x, y, dtype, batch, channels, None if shape is None else (ctypes.c_int32 * 3)(*shape),
                    None if perm is None else (ctypes.c_int32 * 3)(*perm), mask, None)

    def text():
        return fn["last_error"]()

    assert run(shape=None) == -1 and b"null shape or perm" in text()
    assert run(perm=None) == -1 and b"null shape or perm" in text()
    assert run(dtype=9) == -2 and b"dtype 9" in text()
    assert run(dtype=-1) == -2
    assert run(batch=-1) == -1 and b"negative batch" in text()
    assert run(channels=0) == -1 and b"channels must be >= 1" in text()
    for shape in ((0, 4, 5), (3, -1, 5), (3, 4, 0)):
        assert run(shape=shape) == -1 and b"shapes must be >= 1" in text()
    for perm in ((0, 0, 1), (0, 1, 3), (-1, 1, 2), (2, 2, 2), (1, 2, 1)):
        assert run(perm=perm) == -1 and b"is not a permutation of (0, 1, 2)" in text()
    for mask in (-1, 8):
        assert run(mask=mask) == -1 and b"outside 0..7" in text()
    assert run(x=None) == -1 and b"null data" in text()
    assert run(y=None) == -1 and b"null data" in text()
    # nothing to do: OK whatever the pointers are, but only after the other checks
    assert run(x=None, y=None, batch=0) == 0
    assert run(x=None, y=None, batch=0, perm=(0, 0, 0)) == -1


def test_engine_refuses_bad_arguments_before_any_launch():
    engine = ops.Engine(_lib.load()[1], "cuda", "hip")
    data = torch.zeros(2, 1, 3, 4, 5)
    with pytest.raises(ValueError, match=r"expected a \(B, C, I, J, K\) tensor"):
        engine.permute3d(data[0], (0, 1, 2))
    for perm in ((0, 1), (0, 1, 1), (1, 2, 3)):
        with pytest.raises(ValueError, match=r"perm must be a permutation of \(0, 1, 2\)"):
            engine.permute3d(data, perm)
    with pytest.raises(ValueError, match="Axis must be 0, 1, or 2; got 3"):
        engine.permute3d(data, (0, 1, 2), (3,))
    with pytest.raises(ops.EngineError, match="permute3d: tensor on cpu"):
        engine.permute3d(data, (2, 1, 0))


def test_the_classes_have_their_place_in_the_package():
    for name in ("Reorient", "Transpose", "CropOrPad", "EnsureShapeMultiple", "ToReferenceSpace", "CopyAffine"):
        assert getattr(tio.transforms, name) is getattr(tio, name) and name in tio.__all__ and name in tio.transforms.__all__
        assert _TRANSFORM_REGISTRY[name] is getattr(tio, name)  # history replay finds it by name
        assert issubclass(getattr(tio, name), tio.SpatialTransform)
    assert tio.Reorient().invertible and tio.Transpose().invertible
    assert not tio.CropOrPad(4).invertible and not tio.EnsureShapeMultiple(4).invertible  # their Pad / Crop entries are
    assert repr(tio.Reorient()) == "Reorient()" and repr(tio.Reorient("lps")) == "Reorient(orientation='LPS')"


# -- Reorient ------------------------------------------------------------------------------------------------------------
def test_reorient_validation_carries_the_reference_messages():
    for bad in ("RA", "RASS", 3, None):
        with pytest.raises(ValueError) as info:
            tio.Reorient(bad)
        assert str(info.value) == f'Orientation must be a 3-letter string, got "{bad}"'
    with pytest.raises(ValueError, match='Orientation code must be composed of three distinct characters in .* but got "RAX"'):
        tio.Reorient("rax")
    with pytest.raises(ValueError) as info:
        tio.Reorient("RLS")
    assert str(info.value) == (
        "Orientation code must include one character for each axis direction: R or L, A or P, and S or I, but got \"RLS\""
    )
    assert tio.Reorient("lps").orientation == "LPS" and tio.Reorient("sAl").orientation == "SAL"  # lower case is accepted
    assert tio.Reorient().orientation == "RAS"


def test_reorient_matches_the_reference_for_every_code_and_source(golden, on_oracle):
    """All 48 codes x 3 source affines (and the two batch cases): parameters, data through the stand-in, affines."""
    expected = golden["reorient"]
    assert len(expected) == 48 * 3 + 2
    ours = cases.run_moves(tio, cases.reorient_cases())
    assert list(ours) == list(expected)
    for name, entry in expected.items():
        assert_same(ours[name], entry, name, AFFINE_BAR)
    identity = ours["ras_anisotropic_to_RAS"]
    assert identity["params"][-1] == {"ornt": [[0.0, 1.0], [1.0, 1.0], [2.0, 1.0]], "original_orientation": "RAS"}
    assert ours["include_t1_only"]["images"]["seg"]["data"].shape[-3:] == cases.REORIENT_SHAPE  # left alone


class _Spy(_TorchPermute):
    """Notes what every ``permute3d`` call was asked to do."""

    def __init__(self, engine):
        super().__init__(engine)
        self.calls = []

    def permute3d(self, data, perm, flip_axes=()):
        self.calls.append((list(perm), list(flip_axes)))
        return super().permute3d(data, perm, flip_axes)


def test_reorient_keeps_world_positions(oracle, monkeypatch):
    """Independent of the golden file and of the restated nibabel functions: for every case and every corner voxel of the
    output, ``affine_out @ index_out == affine_in @ index_in`` with ``index_in`` worked out from perm / flip directly — the
    pair the data were moved by.  A wrong sign or a wrong centre in ``inv_ornt_aff`` moves a corner by a voxel or more."""
    spy = _Spy(oracle)
    monkeypatch.setattr(ops, "_ENGINE", spy)
    for source, affine_in in cases.SOURCE_AFFINES.items():
        for code in cases.ORIENTATIONS:
            batch = cases.batch_of(tio, [cases.subject(tio, cases.REORIENT_SHAPE, source)])
            spy.calls.clear()
            out = tio.Reorient(code)(batch)
            assert len(spy.calls) in (0, 2) and spy.calls[:1] == spy.calls[1:]  # one launch per image, none for the identity
            perm, flips = spy.calls[0] if spy.calls else ([0, 1, 2], [])
            image = out.images["t1"]
            affine_out = image.affines[0].numpy()
            assert image.affines[0].orientation == tuple(code)
            assert tuple(image.data.shape[-3:]) == tuple(cases.REORIENT_SHAPE[p] for p in perm)
            for corner in cases.corner_indices(image.data.shape[-3:]):
                index_in = cases.input_index(corner, perm, flips, cases.REORIENT_SHAPE)
                world_out, world_in = affine_out @ [*corner, 1.0], affine_in @ [*index_in, 1.0]
                assert np.abs(world_out - world_in).max() <= 1e-9, (source, code, corner)
                # and the voxel there is the one the affine says
                i, j, k = (int(v) for v in index_in)
                o = tuple(int(v) for v in corner)
                assert image.data[0, 0][o] == batch.images["t1"].data[0, 0, i, j, k]


def test_reorient_inverse_goes_back(on_oracle):
    batch = cases.batch_of(tio, [cases.subject(tio, cases.REORIENT_SHAPE, "oblique")])
    out = tio.Reorient("PIR")(batch)
    assert out.applied_transforms[-1].name == "Reorient"
    back = tio.apply_inverse_transform(out)
    for name, image in batch.images.items():
        assert torch.equal(back.images[name].data, image.data)
        assert float((back.images[name].affines[0].data - image.affines[0].data).abs().max()) <= AFFINE_BAR


# -- Transpose -----------------------------------------------------------------------------------------------------------
def test_transpose_matches_the_reference(golden, on_oracle):
    ours = cases.run_moves(tio, cases.transpose_cases())
    for name, entry in golden["transpose"].items():
        assert_same(ours[name], entry, name)
    batch = cases.batch_of(tio, [cases.subject(tio)])
    twice = tio.apply_inverse_transform(tio.Transpose(include=["t1"])(batch))  # include is not consulted: every image moves
    for name, image in batch.images.items():
        assert torch.equal(twice.images[name].data, image.data) and torch.equal(twice.images[name].affines[0].data, image.affines[0].data)


# -- CropOrPad / EnsureShapeMultiple -------------------------------------------------------------------------------------
def test_crop_or_pad_validation():
    with pytest.raises(ValueError, match="only_crop and only_pad cannot both be True"):
        tio.CropOrPad(4, only_crop=True, only_pad=True)
    with pytest.raises(ValueError, match="units must be 'voxels', 'mm', or 'cm', got 'm'"):
        tio.CropOrPad(4, units="m")
    with pytest.raises(ValueError, match="location must be 'center' or 'random', got 'corner'"):
        tio.CropOrPad(4, location="corner")
    with pytest.raises(ValueError, match="target_shape must have 1 or 3 values, got 2"):
        tio.CropOrPad((4, 4))
    with pytest.raises(ValueError, match="padding_mode must be one of"):
        tio.CropOrPad(4, padding_mode="edge")
    with pytest.raises(TypeError):
        tio.CropOrPad(4, "mm")  # keyword-only, as in the reference
    assert tio.CropOrPad((4, None, 5.0)).target_shape == (4.0, None, 5.0)
    with pytest.raises(ValueError, match="target_multiple must be >= 1, got 0"):
        tio.EnsureShapeMultiple(0)
    with pytest.raises(ValueError, match="target_multiple must have 1 or 3 values, got 2"):
        tio.EnsureShapeMultiple((2, 2))
    with pytest.raises(ValueError, match="All target_multiple values must be >= 1, got 0"):
        tio.EnsureShapeMultiple((2, 0, 2))
    with pytest.raises(ValueError, match="method must be 'crop' or 'pad', got 'both'"):
        tio.EnsureShapeMultiple(2, method="both")


def test_crop_or_pad_splits_ceil_in_front_and_floor_behind():
    from torchio_amd.transforms.orientation import _compute_crop_and_pad
    from torchio_amd.transforms.orientation import _to_voxels

    assert _compute_crop_and_pad((6, 9, 7), (9, 4, 7), only_crop=False, only_pad=False) == ((2, 1, 0, 0, 0, 0), (0, 0, 3, 2, 0, 0))
    assert _compute_crop_and_pad((6, 9, 7), (9, 4, 7), only_crop=True, only_pad=False) == (None, (0, 0, 3, 2, 0, 0))
    assert _compute_crop_and_pad((6, 9, 7), (9, 4, 7), only_crop=False, only_pad=True) == ((2, 1, 0, 0, 0, 0), None)
    assert _compute_crop_and_pad((6, 9, 7), (6, 9, 7), only_crop=False, only_pad=False) == (None, None)
    assert _to_voxels((8.0, None, 1.0), "mm", (0.8, 1.5, 2.0), (6, 9, 7)) == (10, 9, 0)
    assert _to_voxels((0.6, 1.2, 1.0), "cm", (0.8, 1.5, 2.0), (6, 9, 7)) == (8, 8, 5)  # round(7.5) is 8: half to even


@pytest.mark.parametrize("group", ["crop_or_pad", "ensure_shape_multiple"])
def test_crop_or_pad_matches_the_reference_bit_for_bit(group, golden, oracle, monkeypatch):
    """Parameters (the random draws included), outputs and affines on the CPU oracle engine, history names."""
    monkeypatch.setattr(ops, "_ENGINE", oracle)
    ours = cases.run_group(tio, group)
    assert list(ours) == list(golden[group])
    for name, entry in golden[group].items():
        assert_same(ours[name], entry, name)
    if group == "crop_or_pad":
        assert ours["subject_mixed"]["history"] == ["Pad", "Crop", "CropOrPad"]
        assert len({tuple(ours[f"random_seed{seed}"]["params"][-1]["cropping"]) for seed in (1, 2, 3)}) > 1
    else:
        assert ours["crop_below_the_multiple"]["images"]["t1"]["data"].shape[-3:] == (1, 8, 1)


@pytest.mark.parametrize("target", [(9, 12, 8), (3, 4, 6), (8, 4, 7)])
def test_crop_or_pad_inverse_restores_the_shape(target, oracle, monkeypatch):
    monkeypatch.setattr(ops, "_ENGINE", oracle)
    batch = cases.batch_of(tio, [cases.subject(tio)])
    out = tio.CropOrPad(target)(batch)
    assert tuple(out.images["t1"].data.shape[-3:]) == target
    with pytest.warns(UserWarning, match="CropOrPad is not invertible, skipping"):
        back = tio.apply_inverse_transform(out)
    for name, image in batch.images.items():
        assert back.images[name].data.shape == image.data.shape
        assert float((back.images[name].affines[0].data - image.affines[0].data).abs().max()) <= AFFINE_BAR
    subject = tio.EnsureShapeMultiple(4)(cases.subject(tio))
    assert subject.spatial_shape == (8, 12, 8)
    with pytest.warns(UserWarning, match="CropOrPad is not invertible, skipping"):
        assert subject.apply_inverse_transform().spatial_shape == cases.SHAPE


# -- ToReferenceSpace / CopyAffine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["to_reference_space", "copy_affine"])
def test_affine_only_transforms_match_the_reference(group, golden, oracle, monkeypatch):
    monkeypatch.setattr(ops, "_ENGINE", oracle)
    ours = cases.run_group(tio, group)
    for name, entry in golden[group].items():
        assert_same(ours[name], entry, name, AFFINE_BAR)


def test_from_tensor_and_the_error_texts(golden):
    ours, expected = cases.from_tensor_case(tio), golden["from_tensor"]
    assert ours["class"] == expected["class"] == "ScalarImage" and torch.equal(ours["data"], expected["data"])
    assert float((ours["affine"] - expected["affine"]).abs().max()) <= AFFINE_BAR
    with pytest.raises(TypeError) as info:
        tio.ToReferenceSpace(torch.zeros(1, 2, 2, 2))
    assert str(info.value) == "reference must be a TorchIO Image, got Tensor"
    batch = cases.batch_of(tio, [cases.subject(tio)])
    with pytest.raises(KeyError) as info:
        tio.CopyAffine("flair")(batch)
    assert info.value.args[0] == "Reference image 'flair' not found. Available: ['t1', 'seg']"
