"""NIfTI-1 reading and writing on the host (no GPU): header parse, the three affine branches, refusals, lazy attributes, the numpy
decode against ``nifti_cases.expected_tensor`` bit for bit, the writer re-parsed with ``struct``, the argument checks of
``tio_nifti_decode``, and the public entry points built on them.  Files come from ``nifti_cases`` (``struct.pack`` +
``tobytes(order="F")``), never from the library's writer, except where the writer is what is tested."""
from __future__ import annotations

import copy
import ctypes
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import nifti_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.data import nifti

SHAPE = (5, 3, 4)


def _write(tmp_path, name, array, code, **kwargs) -> tuple[Path, bytes]:
    content = cases.file_bytes(array, code, **kwargs)
    path = tmp_path / name
    cases.write_file(path, content)
    return path, content


# -- header ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_endian", [False, True])
def test_header_parse_of_hand_built_files(tmp_path, big_endian):
    array = cases.volume(4, SHAPE, channels=3)
    path, _ = _write(tmp_path, "x.nii", array, 4, big_endian=big_endian, scaled=True, vox_offset=352.0)
    header = nifti.read_header(path)
    assert header.big_endian is big_endian and header.datatype == 4 and header.shape == SHAPE and header.channels == 3
    assert header.vox_offset == 352 and header.scaled and header.element_bytes == 2
    assert (header.slope, header.inter) == (cases.SLOPE32, cases.INTER32)
    assert header.natural_dtype == torch.float64 and header.payload_bytes == 3 * 60 * 2
    np.testing.assert_array_equal(header.affine, np.vstack([cases.SHEAR_AFFINE[:3].astype(np.float32).astype(np.float64), [0, 0, 0, 1]]))
    image = tio.ScalarImage(path)
    assert image.shape == (3, *SHAPE) and image.spatial_shape == SHAPE and image.num_channels == 3 and image.dtype == torch.float64
    assert image.path == path and not image.is_loaded


def test_scaling_applies_only_for_finite_nonzero_slopes_other_than_the_identity(tmp_path):
    array = cases.volume(4, SHAPE)
    for index, (slope, inter, scaled) in enumerate([(0.0, 5.0, False), (1.0, 0.0, False), (float("nan"), 1.0, False), (float("inf"), 0.0, False),
                                                    (1.0, 2.0, True), (2.0, 0.0, True), (-1.0, 0.0, True)]):
        path, content = _write(tmp_path, f"s{index}.nii", array, 4, slope=slope, inter=inter)
        image = tio.ScalarImage(path)
        assert nifti.read_header(path).scaled is scaled and image.dtype == (torch.float64 if scaled else torch.int16)
        expected = cases.expected_array(content[352:], 4, SHAPE, 1, big_endian=False, scaling=(slope, inter) if scaled else None)
        assert cases.same_bits(image.data, torch.from_numpy(expected))


def test_affine_from_an_sform_with_shear(tmp_path):
    path, _ = _write(tmp_path, "sform.nii", cases.volume(2, SHAPE), 2, sform_code=1, srow=tuple(cases.SHEAR_AFFINE[:3].reshape(-1)),
                     qform_code=1, quatern=(0.5, 0.5, 0.5), pixdim=(1.0, 9.0, 9.0, 9.0, 1, 1, 1, 1))  # the sform wins over a qform
    np.testing.assert_array_equal(tio.ScalarImage(path).affine.data.numpy(), cases.SHEAR_AFFINE)  # (every entry is a float32 value)


def test_affine_from_a_qform_rotated_by_90_degrees_with_negative_qfac(tmp_path):
    # 90 degrees about the third axis: (a, b, c, d) = (cos 45, 0, 0, sin 45); zooms (2, 3, 4), qfac -1, offset (10, -20, 30)
    half = float(np.sqrt(0.5))
    path, _ = _write(tmp_path, "qform.nii", cases.volume(2, SHAPE), 2, qform_code=1, quatern=(0.0, 0.0, half), qoffset=(10.0, -20.0, 30.0),
                     pixdim=(-1.0, 2.0, 3.0, 4.0, 1, 1, 1, 1))
    # R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; columns scaled by 2, 3 and 4 * (-1)
    by_hand = np.array([[0.0, -3.0, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, -4.0, 30.0], [0.0, 0.0, 0.0, 1.0]])
    np.testing.assert_allclose(tio.ScalarImage(path).affine.data.numpy(), by_hand, rtol=0, atol=1e-6)
    # qfac is -1 only for pixdim[0] == -1
    path, _ = _write(tmp_path, "qform0.nii", cases.volume(2, SHAPE), 2, qform_code=1, quatern=(0.0, 0.0, half), qoffset=(10.0, -20.0, 30.0),
                     pixdim=(0.0, 2.0, 3.0, 4.0, 1, 1, 1, 1))
    by_hand[2, 2] = 4.0
    np.testing.assert_allclose(tio.ScalarImage(path).affine.data.numpy(), by_hand, rtol=0, atol=1e-6)


def test_affine_with_neither_form(tmp_path):
    path, _ = _write(tmp_path, "none.nii", cases.volume(2, SHAPE), 2, qform_code=0, sform_code=0, pixdim=(1.0, 2.0, 3.0, 0.5, 1, 1, 1, 1))
    by_hand = np.array([[-2.0, 0, 0, 2.0 * (5 - 1) / 2], [0, 3.0, 0, -3.0 * (3 - 1) / 2], [0, 0, 0.5, -0.5 * (4 - 1) / 2], [0, 0, 0, 1.0]])
    np.testing.assert_array_equal(tio.ScalarImage(path).affine.data.numpy(), by_hand)


def test_refusals_name_their_cause(tmp_path):
    array = cases.volume(2, SHAPE)
    refusals = [
        ({"sizeof_hdr": 540}, "sizeof_hdr"),
        ({"magic": b"ni1\0"}, "magic"),
        ({"magic": b"n+2\0"}, "magic"),
    ]
    for index, (fields, word) in enumerate(refusals):
        path, _ = _write(tmp_path, f"bad{index}.nii", array, 2, **fields)
        with pytest.raises(ValueError, match=word):
            tio.ScalarImage(path)
    for code in (1, 32, 128, 1536, 1792, 2048, 2304, 0):  # binary, complex64, RGB, float128, complex128, complex256, RGBA, unknown
        path = tmp_path / f"type{code}.nii"
        cases.write_file(path, cases.header_bytes(dim=[3, *SHAPE], datatype=code) + bytes(4 + 60 * 16))
        with pytest.raises(ValueError, match=f"datatype {code}"):
            tio.ScalarImage(path)
    for index, dim in enumerate(([2, 5, 3], [5, 5, 3, 4, 2, 2], [6, 5, 3, 4, 1, 1, 2])):
        path = tmp_path / f"dim{index}.nii"
        cases.write_file(path, cases.header_bytes(dim=dim, datatype=2) + bytes(4 + 1000))
        with pytest.raises(ValueError, match="expected 3D, 4D"):
            tio.ScalarImage(path)
    with pytest.raises(ValueError, match="only .nii and .nii.gz"):
        tio.ScalarImage(tmp_path / "scan.nrrd")
    short = tmp_path / "short.nii"
    cases.write_file(short, cases.file_bytes(array, 2)[:-5])
    with pytest.raises(ValueError, match="promises"):
        tio.ScalarImage(short).load()


def test_nii_and_nii_gz_hold_the_same_image(tmp_path):
    array = cases.volume(16, SHAPE, channels=2)
    plain, _ = _write(tmp_path, "x.nii", array, 16, big_endian=True)
    zipped, _ = _write(tmp_path, "x.nii.gz", array, 16, big_endian=True)
    a, b = tio.ScalarImage(plain), tio.ScalarImage(zipped)
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.affine.data, b.affine.data)
    assert cases.same_bits(a.data, b.data)


# -- lazy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lazy.nii", "lazy.nii.gz"])
def test_header_attributes_do_not_load(tmp_path, monkeypatch, name):
    array = cases.volume(4, (20, 30, 40), channels=2)
    path, content = _write(tmp_path, name, array, 4)
    inflated, staged = [], []
    real_inflate, real_staging = nifti._inflate, nifti._new_staging
    monkeypatch.setattr(nifti, "_inflate", lambda *args, **kwargs: inflated.append(len(out := real_inflate(*args, **kwargs))) or out)
    monkeypatch.setattr(nifti, "_new_staging", lambda nbytes, pinned: staged.append(nbytes) or real_staging(nbytes, pinned))
    image = tio.ScalarImage(path)
    subject = tio.Subject(t1=image)
    assert image.path == path and image.shape == (2, 20, 30, 40) and image.spatial_shape == (20, 30, 40) and image.num_channels == 2
    assert image.dtype == torch.int16 and image.spacing == pytest.approx(tuple(np.linalg.norm(cases.SHEAR_AFFINE[:3, :3], axis=0)))
    assert image.affine.data.shape == (4, 4) and image.device == torch.device("cpu")
    assert subject.shape == (2, 20, 30, 40) and subject.spatial_shape == (20, 30, 40)
    assert image.to("cpu") is image and repr(image) and not copy.deepcopy(image).is_loaded and not copy.deepcopy(subject).t1.is_loaded
    assert not image.is_loaded and staged == []
    assert inflated == ([348] if name.endswith(".gz") else [])  # no more than the header was inflated (and once)
    data = image.data
    assert image.is_loaded and image.data is data and staged == [len(content) - 352]  # loads once, caches
    assert cases.same_bits(data, cases.expected_tensor(content[352:], 4, (20, 30, 40), 2))
    other = tio.Subject(t1=tio.ScalarImage(path), label=tio.LabelMap(path))
    assert other.load() is other and other.t1.is_loaded and other.label.is_loaded


@pytest.mark.parametrize("code", [1024, 1280])
def test_dtype_and_destination_are_recorded_until_the_load(tmp_path, code):
    """``dtype=`` float32 / float64 is one rounding from the exact disk value (uint64 beyond 2^63 included), as on the device."""
    array = cases.volume(code, SHAPE)
    path, content = _write(tmp_path, "x.nii", array, code)
    image = tio.ScalarImage.from_file(path, dtype=torch.float32, note="kept")
    assert isinstance(image, tio.ScalarImage) and image.dtype == torch.float32 and image["note"] == "kept" and not image.is_loaded
    assert cases.same_bits(image.data, cases.expected_tensor(content[352:], code, SHAPE, out="f4"))
    later = tio.read_image(path, image_class=tio.LabelMap).to(torch.float64)
    assert isinstance(later, tio.LabelMap) and not later.is_loaded and later.dtype == torch.float64
    assert cases.same_bits(later.data, cases.expected_tensor(content[352:], code, SHAPE, out="f8"))
    as_half = tio.ScalarImage.from_file(path, dtype=torch.float16)  # any other dtype: a cast of the natural result
    assert as_half.dtype == torch.float16 and torch.equal(as_half.data, cases.expected_tensor(content[352:], code, SHAPE).to(torch.float16))
    own_affine = tio.ScalarImage.from_file(str(path), affine=np.diag([2.0, 2.0, 2.0, 1.0]))
    assert own_affine.spacing == (2.0, 2.0, 2.0)


@pytest.mark.parametrize("name", ["crop.nii", "crop.nii.gz"])
def test_getitem_on_an_unloaded_image_reads_the_box_only(tmp_path, monkeypatch, name):
    array = cases.volume(512, (20, 30, 40), channels=2)
    path, _ = _write(tmp_path, name, array, 512, scaled=True, big_endian=True)
    staged = []
    real_staging = nifti._new_staging
    monkeypatch.setattr(nifti, "_new_staging", lambda nbytes, pinned: staged.append(nbytes) or real_staging(nbytes, pinned))
    image = tio.ScalarImage(path)
    crop = image[1, 3:9, :, 10:-5]
    assert not image.is_loaded and crop.is_loaded and crop.shape == (1, 6, 30, 25)
    assert staged == [1 * 6 * 30 * 25 * 2]  # the box, not the volume, went through staging
    loaded = tio.ScalarImage(path).load()
    assert cases.same_bits(crop.data, loaded.data[1:2, 3:9, :, 10:-5].contiguous())
    expected_origin = loaded.affine.data[:3, 3] + loaded.affine.data[:3, :3] @ torch.tensor([3.0, 0.0, 10.0], dtype=torch.float64)
    assert torch.equal(crop.affine.data[:3, 3], expected_origin) and torch.equal(crop.affine.data[:3, :3], loaded.affine.data[:3, :3])
    assert torch.equal(loaded[1, 3:9, :, 10:-5].affine.data, crop.affine.data)
    strided = image[:, ::2]  # a strided crop loads the image and slices it
    assert image.is_loaded and cases.same_bits(strided.data.contiguous(), loaded.data[:, ::2].contiguous())


# -- values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("big_endian", [False, True], ids=["native", "swapped"])
@pytest.mark.parametrize("code", sorted(cases.DISK_TYPES))
def test_host_decode_is_the_restated_rule_bit_for_bit(tmp_path, code, big_endian, scaled):
    array = cases.volume(code, SHAPE)
    path, content = _write(tmp_path, "x.nii", array, code, big_endian=big_endian, scaled=scaled)
    expected = cases.expected_tensor(content[352:], code, SHAPE, big_endian=big_endian, scaled=scaled)
    got = tio.ScalarImage(path).data
    assert got.shape == (1, *SHAPE) and cases.same_bits(got, expected)
    if not scaled:  # the expectation itself: the volume as built, promoted
        assert cases.same_bits(expected[0], torch.from_numpy(array.astype(cases.PROMOTED[cases.DISK_TYPES[code]])))


@pytest.mark.parametrize("code", [4, 16, 1280])
def test_host_decode_of_channels(tmp_path, code):
    for channels, five_d in ((3, False), (2, True)):
        array = cases.volume(code, SHAPE, channels=channels)
        path, content = _write(tmp_path, f"c{channels}.nii.gz", array, code, five_d=five_d, big_endian=True)
        got = tio.ScalarImage(path).data
        assert got.shape == (channels, *SHAPE)
        assert cases.same_bits(got, cases.expected_tensor(content[352:], code, SHAPE, channels, big_endian=True))
        for channel in range(channels):
            assert cases.same_bits(got[channel], torch.from_numpy(array[..., channel].astype(cases.PROMOTED[cases.DISK_TYPES[code]])))


# -- writer ----------------------------------------------------------------------------------------------------------------
WRITE_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]
WRITTEN_CODE = {torch.float32: 16, torch.float64: 64, torch.float16: 16, torch.bfloat16: 16, torch.uint8: 2, torch.int8: 256, torch.int16: 4,
                torch.int32: 8, torch.int64: 1024}
# a rotation (about (1, 2, 3), 40 degrees) times zooms, third axis mirrored: the determinant is negative
_AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
_CROSS = np.array([[0, -_AXIS[2], _AXIS[1]], [_AXIS[2], 0, -_AXIS[0]], [-_AXIS[1], _AXIS[0], 0]])
_ROTATION = np.eye(3) + np.sin(np.deg2rad(40)) * _CROSS + (1 - np.cos(np.deg2rad(40))) * _CROSS @ _CROSS
WRITE_AFFINE = np.eye(4)
WRITE_AFFINE[:3, :3] = _ROTATION @ np.diag([0.8, 1.25, -2.5])
WRITE_AFFINE[:3, 3] = [12.5, -40.0, 7.75]


def _tensor_of(dtype: torch.dtype, channels: int) -> torch.Tensor:
    generator = torch.Generator().manual_seed(5)
    if dtype.is_floating_point:
        return (torch.randn((channels, *SHAPE), generator=generator, dtype=torch.float64) * 100).to(dtype)
    info = torch.iinfo(dtype)
    return torch.randint(info.min, info.max, (channels, *SHAPE), generator=generator, dtype=torch.int64).to(dtype)


@pytest.mark.parametrize("dtype", WRITE_DTYPES, ids=str)
def test_writer_round_trip(tmp_path, dtype):
    for channels, name in ((1, "w.nii"), (2, "w.nii.gz")):
        tensor = _tensor_of(dtype, channels)
        path = tmp_path / name
        tio.write_nifti(path, tensor, WRITE_AFFINE)
        content = cases.gzip.open(path).read() if name.endswith(".gz") else path.read_bytes()
        fields = cases.raw_reparse(content)
        assert fields["sizeof_hdr"] == 348 and fields["magic"] == b"n+1\0" and fields["extension"] == b"\0\0\0\0" and fields["vox_offset"] == 352.0
        assert fields["datatype"] == WRITTEN_CODE[dtype] and fields["bitpix"] == 8 * np.dtype(cases.DISK_TYPES[WRITTEN_CODE[dtype]]).itemsize
        assert (fields["slope"], fields["inter"], fields["xyzt_units"], fields["qform_code"], fields["sform_code"]) == (1.0, 0.0, 2, 2, 2)
        if channels == 1:
            assert fields["dim"][:4] == (3, *SHAPE) and fields["intent_code"] == 0
        else:
            assert fields["dim"][:6] == (5, *SHAPE, 1, 2) and fields["intent_code"] == 1007
        stored = tensor.to(torch.float32) if dtype in (torch.float16, torch.bfloat16) else tensor
        assert fields["payload_size"] == stored.numel() * stored.element_size()
        assert cases.same_bits(torch.from_numpy(fields["voxels"]), stored)
        np.testing.assert_allclose(fields["srow"], WRITE_AFFINE[:3], rtol=0, atol=1e-6)
        # the quaternion (with qfac and the zooms of pixdim) reproduces the rotation part
        qfac, zooms = fields["pixdim"][0], np.array(fields["pixdim"][1:4])
        assert qfac == -1.0
        np.testing.assert_allclose(zooms, [0.8, 1.25, 2.5], rtol=0, atol=1e-6)
        rebuilt = cases.quaternion_rotation(*fields["quatern"]) * (zooms * [1, 1, qfac])
        np.testing.assert_allclose(rebuilt, WRITE_AFFINE[:3, :3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(fields["qoffset"], WRITE_AFFINE[:3, 3], rtol=0, atol=1e-6)
        # and through the library's reader
        back = tio.ScalarImage(path)
        assert cases.same_bits(back.data, stored)
        np.testing.assert_allclose(back.affine.data.numpy(), WRITE_AFFINE, rtol=0, atol=1e-6)


def test_writer_refusals_and_image_save(tmp_path):
    with pytest.raises(TypeError, match="bool"):
        tio.write_nifti(tmp_path / "b.nii", torch.zeros((1, 2, 2, 2), dtype=torch.bool), np.eye(4))
    image = tio.ScalarImage(_tensor_of(torch.int16, 2), affine=WRITE_AFFINE)
    with pytest.raises(ValueError, match="only .nii and .nii.gz"):
        image.save(tmp_path / "x.nrrd")
    image.save(tmp_path / "saved.nii.gz", compresslevel=6)
    back = tio.ScalarImage(tmp_path / "saved.nii.gz")
    assert cases.same_bits(back.data, image.data)
    np.testing.assert_allclose(back.affine.data.numpy(), WRITE_AFFINE, rtol=0, atol=1e-6)
    identity = tio.ScalarImage(_tensor_of(torch.uint8, 1))
    identity.save(tmp_path / "identity.nii")
    fields = cases.raw_reparse((tmp_path / "identity.nii").read_bytes())
    assert fields["quatern"] == (0.0, 0.0, 0.0) and fields["pixdim"][:4] == (1.0, 1.0, 1.0, 1.0)


# -- the C ABI -------------------------------------------------------------------------------------------------------------
def test_nifti_decode_validates_its_arguments_without_a_gpu():
    _, f = _lib.load()
    assert "nifti_decode" in _abi.HIP_ONLY_PROTOTYPES and "nifti_decode" not in _abi.PROTOTYPES and "tio_nifti_decode" in _abi.HIP_SYMBOLS
    assert f["abi_version"]() == 18
    buffer = (ctypes.c_double * 64)()  # 16-byte aligned, large enough for every call below
    raw, out = ctypes.cast(buffer, ctypes.c_void_p), ctypes.cast(ctypes.byref(buffer, 256), ctypes.c_void_p)

    def layout(**fields):
        values = {"disk_type": 4, "swap_bytes": 0, "shape": (ctypes.c_int32 * 3)(2, 2, 2), "channels": 1, "scaled": 0, "slope": 1.0, "inter": 0.0}
        values.update(fields)
        return ctypes.byref(_abi.NiftiLayout(**values))

    def refused(status, word, *args):
        assert f["nifti_decode"](*args) == status, f["last_error"]()
        assert b"tio_nifti_decode" in f["last_error"]() and word in f["last_error"](), f["last_error"]()

    refused(-1, b"null", raw, out, _abi.I16, 1, None, None)
    refused(-1, b"null", None, out, _abi.I16, 1, layout(), None)
    refused(-1, b"null", raw, None, _abi.I16, 1, layout(), None)
    refused(-1, b"channels", raw, out, _abi.I16, 1, layout(channels=0), None)
    refused(-1, b"channels", raw, out, _abi.I16, 1, layout(channels=-3), None)
    refused(-1, b"disk_type", raw, out, _abi.I16, 1, layout(disk_type=3), None)
    refused(-1, b"disk_type", raw, out, _abi.F32, 1, layout(disk_type=32), None)
    refused(-1, b"shape", raw, out, _abi.I16, 1, layout(shape=(ctypes.c_int32 * 3)(2, 0, 2)), None)
    refused(-1, b"batch", raw, out, _abi.I16, -1, layout(), None)
    refused(-1, b"aligned", ctypes.c_void_p(raw.value + 2), out, _abi.I16, 1, layout(), None)
    refused(-2, b"out_type", raw, out, _abi.F16, 1, layout(), None)
    refused(-2, b"out_type", raw, out, _abi.I32, 1, layout(), None)  # int16 on disk: int16, float32 or float64
    refused(-2, b"out_type", raw, out, _abi.I16, 1, layout(scaled=1, slope=2.0), None)  # scaled: float64 or float32
    refused(-2, b"out_type", raw, out, 9, 1, layout(), None)
    assert f["nifti_decode"](raw, out, _abi.I16, 0, layout(), None) == 0  # an empty batch: nothing to do


# -- public entry points ---------------------------------------------------------------------------------------------------
def test_a_string_is_still_not_image_data_but_a_path_is(tmp_path):
    with pytest.raises(TypeError, match="Image data must be a tensor or ndarray, got str") as caught:
        tio.ScalarImage("x.nii")
    assert "from_file" in str(caught.value) and "pathlib.Path" in str(caught.value)
    path, _ = _write(tmp_path, "x.nii.gz", cases.volume(2, SHAPE), 2)
    assert tio.ScalarImage(path).shape == (1, *SHAPE) and tio.LabelMap(path).dtype == torch.uint8
    with pytest.raises(FileNotFoundError):
        tio.ScalarImage(tmp_path / "missing.nii")


def test_batches_of_file_backed_subjects_on_the_host(tmp_path):
    subjects, tensors = [], []
    for index in range(3):
        array = cases.volume(4, SHAPE, seed=index)
        path, content = _write(tmp_path, f"s{index}.nii", array, 4)
        subjects.append(tio.Subject(t1=tio.ScalarImage(path), index=index))
        tensors.append(cases.expected_tensor(content[352:], 4, SHAPE))
    batch = tio.SubjectsBatch.from_subjects(subjects)
    assert cases.same_bits(batch.t1.data, torch.stack(tensors)) and batch.metadata["index"] == [0, 1, 2]
    again = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(s.t1.path)) for s in subjects], device="cpu")
    assert cases.same_bits(again.t1.data, torch.stack(tensors))


def test_resample_takes_its_target_space_from_a_file_header(tmp_path, monkeypatch):
    """A 10^3 image at 1 mm resampled onto a 6^3 / 2 mm file: the output takes the file's shape and affine, and the file's
    voxels are never read."""
    target_affine = np.diag([2.0, 2.0, 2.0, 1.0])
    content = cases.file_bytes(np.zeros((6, 6, 6), dtype=np.float32), 16, sform_code=1, srow=tuple(target_affine[:3].reshape(-1)))
    staged = []
    monkeypatch.setattr(nifti, "_new_staging", lambda *args: staged.append(args) or pytest.fail("the target's voxels were read"))
    from torchio_amd.transforms import spatial

    batch = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(torch.rand(1, 10, 10, 10)))])
    first_affine = batch.t1.affines[0]
    for name in ("target.nii", "target.nii.gz"):
        path = tmp_path / name
        cases.write_file(path, content)
        for target in (path, str(path)):
            shape, affine = spatial._resolve_target_space(target, batch, (10, 10, 10), first_affine)
            assert shape == (6, 6, 6) and np.array_equal(affine.data.numpy(), target_affine)
            assert tio.Resample(target=target).target == target
    assert staged == []
    shape, _ = spatial._resolve_target_space("t1", batch, (10, 10, 10), first_affine)  # an image name still wins
    assert shape == (10, 10, 10)
    for unknown in ("nope", str(tmp_path / "missing.nii"), tmp_path / "missing.nii.gz"):
        with pytest.raises(ValueError, match="Unknown target"):
            spatial._resolve_target_space(unknown, batch, (10, 10, 10), first_affine)


def test_struct_builder_restates_the_offsets():
    """The builder the other tests rest on, checked against the offsets written out once more."""
    raw = cases.header_bytes(dim=[3, 7, 8, 9], datatype=512, big_endian=True, slope=2.0, inter=3.0, qform_code=1, sform_code=2, vox_offset=352.0)
    assert len(raw) == 348 and struct.unpack_from(">i", raw, 0)[0] == 348 and struct.unpack_from(">4h", raw, 40) == (3, 7, 8, 9)
    assert struct.unpack_from(">hh", raw, 70) == (512, 16) and struct.unpack_from(">3f", raw, 108) == (352.0, 2.0, 3.0)
    assert struct.unpack_from(">hh", raw, 252) == (1, 2) and raw[344:] == b"n+1\0" and raw[123] == 2
    assert struct.unpack_from("<h", raw, 40)[0] == 768  # read little-endian, dim[0] is out of 1..7: that is how readers tell
