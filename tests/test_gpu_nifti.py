"""GPU: ``tio_nifti_decode`` and the file roads built on it, bit for bit against ``nifti_cases.expected_tensor`` (numpy's restatement
of the format rules, plus ONE ``astype`` for the converted outputs): shapes that put tile edges on both tiled axes and the
degenerate routes, every disk type x byte order x scaling x output type, batches, guard-banded destinations, the batch road of
``SubjectsBatch.from_subjects(device="cuda")`` with its single launch, ``Image.save`` of device tensors, and a Compose fed from
files."""
from __future__ import annotations

import gzip

import numpy as np
import pytest
import torch

import guarded_memory
import nifti_cases as cases
import torchio_amd as tio
from torchio_amd import ops

pytestmark = pytest.mark.gpu

EDGE_SHAPE = (65, 3, 66)  # one full tile plus a 1-wide (i) and a 2-wide (k) edge tile
SHAPES = [EDGE_SHAPE, (64, 2, 64), (130, 1, 7), (7, 5, 1), (1, 4, 9), (4, 4, 4)]
OUT_DTYPES = {None: None, "f4": torch.float32, "f8": torch.float64}


def _upload(payload: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(payload), dtype=torch.uint8).cuda()


def _decode(hip, payload: bytes, code: int, shape, *, channels=1, batch=1, big_endian=False, scaled=False, out=None) -> torch.Tensor:
    return hip.nifti_decode(_upload(payload), disk_type=code, shape=shape, channels=channels, batch=batch, swap_bytes=big_endian,
                            slope=cases.SLOPE32 if scaled else None, inter=cases.INTER32, out_dtype=OUT_DTYPES[out])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_route_and_tile_edge(hip, shape):
    """int16, float32 and uint64 (2-, 4- and 8-byte cells; a promoted type), two channels, both byte orders."""
    wrong = []
    for code in (4, 16, 1280, 2):
        for big_endian in (False, True):
            payload = cases.payload_bytes(cases.volume(code, shape, channels=2), big_endian)
            got = _decode(hip, payload, code, shape, channels=2, big_endian=big_endian)
            expected = cases.expected_tensor(payload, code, shape, 2, big_endian=big_endian)
            if got.shape != (1, 2, *shape) or not cases.same_bits(got[0].cpu(), expected):
                wrong.append((code, big_endian))
    assert wrong == []


@pytest.mark.parametrize("code", sorted(cases.DISK_TYPES))
def test_every_type_order_scaling_and_output_in_one_rounding(hip, code):
    """The sweep at the edge shape.  The 64-bit integer inputs hold values near 2^53 and 2^63 at which a conversion through
    float64 and one straight to float32 differ (checked below on the host), so a double rounding cannot pass."""
    array = cases.volume(code, EDGE_SHAPE)
    if cases.DISK_TYPES[code] in ("i8", "u8"):
        assert (array.astype("f4") != array.astype("f8").astype("f4")).sum() >= 2  # the inputs do tell the two apart
    wrong = []
    for big_endian in (False, True):
        payload = cases.payload_bytes(array, big_endian)
        for scaled in (False, True):
            for out in (None, "f4", "f8"):
                got = _decode(hip, payload, code, EDGE_SHAPE, big_endian=big_endian, scaled=scaled, out=out)
                expected = cases.expected_tensor(payload, code, EDGE_SHAPE, big_endian=big_endian, scaled=scaled, out=out)
                if not cases.same_bits(got[0].cpu(), expected):
                    wrong.append((big_endian, scaled, out, str(got.dtype)))
    assert wrong == []


def test_unsupported_outputs_are_refused(hip):
    payload = cases.payload_bytes(cases.volume(4, (4, 4, 4)), False)
    for kwargs in ({"out_dtype": torch.float16}, {"out_dtype": torch.int32}, {"out_dtype": torch.int16, "slope": 2.0}):
        with pytest.raises(ops.EngineError, match="tio_nifti_decode"):
            hip.nifti_decode(_upload(payload), disk_type=4, shape=(4, 4, 4), **kwargs)
    with pytest.raises(ValueError, match="at least"):
        hip.nifti_decode(_upload(payload)[:-1], disk_type=4, shape=(4, 4, 4))
    with pytest.raises(ops.EngineError, match="tensor on cpu"):
        hip.nifti_decode(torch.zeros(128, dtype=torch.uint8), disk_type=4, shape=(4, 4, 4))


def test_batches_of_channels_equal_the_single_decodes_stacked(hip):
    shape, channels, batch = (65, 3, 66), 3, 3
    for code, scaled, out in ((4, True, "f4"), (512, False, None), (64, False, "f4")):
        payloads = [cases.payload_bytes(cases.volume(code, shape, channels=channels, seed=index), True) for index in range(batch)]
        got = _decode(hip, b"".join(payloads), code, shape, channels=channels, batch=batch, big_endian=True, scaled=scaled, out=out)
        singles = [_decode(hip, payload, code, shape, channels=channels, big_endian=True, scaled=scaled, out=out)[0] for payload in payloads]
        assert got.shape == (batch, channels, *shape) and cases.same_bits(got, torch.stack(singles))
        expected = torch.stack([cases.expected_tensor(p, code, shape, channels, big_endian=True, scaled=scaled, out=out) for p in payloads])
        assert cases.same_bits(got.cpu(), expected)
        assert not cases.same_bits(got[0], got[1])  # distinct contents per element


@pytest.mark.parametrize("code, scaled, out", [(16, True, None), (2, False, None), (1280, False, "f8"), (4, False, None)], ids=str)
def test_destination_between_guards(hip, code, scaled, out):
    """float64 and uint8 (and int16) outputs at the edge shape inside ``0xFF`` guards: every guard byte stays intact."""
    payload = cases.payload_bytes(cases.volume(code, EDGE_SHAPE, channels=2), False)
    arena = guarded_memory.Arena()
    with guarded_memory.guarded_engine_allocations(arena):
        got = _decode(hip, payload, code, EDGE_SHAPE, channels=2, scaled=scaled, out=out)
    torch.cuda.synchronize()
    assert arena.owns(got)
    arena.check_guards()
    assert cases.same_bits(got[0].cpu(), cases.expected_tensor(payload, code, EDGE_SHAPE, 2, scaled=scaled, out=out))


# -- the public road -------------------------------------------------------------------------------------------------------
def _subjects(tmp_path, specs, shape=(24, 24, 24)):
    """One subject per ``(code, big_endian, scaled)`` in *specs*, files from the struct builder; and the expected tensors."""
    subjects, expected = [], []
    for index, (code, big_endian, scaled) in enumerate(specs):
        array = cases.volume(code, shape, seed=index)
        content = cases.file_bytes(array, code, big_endian=big_endian, scaled=scaled)
        path = tmp_path / f"subject{index}{'.nii.gz' if index % 2 else '.nii'}"
        cases.write_file(path, content)
        subjects.append(tio.Subject(t1=tio.ScalarImage(path), name=f"s{index}"))
        expected.append(cases.expected_tensor(content[352:], code, shape, big_endian=big_endian, scaled=scaled))
    return subjects, expected


@pytest.fixture
def decode_calls(monkeypatch):
    calls = []
    real = ops.Engine.nifti_decode

    def counted(self, raw, **kwargs):
        calls.append(kwargs["batch"])
        return real(self, raw, **kwargs)

    monkeypatch.setattr(ops.Engine, "nifti_decode", counted)
    return calls


def test_a_homogeneous_group_is_stacked_by_one_launch(hip, tmp_path, decode_calls):
    subjects, expected = _subjects(tmp_path, [(4, False, True)] * 3)
    batch = tio.SubjectsBatch.from_subjects(subjects, device="cuda")
    assert decode_calls == [3]  # ONE launch wrote the stacked tensor
    assert batch.t1.data.is_cuda and batch.t1.data.shape == (3, 1, 24, 24, 24) and batch.metadata["name"] == ["s0", "s1", "s2"]
    assert all(not subject.t1.is_loaded for subject in subjects)
    assert cases.same_bits(batch.t1.data.cpu(), torch.stack(expected))
    per_image = torch.stack([tio.ScalarImage(subject.t1.path).load(device="cuda").data for subject in subjects])
    assert per_image.is_cuda and cases.same_bits(batch.t1.data, per_image)
    on_host = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(subject.t1.path)) for subject in subjects])
    assert not on_host.t1.data.is_cuda and cases.same_bits(batch.t1.data, on_host.to("cuda").t1.data)
    for affine, subject in zip(batch.t1.affines, subjects, strict=True):
        assert torch.equal(affine.data, subject.t1.affine.data)
    as_float = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage.from_file(s.t1.path, dtype=torch.float32)) for s in subjects], device="cuda")
    assert cases.same_bits(as_float.t1.data.cpu(), torch.from_numpy(torch.stack(expected).numpy().astype("f4")))  # float64 scaled values, one rounding


def test_a_mixed_group_falls_back_to_per_image_loads(hip, tmp_path, decode_calls):
    subjects, expected = _subjects(tmp_path, [(4, False, False), (4, True, False), (4, False, False)])  # one file is big-endian
    batch = tio.SubjectsBatch.from_subjects(subjects, device="cuda")
    assert decode_calls == [1, 1, 1]
    assert batch.t1.data.is_cuda and cases.same_bits(batch.t1.data.cpu(), torch.stack(expected))
    loaded = [tio.Subject(t1=tio.ScalarImage(subject.t1.path).load()) for subject in subjects]  # already on the host: moved, not decoded again
    del decode_calls[:]
    moved = tio.SubjectsBatch.from_subjects(loaded, device="cuda")
    assert decode_calls == [] and cases.same_bits(moved.t1.data, batch.t1.data)


def test_lazy_images_decode_where_they_are_sent(hip, tmp_path, decode_calls):
    subjects, expected = _subjects(tmp_path, [(512, True, False)], shape=(65, 3, 66))
    image = subjects[0].t1
    assert image.to("cuda") is image and not image.is_loaded and image.device.type == "cuda"
    crop = image[:, 60:, 1:, 3:66]
    assert not image.is_loaded and crop.data.is_cuda and cases.same_bits(crop.data.cpu(), expected[0][:, 60:, 1:, 3:66].contiguous())
    assert image.data.is_cuda and image.is_loaded and cases.same_bits(image.data.cpu(), expected[0])
    assert decode_calls == [1, 1]
    subject = tio.Subject(t1=tio.ScalarImage(image.path), label=tio.LabelMap(image.path)).load(device="cuda")
    assert subject.t1.data.is_cuda and subject.label.data.is_cuda and cases.same_bits(subject.label.data.cpu(), expected[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.uint8, torch.bfloat16], ids=str)
def test_saving_a_device_tensor(hip, tmp_path, dtype):
    affine = np.array([[0.0, -2.0, 0.0, 5.0], [1.5, 0.0, 0.0, 6.0], [0.0, 0.0, 3.0, 7.0], [0.0, 0.0, 0.0, 1.0]])
    for channels in (1, 2):
        generator = torch.Generator().manual_seed(channels)
        host = (torch.randn((channels, 65, 3, 66), generator=generator) * 50).to(dtype)
        path = tmp_path / f"saved{channels}.nii.gz"
        tio.ScalarImage(host.cuda(), affine=affine).save(path)
        fields = cases.raw_reparse(gzip.open(path).read())
        stored = host.to(torch.float32) if dtype == torch.bfloat16 else host
        assert fields["channels"] == channels and fields["dim"][1:4] == (65, 3, 66) and fields["intent_code"] == (1007 if channels > 1 else 0)
        assert cases.same_bits(torch.from_numpy(fields["voxels"]), stored)
        np.testing.assert_allclose(fields["srow"], affine[:3], rtol=0, atol=1e-6)
        assert cases.same_bits(tio.ScalarImage(path).load(device="cuda").data.cpu(), stored)


def test_a_compose_fed_from_files_equals_the_same_compose_fed_from_tensors(hip, tmp_path):
    subjects, expected = _subjects(tmp_path, [(4, False, False)] * 2)
    affines = [subject.t1.affine.data.clone() for subject in subjects]
    transform = tio.Compose([tio.Affine(degrees=5), tio.Noise()])
    from_files = tio.SubjectsBatch.from_subjects(subjects, device="cuda")
    from_tensors = tio.SubjectsBatch.from_subjects(
        [tio.Subject(t1=tio.ScalarImage(tensor, affine=affine), name=f"s{index}") for index, (tensor, affine) in enumerate(zip(expected, affines, strict=True))]
    ).to("cuda")
    assert from_files.t1.data.dtype == torch.int16
    torch.manual_seed(31)
    got = transform(from_files)
    torch.manual_seed(31)
    want = transform(from_tensors)
    torch.cuda.synchronize()
    assert got.t1.data.is_cuda and cases.same_bits(got.t1.data, want.t1.data)
    assert not cases.same_bits(got.t1.data.cpu().to(torch.float32), torch.stack(expected).to(torch.float32))  # the transforms did something
    for a, b in zip(got.t1.affines, want.t1.affines, strict=True):
        assert torch.equal(a.data, b.data)
