"""GPU: ``tio_permute3d`` against ``torch.flip`` + ``permute`` + ``contiguous`` on the device, bit for bit, on shapes that
put tile edges on every axis; the slow grid dimension beyond 65535; element offsets beyond 2^31; the six classes against the
golden file of the unmodified reference (``tests/golden/make_golden_orientation.py``); inverse and backward."""
from __future__ import annotations

import os

import pytest
import torch

import orientation_cases as cases
import torchio_amd as tio
from orientation_cases import AFFINE_BAR
from orientation_cases import assert_same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orientation_golden.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def _flips(mask: int) -> list[int]:
    return [axis for axis in range(3) if mask & (1 << axis)]


# -- the kernel ----------------------------------------------------------------------------------------------------------
def test_permute3d_is_the_aten_sequence_bit_for_bit(hip):
    """6 permutations x 8 flip masks x element sizes 1 / 2 / 4 / 8 on every shape; one list of everything that differs."""
    wrong = []
    shapes = [((2, 2), shape) for shape in cases.PERMUTE_SHAPES] + [((1, 1), cases.PERMUTE_SHAPE_ONE_ELEMENT)]
    for dtype in cases.PERMUTE_DTYPES:
        for leading, shape in shapes:
            data = cases.distinct((*leading, *shape), dtype, "cuda")
            for perm in cases.PERMUTATIONS:
                for mask in range(8):
                    out = hip.permute3d(data, perm, _flips(mask))
                    expected = cases.aten_permute(data, perm, mask)
                    if out.shape != expected.shape or out.dtype != dtype or not torch.equal(out, expected):
                        wrong.append((str(dtype), shape, perm, mask))
    assert not wrong, f"{len(wrong)} of {4 * len(shapes) * 48} launches differ, first {wrong[:8]}"


@pytest.mark.parametrize("shape, perm", [((70000, 2, 2), (0, 2, 1)), ((2, 70000, 2), (2, 1, 0))], ids=["r_is_axis0", "r_is_axis1"])
def test_slow_dimension_beyond_65535(hip, shape, perm):
    """The untiled axis times B * C exceeds what ``gridDim.y`` / ``gridDim.z`` hold: it is part of the linear tile index."""
    data = cases.distinct((1, 1, *shape), torch.float32, "cuda")
    for mask in (0, 7):
        assert torch.equal(hip.permute3d(data, perm, _flips(mask)), cases.aten_permute(data, perm, mask))


def test_element_offsets_beyond_2_to_31(hip):
    shape = (1025, 1024, 2048)  # 2^31 + 2^21 one-byte elements
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 1024**3:
        pytest.skip(f"needs 8 GB of free device memory, {free / 1024**3:.1f} GB are free")
    i, j, k = (torch.arange(extent, device="cuda") for extent in shape)
    data = ((i * 7 % 251).to(torch.uint8)[:, None, None] + (j * 13 % 241).to(torch.uint8)[None, :, None]
            + (k * 31 % 239).to(torch.uint8)[None, None, :])[None, None]  # (uint8 sums wrap: still a function of the position)
    assert data.numel() > 2**31 and data.dtype == torch.uint8
    expected = torch.flip(data, [2, 3, 4]).permute(0, 1, 4, 3, 2).contiguous()
    out = hip.permute3d(data, (2, 1, 0), (0, 1, 2))
    assert torch.equal(out, expected)
    assert out[0, 0, -1, -1, -1] == data[0, 0, 0, 0, 0] and out[0, 0, 0, 0, 0] == data[0, 0, -1, -1, -1]


@pytest.mark.parametrize("perm, flips", [((1, 2, 0), (0, 2)), ((2, 1, 0), (1,))])
def test_backward_is_autograds(hip, perm, flips):
    """The adjoint of a permutation with flips, exactly: gradients are moved, never added."""
    shape = (2, 2, 5, 33, 7)
    generator = torch.Generator().manual_seed(3)
    data = torch.randn(shape, generator=generator).cuda()
    ours, theirs = data.clone().requires_grad_(), data.clone().requires_grad_()
    out = hip.permute3d(ours, perm, flips)
    expected = cases.aten_permute(theirs, perm, sum(1 << axis for axis in flips))
    assert torch.equal(out.detach(), expected.detach())
    weight = torch.randn(out.shape, generator=generator).cuda()
    (out * weight).sum().backward()
    (expected * weight).sum().backward()
    assert torch.equal(ours.grad, theirs.grad)


# -- the classes ---------------------------------------------------------------------------------------------------------
def test_reorient_and_transpose_match_the_reference(hip, golden):
    """Every golden case on the device: data bit for bit (one ``permute3d`` launch per image), affines, history."""
    ours = cases.run_moves(tio, cases.reorient_cases("cuda"))
    assert list(ours) == list(golden["reorient"])
    for name, entry in golden["reorient"].items():
        assert_same(ours[name], entry, name, AFFINE_BAR)
    ours = cases.run_moves(tio, cases.transpose_cases("cuda"))
    for name, entry in golden["transpose"].items():
        assert_same(ours[name], entry, name)


@pytest.mark.parametrize("group", ["crop_or_pad", "ensure_shape_multiple"])
def test_crop_or_pad_matches_the_reference_on_the_hip_engine(hip, golden, group):
    ours = cases.run_group(tio, group, "cuda")
    assert list(ours) == list(golden[group])
    for name, entry in golden[group].items():
        assert_same(ours[name], entry, name)


def test_inverse_of_a_pipeline_goes_back_to_the_input(hip):
    """Reorient, a CropOrPad that pads two axes and keeps one, a flip: undone newest first, the data come back bit for bit and
    the affines within the float64 margin."""
    batch = cases.batch_of(tio, [cases.subject(tio, affine="oblique"), cases.subject(tio, affine="oblique", shift=4)], "cuda")
    pipeline = tio.Compose([tio.Reorient("LPS"), tio.CropOrPad((11, 8, 9)), tio.Flip(axes=(0,))])
    out = pipeline(batch)
    assert tuple(out.images["t1"].data.shape[-3:]) == (11, 8, 9) and out.images["t1"].affines[0].orientation == ("L", "P", "S")
    reoriented = tio.Reorient("LPS")(batch)
    with pytest.warns(UserWarning, match="CropOrPad is not invertible, skipping"):
        back = tio.apply_inverse_transform(out)
    plain = tio.apply_inverse_transform(reoriented)
    for name, image in batch.images.items():
        assert torch.equal(back.images[name].data, image.data) and torch.equal(plain.images[name].data, image.data)
        for restored, original in zip(back.images[name].affines, image.affines, strict=True):
            assert float((restored.data - original.data).abs().max()) <= AFFINE_BAR


def test_the_pipeline_of_the_readme_runs_on_a_device_batch(hip):
    batch = cases.batch_of(tio, [cases.subject(tio, (20, 24, 18), "lps")], "cuda")
    out = tio.Compose([tio.Reorient(), tio.CropOrPad(24), tio.Affine(degrees=5.0)])(batch)
    assert out.images["t1"].data.shape == (1, 2, 24, 24, 24) and out.images["t1"].data.is_cuda
    assert out.images["t1"].affines[0].orientation == ("R", "A", "S")
