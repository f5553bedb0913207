"""``To`` and ``Lambda`` without a GPU: exports, constructor errors with the reference's messages, parameters, history,
non-invertibility, and the data path itself (neither transform calls the engine, so host tensors go through the public call)."""
from __future__ import annotations

import pytest
import torch

import torchio_amd as tio
from torchio_amd.transforms.transform import _TRANSFORM_REGISTRY


# Neither transform calls the engine.  Where a GPU is present the public call would stage host tensors on it and bring them
# back (transform.py: _stage_on_engine_device), which replaces every tensor; the batches live where nothing has to move.
DEVICE = "cuda" if torch.cuda.is_available() else "cpu"


def _batch():
    generator = torch.Generator().manual_seed(5)
    image = torch.randn(2, 3, 4, 5, generator=generator)
    label = torch.randint(0, 4, (1, 3, 4, 5), generator=generator).to(torch.int16)
    subjects = [tio.Subject(t1=tio.ScalarImage((image + k).to(DEVICE)), seg=tio.LabelMap((label + k).to(DEVICE))) for k in range(2)]
    return tio.SubjectsBatch.from_subjects(subjects)


def test_the_two_classes_are_exported():
    for name in ("To", "Lambda"):
        assert name in tio.__all__ and name in tio.transforms.__all__ and getattr(tio.transforms, name) is getattr(tio, name)
        assert _TRANSFORM_REGISTRY[name] is getattr(tio, name)


def test_constructor_errors_carry_the_reference_messages():
    for bad in (3, None, "negate"):
        with pytest.raises(TypeError) as info:
            tio.Lambda(bad)
        assert str(info.value) == f"function must be callable, got {type(bad).__name__}"
    assert tio.Lambda(abs).types_to_apply is None and tio.Lambda(abs, "label").types_to_apply == "label"
    assert tio.Lambda(abs, types_to_apply="scalar", p=0.5).p == 0.5
    to = tio.To("cpu", dtype=torch.float16)
    assert to.to_args == ("cpu",) and to.to_kwargs == {"dtype": torch.float16}
    assert tio.To().to_args == () and tio.To().to_kwargs == {}


def test_params_and_inverse():
    batch = _batch()
    assert tio.Lambda(abs).make_params(batch) == {}
    assert tio.To(torch.float16, non_blocking=True).make_params(batch) == {"to_args": (torch.float16,), "to_kwargs": {"non_blocking": True}}
    for transform in (tio.To("cpu"), tio.Lambda(abs)):
        assert not transform.invertible
        with pytest.raises(NotImplementedError):
            transform.inverse({})


def test_types_to_apply():
    for kind, mine, other in (("scalar", tio.ScalarImage, tio.LabelMap), ("label", tio.LabelMap, tio.ScalarImage)):
        assert tio.Lambda(abs, kind)._should_apply(mine) and not tio.Lambda(abs, kind)._should_apply(other)
    for kind in (None, "anything else"):  # as in the reference: an unknown word applies to every image
        assert tio.Lambda(abs, kind)._should_apply(tio.ScalarImage) and tio.Lambda(abs, kind)._should_apply(tio.LabelMap)


def test_the_data_path_on_host_tensors():
    batch = _batch()
    before_image, before_label = batch.images["t1"].data.clone(), batch.images["seg"].data.clone()
    out = tio.Compose([tio.To(torch.float64), tio.Lambda(lambda x: -x, types_to_apply="scalar")])(batch)
    assert out.images["t1"].data.dtype == torch.float64 and out.images["seg"].data.dtype == torch.float64
    assert torch.equal(out.images["t1"].data, -before_image.double()) and torch.equal(out.images["seg"].data, before_label.double())
    assert torch.equal(batch.images["t1"].data, before_image) and batch.images["t1"].data.dtype == torch.float32  # the input is untouched
    assert [entry.name for entry in out.applied_transforms][-2:] == ["To", "Lambda"]
    assert out.applied_transforms[-2].params == {"to_args": (torch.float64,), "to_kwargs": {}} and out.applied_transforms[-1].params == {}
    # the result is assigned INTO the element: the batch keeps its dtype, another shape is torch's own error
    kept = tio.Lambda(lambda x: (x > 1).double(), types_to_apply="label")(batch)
    assert kept.images["seg"].data.dtype == torch.int16 and torch.equal(kept.images["seg"].data, (before_label > 1).to(torch.int16))
    assert torch.equal(kept.images["t1"].data, before_image)
    with pytest.raises(RuntimeError):
        tio.Lambda(lambda x: x[:, 1:])(batch)
    # copy=False writes the tensor it is given, as the reference does
    own = tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(before_image[0].clone()))])
    pointer = own.images["t1"].data.data_ptr()
    plain = tio.Lambda(lambda x: x * 2, copy=False)(own)
    assert torch.equal(plain.images["t1"].data, before_image[:1] * 2) and plain.images["t1"].data.data_ptr() == pointer


def test_lambda_clones_only_a_tensor_the_batch_still_shares_with_the_caller():
    """Copy-on-replace (data/_lazy.py): the caller's tensor is cloned before the first in-place write; a tensor that an
    earlier transform of the same call has already replaced is the batch's own and is written where it lies."""
    batch = _batch()
    before = batch.images["t1"].data.clone()
    pointer = batch.images["t1"].data.data_ptr()
    seen = []

    def remember(x):
        seen.append(x.data_ptr())
        return x + 1

    out = tio.Lambda(remember, types_to_apply="scalar")(batch)
    assert torch.equal(batch.images["t1"].data, before) and batch.images["t1"].data.data_ptr() == pointer
    assert torch.equal(out.images["t1"].data, before + 1) and out.images["t1"].data.data_ptr() == seen[0] != pointer
    # after To has replaced the tensor (a cast), Lambda writes the cast's result in place: one allocation, not two
    seen.clear()
    out = tio.Compose([tio.To(torch.float64), tio.Lambda(remember, types_to_apply="scalar")])(batch)
    assert out.images["t1"].data.data_ptr() == seen[0] and torch.equal(out.images["t1"].data, before.double() + 1)
    assert torch.equal(batch.images["t1"].data, before)
    # a To that changes nothing hands the caller's tensor on: still cloned
    out = tio.Compose([tio.To(torch.float32), tio.Lambda(remember, types_to_apply="scalar")])(batch)
    assert torch.equal(batch.images["t1"].data, before) and out.images["t1"].data.data_ptr() != pointer
    assert not hasattr(out.images["t1"], "_borrowed_tensor") or out.images["t1"]._borrowed_tensor is None
