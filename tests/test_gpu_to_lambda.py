"""GPU: ``tio.To`` and ``tio.Lambda`` on device-resident batches: dtype cast and history through a ``Compose``, the
assignment into the element, and the callable seeing finished values after a transform that defers its launch."""
from __future__ import annotations

import pytest
import torch

import torchio_amd as tio

pytestmark = pytest.mark.gpu


def _scalar_and_label():
    generator = torch.Generator().manual_seed(5)
    image = torch.randn(2, 6, 7, 8, generator=generator)
    label = torch.randint(0, 4, (1, 6, 7, 8), generator=generator).to(torch.int16)
    subjects = [tio.Subject(t1=tio.ScalarImage((image + k).to("cuda")), seg=tio.LabelMap((label + k).to("cuda"))) for k in range(2)]
    return tio.SubjectsBatch.from_subjects(subjects)


def test_to_and_lambda_in_a_compose(hip):
    batch = _scalar_and_label()
    before_image, before_label = batch.images["t1"].data.clone(), batch.images["seg"].data.clone()
    out = tio.Compose([tio.To(torch.float16), tio.Lambda(lambda x: -x, types_to_apply="scalar")])(batch)
    assert out.images["t1"].data.dtype == torch.float16 and out.images["seg"].data.dtype == torch.float16
    assert out.images["t1"].data.device.type == "cuda"
    assert torch.equal(out.images["t1"].data, -before_image.to(torch.float16))
    assert torch.equal(out.images["seg"].data, before_label.to(torch.float16))
    assert torch.equal(batch.images["t1"].data, before_image) and batch.images["t1"].data.dtype == torch.float32  # the input is untouched
    history = out.applied_transforms
    assert [entry.name for entry in history][-2:] == ["To", "Lambda"]
    assert history[-2].params == {"to_args": (torch.float16,), "to_kwargs": {}} and history[-1].params == {}


def test_to_moves_between_devices(hip):
    batch = _scalar_and_label()
    home = tio.To("cpu")(batch)
    assert home.images["t1"].data.device.type == "cpu" and home.images["seg"].data.device.type == "cpu"
    assert torch.equal(home.images["t1"].data, batch.images["t1"].data.cpu())
    assert batch.images["t1"].data.device.type == "cuda"


def test_lambda_keeps_the_dtype_and_refuses_another_shape(hip):
    batch = _scalar_and_label()
    seen = []
    out = tio.Lambda(lambda x: (seen.append((x.device.type, tuple(x.shape))), (x > 1).double())[1], types_to_apply="label")(batch)
    assert seen == [("cuda", (1, 6, 7, 8))] * 2  # each element's (C, I, J, K) device tensor
    assert out.images["seg"].data.dtype == torch.int16
    assert torch.equal(out.images["seg"].data, (batch.images["seg"].data > 1).to(torch.int16))
    assert torch.equal(out.images["t1"].data, batch.images["t1"].data)
    with pytest.raises(RuntimeError):
        tio.Lambda(lambda x: x[:, 1:])(batch)


def test_lambda_never_writes_the_callers_tensor(hip):
    """Inside the copy-on-replace scope the batch's tensor is still the caller's: the assignment goes into a private copy."""
    batch = _scalar_and_label()
    before = batch.images["t1"].data.clone()
    pointer = batch.images["t1"].data.data_ptr()
    out = tio.Lambda(lambda x: x * 0 + 7)(batch)
    assert torch.equal(batch.images["t1"].data, before) and batch.images["t1"].data.data_ptr() == pointer
    assert bool((out.images["t1"].data == 7).all()) and out.images["t1"].data.data_ptr() != pointer


def test_lambda_after_a_lazy_stage_sees_the_finished_data(hip):
    batch = _scalar_and_label()
    seen = []

    def record(x):
        seen.append(x.clone())
        return x

    out = tio.Compose([tio.Flip(axes=(0,)), tio.Lambda(record, types_to_apply="scalar")])(batch)
    flipped = torch.flip(batch.images["t1"].data, dims=(2,))
    assert len(seen) == 2 and all(torch.equal(seen[k], flipped[k]) for k in range(2))
    assert torch.equal(out.images["t1"].data, flipped)
    # Blur queues its stencil on the batch instead of launching it: the callable must see the blurred values
    seen.clear()
    blurred = tio.Blur(std=1.0)(batch).images["t1"].data
    assert not torch.equal(blurred, batch.images["t1"].data)
    out = tio.Compose([tio.Blur(std=1.0), tio.Lambda(record, types_to_apply="scalar")])(batch)
    assert len(seen) == 2 and all(torch.allclose(seen[k], blurred[k], rtol=0, atol=1e-5) for k in range(2))
    assert torch.allclose(out.images["t1"].data, blurred, rtol=0, atol=1e-5)
