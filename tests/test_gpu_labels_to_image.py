"""GPU: ``Engine.labels_to_image`` and the ``LabelsToImage`` transform.

Fused mode is held bit for bit against a composition of torch ops on the device from ``Engine.philox_normal`` (the same
stream by contract); reference mode against the unmodified reference's recorded outputs
(``tests/golden/labels_to_image_golden.pt``); the transform in philox mode by its structure and its statistics."""
from __future__ import annotations

import math
import os

import pytest
import torch

import labels_to_image_cases as cases
import torchio_amd as tio

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labels_to_image_golden.pt")
LDS_KEYS = 2048  # the kernel's cap on keys staged in LDS (csrc/labels_to_image.hip: kLdsKeys); beyond it the search reads global memory
DTYPES = [torch.uint8, torch.int8, torch.int16, torch.int32, torch.float32, torch.float64]
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


@pytest.fixture
def noise_rng():
    """Sets the source of draws for one test and puts the process's choice back."""
    before = tio.get_noise_rng()
    yield tio.set_noise_rng
    tio.set_noise_rng(before)


def composed(hip, labels, keys, means, stds, seed):
    """``where(found, mean_k + std_k * z, 0)`` in float32 torch ops on the device (two kernels: two roundings)."""
    device = labels.device
    batch = labels.shape[0]
    z = hip.philox_normal((batch, 1, *labels.shape[2:]), seed, 0, device)
    value = labels[:, :1].double().contiguous()  # exact for every dtype here
    keys_t = torch.tensor([float(k) for k in keys], dtype=torch.float64, device=device)
    index = torch.searchsorted(keys_t, value).clamp(max=len(keys) - 1)
    found = keys_t[index] == value
    mean_t = torch.tensor(means, dtype=torch.float32, device=device)
    std_t = torch.tensor(stds, dtype=torch.float32, device=device)
    if mean_t.ndim == 2:
        flat = index.reshape(batch, -1)
        mean_k, std_k = mean_t.gather(1, flat).reshape(index.shape), std_t.gather(1, flat).reshape(index.shape)
    else:
        mean_k, std_k = mean_t[index], std_t[index]
    product = std_k * z
    return torch.where(found, mean_k + product, torch.zeros_like(z))


def _values(dtype):
    """Label values of a map, and which of them are keys: negative labels where the dtype has them, one value without a key,
    a non-integer one in the floating maps."""
    if dtype == torch.uint8:
        return [0, 1, 2, 5, 200, 255], [0, 1, 2, 200, 255]
    if dtype.is_floating_point:
        return [-3.0, 0.0, 1.0, 1.5, 2.0, 7.0, 100.0], [-3, 0, 1, 2, 100]
    return [-128 if dtype == torch.int8 else -3, 0, 1, 2, 7, 100], [-128 if dtype == torch.int8 else -3, 0, 1, 2, 100]


def _parameters(n_keys, batch, batched, zero_at):
    generator = torch.Generator().manual_seed(n_keys + 7 * batch + int(batched))
    rows = batch if batched else 1
    means = (torch.rand(rows, n_keys, generator=generator) * 2 - 0.5).tolist()
    stds = (torch.rand(rows, n_keys, generator=generator) * 0.2 + 0.01).tolist()
    for row in range(rows):  # one key whose mean and deviation are both zero: the reference's `continue`
        means[row][zero_at] = stds[row][zero_at] = 0.0
    return (means, stds) if batched else (means[0], stds[0])


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 1, 7, 5, 9), (2, 2, 4, 4, 4)], ids=ids)
def test_fused_mode_is_the_philox_composition_bit_for_bit(hip, shape, dtype, batched):
    values, keys = _values(dtype)
    spatial = shape[2:]
    elements = [cases.label_volume(spatial, values, shift) for shift in range(shape[0])]
    labels = torch.stack(elements).to(dtype)
    if shape[1] == 2:  # a second channel full of a label with a very different mean: it must not show
        labels = torch.cat([labels, torch.full_like(labels, keys[-1])], dim=1)
    means, stds = _parameters(len(keys), shape[0], batched, zero_at=2)
    for row in (means if batched else [means]):
        row[-1] = 1000.0
    if shape[1] == 2:  # (channel 0 then holds no voxel of that label)
        labels[:, 0][labels[:, 0] == keys[-1]] = keys[0]
    labels = labels.cuda()
    seed = 1234 + shape[0]
    out = hip.labels_to_image(labels, keys, means, stds, seed=seed)
    expected = composed(hip, labels, keys, means, stds, seed)
    assert out.shape == (shape[0], 1, *spatial) and out.dtype == torch.float32 and out.device == labels.device
    assert torch.equal(out.view(torch.int32), expected.view(torch.int32))
    if shape[1] == 2:
        assert float(out.abs().max()) < 100.0
    no_key = torch.isin(labels[:, :1].double(), torch.tensor([float(k) for k in (*[v for v in values if v not in keys], keys[2])], dtype=torch.float64).cuda())
    assert bool((out[no_key].view(torch.int32) == 0).all())  # +0.0: no key, or a key of zero mean and deviation
    if math.prod(shape) > 1:
        assert bool(no_key.any()) and bool((out[~no_key] != 0).all())


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
def test_fused_mode_searches_global_memory_beyond_the_lds_cap(hip, batched):
    shape, n_keys = (1, 1, 3, 5, 67), LDS_KEYS + 1
    keys = [3 * j - 1000 for j in range(n_keys)]
    n = math.prod(shape)
    spread = torch.tensor(keys, dtype=torch.int32)[(torch.arange(n) * 37) % n_keys]  # labels all over the keys ...
    spread[::11] += 1                                                                 # ... and some between two keys
    spread[0], spread[1] = keys[0], keys[-1]
    labels = spread.reshape(shape).cuda()
    means, stds = _parameters(n_keys, 1, batched, zero_at=5)
    out = hip.labels_to_image(labels, keys, means, stds, seed=99)
    expected = composed(hip, labels, keys, means, stds, 99)
    assert torch.equal(out.view(torch.int32), expected.view(torch.int32))
    zero = ~torch.isin(labels, torch.tensor(keys, dtype=torch.int32).cuda()) | (labels == keys[5])  # no key, or the key of zero mean and deviation
    assert torch.equal(out == 0, zero) and int(zero.sum()) >= len(range(0, n, 11)) - 1 and int((~zero).sum()) > n // 2
    # the same keys, one fewer: the LDS road gives the same voxels wherever the dropped key is not the label
    fewer = hip.labels_to_image(labels, keys[:-1], means[0][:-1] if batched else means[:-1], stds[0][:-1] if batched else stds[:-1], seed=99)
    kept = labels != keys[-1]
    assert torch.equal(fewer[kept], out[kept]) and bool((fewer[~kept] == 0).all())


def test_one_label_mode_touches_its_own_voxels_only(hip):
    labels = torch.stack([cases.label_volume((7, 5, 9), [0, 1, 2, 3], s) for s in range(2)]).to(torch.int16).cuda()
    base = torch.randn(2, 1, 7, 5, 9, generator=torch.Generator().manual_seed(5)).cuda()
    before = torch.full((2, 1, 7, 5, 9), 7.0, device="cuda")
    out = before.clone()
    result = hip.labels_to_image(labels, [0, 1, 2, 3], [[0.5, 0.25, 0.125, 1.0], [0.5, -0.25, 0.125, 1.0]], [[0.1, 0.2, 0.3, 0.4]] * 2, base=base, base_key=1,
                                 out=out)
    assert result is out
    mask = labels == 1
    sign = torch.tensor([1.0, -1.0], device="cuda").reshape(2, 1, 1, 1, 1)
    expected = torch.where(mask, base * 0.2 + 0.25 * sign, before)
    assert torch.equal(out.view(torch.int32), expected.view(torch.int32))
    fresh = hip.labels_to_image(labels, [0, 1, 2, 3], [0.5, 0.25, 0.125, 1.0], [0.1, 0.2, 0.3, 0.4], base=base, base_key=3)  # out=None: zeros
    assert torch.equal(fresh, torch.where(labels == 3, base * 0.4 + 1.0, torch.zeros_like(base)))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_reference_mode_reproduces_the_reference(name, golden, hip, noise_rng):
    """The whole call on a device-resident batch under the fixture's seed: output, parameters, history name and the global
    generator's next draw are the reference's."""
    noise_rng("reference")
    entry = golden[name]
    out, params, history_name, after = cases.run_case(tio, name, device="cuda")
    image = out.images[cases.IMAGE_KEY]
    assert params == entry["params"] and history_name == entry["name"] == "LabelsToImage"
    assert image.data.is_cuda and image.data.dtype == torch.float32 and image.data.shape == entry["out"].shape
    assert torch.equal(image.data.cpu().view(torch.int32), entry["out"].view(torch.int32))
    assert float(after) == entry["after"]
    assert torch.equal(out.images["seg"].data.cpu(), entry["labels"]) and list(out.images) == ["t1", "seg", cases.IMAGE_KEY]


def _label_batch(shape, values, dtype, count):
    subjects = []
    for shift in range(count):
        affine = torch.eye(4, dtype=torch.float64)
        affine[0, 3] = 10.0 + shift
        subjects.append(tio.Subject(seg=tio.LabelMap(cases.label_volume(shape, values, shift).to(dtype), affine=affine)))
    return tio.SubjectsBatch.from_subjects(subjects).to("cuda")


def test_transform_in_philox_mode(hip, noise_rng):
    noise_rng("philox")
    shape, values = (12, 10, 18), [0, 1, 2, 3]
    batch = _label_batch(shape, values, torch.int16, 2)
    transform = tio.LabelsToImage(image_key="synthetic", ignore_background=True)
    torch.manual_seed(21)
    out = transform(batch)
    assert list(out.images) == ["seg", "synthetic"] and "synthetic" not in batch.images  # the input batch is copied
    image, seg = out.images["synthetic"], out.images["seg"]
    assert image._image_class is tio.ScalarImage and image.data.shape == (2, 1, *shape) and image.data.dtype == torch.float32 and image.data.is_cuda
    assert torch.equal(seg.data, batch.images["seg"].data)
    for ours, theirs in zip(image.affines, seg.affines, strict=True):
        assert ours is not theirs and torch.equal(torch.as_tensor(ours.data), torch.as_tensor(theirs.data))
    record = out.applied_transforms[-1]
    assert record.name == "LabelsToImage" and record.params["_batched_keys"] == ["means", "stds"]
    assert bool((image.data[seg.data == 0].view(torch.int32) == 0).all())  # ignore_background: exactly +0.0
    # per label and element, the sample mean of `count` draws of N(mean, std) lies within 6 std / sqrt(count) of the mean
    # (probability 2e-9 per comparison to miss; the seed is fixed, so the test is deterministic); the sample deviation of
    # 250 and more draws lies within 6 std / sqrt(2 count) of std
    for b in range(2):
        for label in values[1:]:
            mean, std = record.params["means"][b][label], record.params["stds"][b][label]
            voxels = image.data[b][seg.data[b] == label].double()
            count = voxels.numel()
            assert count >= 250 and std > 0
            assert abs(float(voxels.mean()) - mean) <= 6 * std / math.sqrt(count)
            assert abs(float(voxels.std()) - std) <= 6 * std / math.sqrt(2 * count)
    torch.manual_seed(21)
    again = transform(batch)
    assert again.applied_transforms[-1].params == record.params
    assert torch.equal(again.images["synthetic"].data.view(torch.int32), image.data.view(torch.int32))
    torch.manual_seed(22)
    assert not torch.equal(transform(batch).images["synthetic"].data, image.data)


def test_pipeline_with_blur_and_bias_field(hip, noise_rng):
    noise_rng("philox")
    batch = _label_batch((16, 12, 20), [0, 1, 2, 3, 4], torch.uint8, 2)
    before = batch.images["seg"].data.clone()
    pipeline = tio.Compose([tio.LabelsToImage(label_key="seg"), tio.Blur(std=1.0), tio.BiasField()])
    torch.manual_seed(3)
    out = pipeline(batch)
    image = out.images["image_from_labels"].data
    assert image.shape == (2, 1, 16, 12, 20) and image.dtype == torch.float32 and bool(torch.isfinite(image).all()) and float(image.std()) > 0
    assert out.images["seg"].data.dtype == torch.uint8 and torch.equal(out.images["seg"].data, before) and torch.equal(batch.images["seg"].data, before)
    assert [record.name for record in out.applied_transforms][-3:] == ["LabelsToImage", "Blur", "BiasField"]
