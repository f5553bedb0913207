"""GPU: ``tio_centre_law_sums`` / ``tio_centre_draw`` / ``tio_patch_gather`` and the public road built on them.

The draw is held to the float64 numpy statement of ``patch_feed_cases.py``.  With integer-valued weights every float64
partial sum is exact in any order, so the chosen index must EQUAL ``searchsorted(cumsum(w), u * total, side="right")``; with
real-valued weights it must lie within the float64 summation bound ``n_voxels * 2^-53 * total`` of it.  The gather must equal
``torch.stack`` of the slices bit for bit.
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import patch_feed_cases as cases
import torchio_amd as tio
from torchio_amd.data.sampler import cut

pytestmark = pytest.mark.gpu

SMALL = (12, 10, 9)  # less than one segment
LARGE = (40, 33, 31)  # 40 920 voxels: 19 whole segments and one of 2 008


@pytest.fixture(autouse=True)
def _reference_mode():
    tio.set_centre_draw("reference")
    yield
    tio.set_centre_draw("reference")


def _integers(shape, seed=0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 4, shape)


def _check_exact(hip, source: torch.Tensor, weights: np.ndarray, patch, uniforms: np.ndarray, table=None):
    """Indices, corners and total of a draw with explicit uniforms equal the numpy reference; returns the indices."""
    flat = cases.masked_weights(weights, patch)
    expected, _, total = cases.draw_reference(flat, uniforms)
    draw = hip.centre_draw(source.cuda(), patch, len(uniforms), label_table=table, uniforms=torch.from_numpy(uniforms).cuda(), return_uniforms=True)
    corners, got_total, invalid = draw.on_host()
    assert got_total == total and not invalid
    assert np.array_equal(draw.uniforms.cpu().numpy(), uniforms)
    centres = draw.centres.cpu().numpy()
    assert np.array_equal(centres, expected)
    assert (flat[centres] > 0).all()
    assert np.array_equal(corners.numpy(), cases.corners_reference(expected, weights.shape, patch))
    assert np.array_equal(draw.corners.cpu().numpy(), corners.numpy())
    return centres


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8])
@pytest.mark.parametrize("shape,patch", [(SMALL, (4, 3, 1)), (SMALL, (1, 1, 1)), (LARGE, (5, 4, 3)), (LARGE, (1, 1, 1))])
def test_map_mode_integer_weights_equal_the_reference(hip, shape, patch, dtype):
    values = _integers(shape)
    weights = values.astype(np.float32)
    uniforms = cases.boundary_uniforms(cases.masked_weights(weights, patch))
    assert shape is SMALL or len(uniforms) > 2 + 37  # (some c / total land exactly on a segment boundary)
    _check_exact(hip, torch.from_numpy(values).to(dtype), weights, patch, uniforms)


@pytest.mark.parametrize("dtype", [torch.int16, torch.uint8])
@pytest.mark.parametrize("table", [[(1, 2.0), (2, 1.0), (1, 3.0), (7, 1.0)], []], ids=["duplicate_key", "empty_table"])
@pytest.mark.parametrize("shape,patch", [(SMALL, (4, 3, 1)), (LARGE, (5, 4, 3))])
def test_label_mode_integer_weights_equal_the_reference(hip, shape, patch, table, dtype):
    labels = _integers(shape, seed=3)
    weights = cases.label_weights(labels, table)
    assert not table or (weights[labels == 1] == 3.0).all()  # the later pair wins
    uniforms = cases.boundary_uniforms(cases.masked_weights(weights, patch))
    _check_exact(hip, torch.from_numpy(labels).to(dtype), weights, patch, uniforms, table=table)


def test_segment_that_begins_and_ends_in_zeros_and_weight_in_one_voxel(hip):
    # segment 3 holds weight only in its middle; segments 4 .. 6 are empty; the rest is dense
    values = _integers(LARGE, seed=5).reshape(-1)
    values[3 * cases.SEGMENT : 7 * cases.SEGMENT] = 0
    values[3 * cases.SEGMENT + 500 : 3 * cases.SEGMENT + 1500] = 2
    values = values.reshape(LARGE)
    weights = values.astype(np.float32)
    flat = cases.masked_weights(weights, (1, 1, 1))
    cdf = np.cumsum(flat)
    inside = cdf[[3 * cases.SEGMENT + 500, 3 * cases.SEGMENT + 1000, 3 * cases.SEGMENT + 1499]]
    uniforms = np.concatenate([(inside - 2.0) / cdf[-1], (inside - 1.0) / cdf[-1], inside / cdf[-1], cases.boundary_uniforms(flat)])
    centres = _check_exact(hip, torch.from_numpy(weights), weights, (1, 1, 1), uniforms)
    assert ((centres >= 3 * cases.SEGMENT + 500) & (centres < 3 * cases.SEGMENT + 1500)).sum() >= 6
    assert 7 * cases.SEGMENT in centres or (centres >= 7 * cases.SEGMENT).any()  # a draw just past the empty segments
    uniforms = np.array([0.0, 0.3, 1.0 - 2.0**-53])
    for shape in (SMALL, LARGE):
        # all the weight in the last voxel
        weights = np.zeros(shape, np.float32)
        weights[-1, -1, -1] = 3
        centres = _check_exact(hip, torch.from_numpy(weights), weights, (1, 1, 1), uniforms)
        assert (centres == weights.size - 1).all()
        # all of it in the first voxel the mask allows
        weights = np.zeros(shape, np.float32)
        weights[2, 1, 0] = 2
        weights[0, 0, 0] = weights[1, 1, 0] = weights[2, 0, 0] = 5  # (masked)
        centres = _check_exact(hip, torch.from_numpy(weights), weights, (4, 3, 1), uniforms)
        assert (centres == np.ravel_multi_index((2, 1, 0), shape)).all()


def test_real_valued_weights_stay_within_the_summation_bound(hip):
    rng = np.random.default_rng(11)
    weights = rng.random(LARGE, dtype=np.float32)
    patch = (5, 4, 3)
    uniforms = np.concatenate([[0.0, 1.0 - 2.0**-53], rng.random(4094)])
    flat = cases.masked_weights(weights, patch)
    _, cdf, total = cases.draw_reference(flat, uniforms)
    draw = hip.centre_draw(torch.from_numpy(weights).cuda(), patch, len(uniforms), uniforms=torch.from_numpy(uniforms).cuda())
    _, got_total, invalid = draw.on_host()
    centres = draw.centres.cpu().numpy()
    eps = flat.size * 2.0**-53 * total  # the float64 summation bound: derived, not measured
    assert abs(got_total - total) <= eps and not invalid
    t = uniforms * total
    before = np.where(centres > 0, cdf[np.maximum(centres - 1, 0)], 0.0)
    print("largest excursion / eps:", max((before - t).max(), (t - cdf[centres]).max()) / eps)
    assert (centres >= 0).all() and (flat[centres] > 0).all()
    assert (before - eps <= t).all() and (t < cdf[centres] + eps).all()


@pytest.fixture(scope="module")
def small_law():
    weights = np.random.default_rng(0).integers(0, 4, SMALL).astype(np.float32)
    return weights, cases.masked_weights(weights, (4, 3, 1))


@pytest.mark.parametrize("seed", [0, 1234, 2**62 - 1])
def test_own_stream_is_the_declared_philox_stream(hip, small_law, seed):
    weights, flat = small_law
    n = 65536
    draw = hip.centre_draw(torch.from_numpy(weights).cuda(), (4, 3, 1), n, seed=seed, return_uniforms=True)
    uniforms = cases.centre_uniforms(seed, n)
    assert np.array_equal(draw.uniforms.cpu().numpy().view(np.uint64), uniforms.view(np.uint64))
    assert uniforms.min() >= 0.0 and uniforms.max() < 1.0
    expected, _, _ = cases.draw_reference(flat, uniforms)
    centres = draw.centres.cpu().numpy()
    assert np.array_equal(centres, expected)
    assert np.array_equal(draw.corners.cpu().numpy(), cases.corners_reference(expected, SMALL, (4, 3, 1)))
    if seed == 1234:  # end to end: the draws follow the law
        positive = np.flatnonzero(flat > 0)
        assert len(positive) == 441
        expectation = n * flat[positive] / flat.sum()
        counts = np.bincount(centres, minlength=flat.size)[positive]
        assert counts.sum() == n and expectation.min() > 50
        statistic = float(((counts - expectation) ** 2 / expectation).sum())
        df = len(positive) - 1
        bound = df * (1 - 2 / (9 * df) + 4.7534 * np.sqrt(2 / (9 * df))) ** 3  # Wilson-Hilferty, the 1 - 1e-6 quantile
        print("chi-square", statistic, "bound", bound)
        assert statistic < bound


def _probability_subject(weights: np.ndarray) -> tio.Subject:
    return tio.Subject(prob=tio.ScalarImage(torch.from_numpy(weights.astype(np.float32))[None].cuda()))


def test_errors_of_the_device_draw(hip):
    tio.set_centre_draw("device")
    patch = (4, 3, 3)

    def sample(weights, size=patch):
        subject = _probability_subject(weights)
        return tio.WeightedSampler(subject, size, probability_map="prob").sample_batch(subject, 3)

    zeros = np.zeros(SMALL)
    with pytest.raises(RuntimeError, match="Probability map 'prob' is all zeros"):
        sample(zeros)
    border = zeros.copy()
    border[:2] = border[-2:] = 1
    border[:, 0] = border[:, -1] = border[:, :, 0] = border[:, :, -1] = 1
    with pytest.raises(RuntimeError, match="Probability map 'prob' is all zeros"):
        sample(border)
    with pytest.raises(RuntimeError, match="Probability map 'prob' is all zeros"):
        sample(np.ones(SMALL), size=(13, 3, 3))
    for bad in (-1.0, np.nan):
        inside = np.ones(SMALL)
        inside[5, 5, 4] = bad
        with pytest.raises(RuntimeError, match="probability tensor contains either"):
            sample(inside)
        masked = np.ones(SMALL)
        masked[0, 5, 4] = masked[5, 0, 4] = masked[5, 5, 8] = masked[11, 9, 8] = bad
        assert sample(masked).batch_size == 3
    # a table that was given and is empty weighs nothing (unlike no table at all: label > 0)
    subject = cases.make_subject(device="cuda")
    with pytest.raises(RuntimeError, match="Probability map 'seg' is all zeros"):
        tio.LabelSampler(subject, patch, label_name="seg", label_probabilities={}).sample_batch(subject, 2)
    assert tio.LabelSampler(subject, patch, label_name="seg").sample_batch(subject, 2).batch_size == 2


GATHER_CASES = [
    ((2, 13, 11, 10), (5, 4, 3)),
    ((2, 13, 11, 10), (13, 11, 10)),
    ((2, 13, 11, 10), (1, 1, 1)),
    ((1, 9, 8, 37), (3, 2, 1)),
    ((1, 9, 8, 37), (3, 2, 3)),
    ((1, 9, 8, 37), (3, 2, 16)),
    ((1, 9, 8, 37), (3, 2, 17)),
]
GATHER_DTYPES = [torch.uint8, torch.int16, torch.float32, torch.float64, torch.bfloat16]


def _volume(shape, dtype) -> torch.Tensor:
    count = int(np.prod(shape))
    values = torch.arange(count, dtype=torch.int64).reshape(shape)
    if dtype in (torch.uint8, torch.bfloat16):
        values = values % 251  # (every value exact in the type, neighbours differ)
    return values.to(dtype).cuda()


def _corners(shape, patch, n, seed=0) -> np.ndarray:
    limit = np.array(shape[1:]) - np.array(patch)
    rng = np.random.default_rng(seed)
    corners = rng.integers(0, limit + 1, (n, 3))
    corners[0] = 0
    if n > 1:
        corners[1] = limit
        corners[2:, 2] = np.minimum(corners[2:, 2] | 1, limit[2])  # odd k where it fits
    return corners.astype(np.int32)


def _stacked(volume, corners, patch) -> torch.Tensor:
    return torch.stack([volume[:, i : i + patch[0], j : j + patch[1], k : k + patch[2]] for i, j, k in corners.tolist()])


@pytest.mark.parametrize("shape,patch", GATHER_CASES)
def test_gather_equals_the_stack_of_slices(hip, shape, patch):
    for dtype, n in itertools.product(GATHER_DTYPES, (1, 40)):
        volume = _volume(shape, dtype)
        corners = _corners(shape, patch, n)
        for handed in (torch.from_numpy(corners), torch.from_numpy(corners).cuda()):  # staged upload / as a draw leaves them
            out = hip.patch_gather(volume, handed, patch)
            assert out.shape == (n, shape[0], *patch) and out.dtype == dtype and out.is_contiguous()
            assert torch.equal(out, _stacked(volume, corners, patch)), (dtype, n)


@pytest.mark.parametrize("dtype", GATHER_DTYPES)
def test_gather_clamps_corners_out_of_range(hip, dtype):
    shape, patch = (2, 13, 11, 10), (5, 4, 3)
    volume = _volume(shape, dtype)
    wild = np.array([[-3, -3, -3], [13, 11, 10], [-3, 5, 10], [2**31 - 1, -(2**31), 4]], dtype=np.int32)
    clamped = np.clip(wild.astype(np.int64), 0, np.array(shape[1:]) - np.array(patch))
    out = hip.patch_gather(volume, torch.from_numpy(wild), patch)
    assert torch.equal(out, _stacked(volume, clamped, patch))


def test_gather_at_working_size(hip):
    volume = torch.rand((1, 256, 256, 256), device="cuda")
    corners = np.array([[0, 0, 0], [192, 192, 192], [77, 101, 33]], dtype=np.int32)
    out = hip.patch_gather(volume, torch.from_numpy(corners), (64, 64, 64))
    assert torch.equal(out, _stacked(volume, corners, (64, 64, 64)))


def test_gather_refuses_a_patch_larger_than_the_volume(hip):
    with pytest.raises(ValueError, match="cannot be larger"):
        hip.patch_gather(_volume((1, 4, 4, 4), torch.float32), torch.zeros((1, 3), dtype=torch.int32), (5, 1, 1))


@pytest.mark.parametrize("kind", ["uniform", "weighted", "label"])
def test_sample_batch_on_the_device_equals_the_views_and_stack_road(hip, kind):
    subject = cases.make_subject(device="cuda")
    sampler = cases.samplers(subject)[kind]
    torch.manual_seed(7)
    expected = tio.SubjectsBatch.from_subjects(list(itertools.islice(sampler(subject), 6)))
    probe = torch.rand(1)
    torch.manual_seed(7)
    ours = sampler.sample_batch(subject, 6)
    assert torch.equal(torch.rand(1), probe)
    assert ours.device.type == "cuda"
    cases.assert_same_batch(ours, expected)
    # the same corners as on a host copy of the subject
    host = cases.make_subject()
    torch.manual_seed(7)
    assert cases.samplers(host)[kind].sample_batch(host, 6).metadata["patch_location"] == ours.metadata["patch_location"]


@pytest.mark.parametrize("kind", ["weighted", "label"])
def test_sample_batch_in_device_mode(hip, kind):
    subject = cases.make_subject(device="cuda")
    sampler = cases.samplers(subject)[kind]
    tio.set_centre_draw("device")
    torch.manual_seed(5)
    first = sampler.sample_batch(subject, 16)
    probe = torch.rand(1)
    torch.manual_seed(5)
    second = sampler.sample_batch(subject, 16)
    assert torch.equal(torch.rand(1), probe)
    cases.assert_same_batch(first, second)
    torch.manual_seed(6)
    assert sampler.sample_batch(subject, 16).metadata["patch_location"] != first.metadata["patch_location"]
    # the gathered data sits where patch_location says, with everything else from the slicing road
    locations = first.metadata["patch_location"]
    cases.assert_same_batch(first, tio.SubjectsBatch.from_subjects([cut(subject, where) for where in locations]))
    # every centre has positive weight (an allowed centre's corner is never clamped: centre = corner + patch // 2)
    law = sampler._law(subject).map.cpu().numpy()
    half = [p // 2 for p in sampler.patch_size]
    assert len({where.index for where in locations}) > 1
    for where in locations:
        assert where.size == sampler.patch_size
        assert law[tuple(c + h for c, h in zip(where.index, half, strict=True))] > 0
    if kind == "label":  # more labels than the kernel's table holds: the weight tensor goes over in map mode
        many = {label: 1.0 for label in range(100, 170)} | {2: 2.0}
        wide = tio.LabelSampler(subject, (5, 4, 3), label_name="seg", label_probabilities=many)
        labels = subject.images["seg"].data[0].cpu().numpy()
        for where in wide.sample_batch(subject, 8).metadata["patch_location"]:
            assert labels[tuple(c + h for c, h in zip(where.index, (2, 2, 1), strict=True))] == 2


def test_grid_batches_through_the_crop_aggregator_return_the_volume(hip):
    subject = cases.make_subject(2, device="cuda")
    grid = tio.GridSampler(subject, (6, 5, 4), patch_overlap=(2, 2, 2))
    aggregator = tio.PatchAggregator(subject.spatial_shape, "crop", patch_overlap=(2, 2, 2))
    count = 0
    for number, batch in enumerate(grid.batches(5)):
        expected = tio.SubjectsBatch.from_subjects([grid[index] for index in range(5 * number, min(5 * number + 5, len(grid)))])
        cases.assert_same_batch(batch, expected)
        aggregator.add_batch(batch.images["t1"].data, batch.metadata["patch_location"])
        count += batch.batch_size
    assert count == len(grid) and len(grid) % 5 != 0
    assert torch.equal(aggregator.get_output(), subject.images["t1"].data)


def test_queue_with_gathered_patches_does_not_pin_the_parents(hip):
    subjects = [cases.make_subject(seed, device="cuda") for seed in range(2)]
    sampler = tio.LabelSampler(subjects[0], (4, 3, 3), label_name="seg")
    queue = tio.Queue(subjects, sampler, max_length=6, patches_per_volume=3, shuffle_subjects=False, shuffle_patches=False, gather_patches=True)
    torch.manual_seed(1)
    patches = list(queue)
    assert len(patches) == 6
    parents = {image.data.untyped_storage().data_ptr() for subject in subjects for image in subject.images.values()}
    for patch in patches:
        where = patch.metadata["patch_location"]
        parent = next(s for s in subjects if s.metadata["name"] == patch.metadata["name"])
        for name, image in patch.images.items():
            assert image.data.untyped_storage().data_ptr() not in parents
            assert torch.equal(image.data, parent.images[name].data[(slice(None), *where.to_slices())])
