"""No GPU: the interface of the patch feed — ``sample_batch``, ``GridSampler.batches``, ``Queue(gather_patches=True)``,
``set_centre_draw`` — on host-resident subjects, where it must equal the views-and-stack road it abbreviates and consume
the global CPU generator identically; and the three new entry points in the ctypes table and the header."""
from __future__ import annotations

import itertools
import os
import random
import re

import pytest
import torch

import torchio_amd as tio
from patch_feed_cases import assert_same_batch
from patch_feed_cases import make_subject
from patch_feed_cases import samplers
from torchio_amd import _abi
from torchio_amd.data.sampler import cut

ENTRY_POINTS = ("centre_law_sums", "centre_draw", "patch_gather")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tio_hip.h")


@pytest.fixture(autouse=True)
def _reference_mode():
    tio.set_centre_draw("reference")
    yield
    tio.set_centre_draw("reference")


def test_entry_points_are_declared_and_the_abi_version_stays():
    assert _abi.ABI_VERSION == 18
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define TIO_ABI_VERSION 18" in text
    for name in ENTRY_POINTS:
        assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
        assert re.search(rf"\bint tio_{name}\s*\(", text), name
    assert f"#define TIO_CENTRE_SEGMENT {_abi.CENTRE_SEGMENT}" in text and _abi.CENTRE_SEGMENT >= 256
    assert f"#define TIO_CENTRE_MAX_LABELS {_abi.CENTRE_MAX_LABELS}" in text and _abi.CENTRE_MAX_LABELS == 64


def test_entry_points_validate_without_a_gpu():
    from torchio_amd import _lib

    _, f = _lib.load()
    i32x3 = _abi.C.c_int32 * 3
    buffer = _abi.C.create_string_buffer(4096)
    p = _abi.C.c_void_p(_abi.C.addressof(buffer))
    q = _abi.C.c_void_p(_abi.C.addressof(buffer) + 2048)
    assert f["patch_gather"](p, q, 4, 1, i32x3(4, 4, 4), i32x3(5, 1, 1), p, 1, None) == -1  # TIO_ERR_INVALID_ARGUMENT, nothing launched
    assert b"tio_patch_gather" in f["last_error"]() and b"larger than the volume" in f["last_error"]()
    assert f["patch_gather"](p, q, 3, 1, i32x3(4, 4, 4), i32x3(1, 1, 1), p, 1, None) == -2
    assert f["patch_gather"](p, q, 4, 1, i32x3(4, 4, 4), i32x3(1, 0, 1), p, 1, None) == -1
    assert f["centre_law_sums"](p, 99, 0, None, None, 0, i32x3(4, 4, 4), i32x3(1, 1, 1), q, q, None) == -2
    assert b"tio_centre_law_sums" in f["last_error"]()
    assert f["centre_law_sums"](p, _abi.I16, 1, None, None, 65, i32x3(4, 4, 4), i32x3(1, 1, 1), q, q, None) == -1
    assert f["centre_draw"](p, _abi.F32, 0, None, None, 0, i32x3(4, 4, 4), i32x3(1, 1, 1), q, q, -1, 0, None, None, q, q, None) == -1
    assert b"tio_centre_draw" in f["last_error"]()


def test_set_centre_draw_refuses_other_words():
    assert tio.get_centre_draw() == "reference"
    tio.set_centre_draw("device")
    assert tio.get_centre_draw() == "device"
    for word in ("gpu", "", "Reference", None):
        with pytest.raises(ValueError, match="centre draw mode"):
            tio.set_centre_draw(word)
    assert tio.get_centre_draw() == "device"


@pytest.mark.parametrize("kind", ["uniform", "weighted", "label"])
def test_sample_batch_is_the_collated_iteration_and_consumes_the_generator_alike(kind):
    subject = make_subject()
    sampler = samplers(subject)[kind]
    torch.manual_seed(7)
    expected = tio.SubjectsBatch.from_subjects(list(itertools.islice(sampler(subject), 6)))
    probe = torch.rand(1)
    torch.manual_seed(7)
    ours = sampler.sample_batch(subject, 6)
    assert torch.equal(torch.rand(1), probe)
    assert ours.batch_size == 6
    assert_same_batch(ours, expected)
    locations = ours.metadata["patch_location"]
    again = tio.SubjectsBatch.from_subjects([cut(subject, where) for where in locations])
    assert_same_batch(ours, again)
    assert ours.metadata["name"] == ["case0"] * 6 and all(where.size == sampler.patch_size for where in locations)


def test_grid_batches_are_the_collated_items_with_a_short_last_batch():
    subject = make_subject(1)
    grid = tio.GridSampler(subject, (6, 5, 4), patch_overlap=(0, 0, 2))
    assert len(grid) % 3 != 0
    batches = list(grid.batches(3))
    assert [b.batch_size for b in batches] == [3] * (len(grid) // 3) + [len(grid) % 3]
    for number, batch in enumerate(batches):
        expected = tio.SubjectsBatch.from_subjects([grid[index] for index in range(3 * number, min(3 * number + 3, len(grid)))])
        assert_same_batch(batch, expected)
    with pytest.raises(ValueError):
        next(grid.batches(0))


def _queue_patches(gather: bool):
    subjects = [make_subject(seed) for seed in range(3)]
    sampler = tio.LabelSampler(subjects[0], (4, 3, 3), label_name="seg")
    queue = tio.Queue(subjects, sampler, max_length=8, patches_per_volume=4, gather_patches=gather)
    torch.manual_seed(3)
    random.seed(3)
    return list(queue)


def test_queue_with_gathered_patches_hands_out_the_same_patches():
    def key(patch):
        return (patch.metadata["name"], patch.metadata["patch_location"].index)

    plain, gathered = _queue_patches(False), _queue_patches(True)
    assert len(plain) == len(gathered) == 12
    assert sorted(map(key, plain)) == sorted(map(key, gathered))
    for ours, theirs in zip(sorted(gathered, key=key), sorted(plain, key=key), strict=True):
        assert ours.metadata["patch_location"] == theirs.metadata["patch_location"]
        for name in theirs.images:
            assert torch.equal(ours.images[name].data, theirs.images[name].data)
            assert torch.equal(ours.images[name].affine.data, theirs.images[name].affine.data)
    assert tio.Queue([], None).gather_patches is False  # the default stays the views


@pytest.mark.parametrize("kind", ["weighted", "label"])
def test_device_mode_refuses_a_host_subject(kind):
    subject = make_subject()
    tio.set_centre_draw("device")
    with pytest.raises(RuntimeError, match="draws on the GPU"):
        samplers(subject)[kind].sample_batch(subject, 2)
    # iteration stays the reference's road, and so does the uniform sampler
    assert len(list(itertools.islice(samplers(subject)[kind](subject), 2))) == 2
    assert samplers(subject)["uniform"].sample_batch(subject, 2).batch_size == 2
