"""GPU: the label-map kernels and the six classes, bit for bit (``torch.equal``) against analytic constructions, the torch-CPU
restatements of ``label_cases.py`` and the golden file made from the reference (``tests/golden/labels_golden.pt``).

Shapes: the smallest that cross what can break — K below / above the 64-voxel row pieces of the component kernels and the
64-wide contour tile, J off the 8-row tile, a single plane, sizes that are no multiple of a 16-byte vector, two batch
elements, and one volume that spans several tiles along every axis."""
from __future__ import annotations

import os

import pytest
import torch

import label_cases
import torchio_amd as tio

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 24, 20, 37), (1, 1, 5, 7, 66), (1, 1, 1, 9, 130), (1, 1, 33, 33, 33)]
LARGE = (1, 1, 70, 65, 130)
FIELDS = [(shape, seed) for shape in SHAPES for seed in range(3)] + [(LARGE, 0)]
IDS = ["x".join(map(str, shape)) + f"-seed{seed}" for shape, seed in FIELDS]
DTYPES = [torch.uint8, torch.int16, torch.int64, torch.float32]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labels_golden.pt")


def field(shape, seed, dtype=torch.int16):
    return label_cases.label_field(tuple(shape), seed).to(dtype)


# -- remap family ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES + [LARGE], ids=lambda s: "x".join(map(str, s)))
def test_remap_swap_absent_key_and_constant_mode(hip, shape, dtype):
    data = field(shape, 0, dtype)
    mapping = {1: 2, 2: 1, 3: 9, 77: 5}  # a swap, a plain pair, a key the data does not hold
    assert torch.equal(hip.label_remap(data.cuda(), mapping).cpu(), label_cases.remap(data, mapping))
    assert torch.equal(hip.label_remap(data.cuda(), mapping, default=4).cpu(), label_cases.remap(data, mapping, default=4))
    assert torch.equal(hip.label_remap(data.cuda(), {}).cpu(), data)


@pytest.mark.parametrize("dtype", [torch.int8, torch.int32, torch.float64, torch.float16, torch.bfloat16], ids=str)
def test_remap_other_dtypes_and_negative_keys(hip, dtype):
    data = field(SHAPES[0], 1, dtype) - 1  # values -1 .. 2
    mapping = {-1: 3, 0: -2, 2: 0, 1000: 1, 0.5: 1}
    assert torch.equal(hip.label_remap(data.cuda(), mapping).cpu(), label_cases.remap(data, mapping))
    assert torch.equal(hip.label_remap(data.cuda(), mapping, default=-5).cpu(), label_cases.remap(data, mapping, default=-5))


@pytest.mark.parametrize("pairs", [300, 3000], ids=["lds", "global"])
def test_remap_many_pairs_on_int32(hip, pairs):
    """300 pairs are searched in LDS, 3000 (beyond the 2048 that fit) in global memory."""
    generator = torch.Generator().manual_seed(pairs)
    data = torch.randint(-50, 4000, (1, 1, 9, 11, 37), generator=generator, dtype=torch.int32)
    keys = torch.randperm(4000, generator=generator)[:pairs] - 20
    values = torch.randint(-(2**31), 2**31 - 1, (pairs,), generator=generator)
    mapping = dict(zip(keys.tolist(), values.tolist(), strict=True))
    lookup = torch.full((4100,), 2**40)
    lookup[keys + 50] = values
    hit = lookup[data.long() + 50]
    expected = torch.where(hit != 2**40, hit, data.long()).to(torch.int32)
    assert torch.equal(hip.label_remap(data.cuda(), mapping).cpu(), expected)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_remap_in_place_and_off_a_vector_boundary(hip, dtype):
    data = field(SHAPES[1], 2, dtype)
    mapping = {0: 3, 3: 0, 1: 1}
    expected = label_cases.remap(data, mapping)
    on_device = data.cuda()
    assert hip.label_remap(on_device, mapping, inplace=True) is on_device and torch.equal(on_device.cpu(), expected)
    flat = torch.cat([data.reshape(-1)[:3], data.reshape(-1)]).cuda()[3:]  # a dense view three elements off its allocation
    assert torch.equal(hip.label_remap(flat, mapping).cpu(), expected.reshape(-1))
    assert hip.label_remap(flat, mapping, inplace=True) is flat and torch.equal(flat.cpu(), expected.reshape(-1))


def test_remap_refuses_autograd_inputs(hip):
    with pytest.raises(tio.ops.EngineError, match="no backward"):
        hip.label_remap(torch.zeros(1, 1, 2, 2, 2, device="cuda", requires_grad=True), {0: 1})


def _subjects(seg, image=None):
    subjects = []
    for b in range(seg.shape[0]):
        entries = {"seg": tio.LabelMap(seg[b].clone())}
        if image is not None:
            entries["t1"] = tio.ScalarImage(image[b].clone())
        subjects.append(tio.Subject(**entries))
    return tio.SubjectsBatch.from_subjects(subjects).to("cuda")


def test_remap_remove_and_sequential_classes(hip):
    data = field(SHAPES[0], 2)
    sparse = torch.tensor([0, 5, 10, 40], dtype=torch.int16)[data.long()]
    image = torch.rand(2, 1, 24, 20, 37)
    out = tio.RemapLabels({1: 2, 2: 1})(_subjects(data, image))
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.remap(data, {1: 2, 2: 1})) and torch.equal(out.images["t1"].data.cpu(), image)
    assert torch.equal(tio.apply_inverse_transform(out).images["seg"].data.cpu(), data)
    out = tio.RemoveLabels([2, 3], background_label=6)(_subjects(data))
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.remap(data, {2: 6, 3: 6}))
    sparse[1] = torch.where(sparse[1] == 10, 7, sparse[1])  # element 1 holds a value element 0 does not: it becomes 0
    out = tio.SequentialLabels()(_subjects(sparse))
    assert out.applied_transforms[-1].params == {"remappings": {"seg": {0: 0, 5: 1, 10: 2, 40: 3}}}
    expected = label_cases.remap(sparse, {0: 0, 5: 1, 10: 2, 40: 3}, default=0)
    assert torch.equal(out.images["seg"].data.cpu(), expected) and bool((expected[1] != 2).all())
    restored = tio.apply_inverse_transform(out).images["seg"].data.cpu()
    assert torch.equal(restored, label_cases.remap(expected, {0: 0, 1: 5, 2: 10, 3: 40}, default=0)) and torch.equal(restored[0], sparse[0])
    with pytest.raises(ValueError, match="cannot be represented"):
        tio.RemapLabels({1: 70000})(_subjects(data))


# -- one-hot -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES + [LARGE], ids=lambda s: "x".join(map(str, s)))
def test_one_hot_inferred_and_given(hip, shape, dtype):
    data = field(shape, 1, dtype)
    inferred = hip.label_one_hot(data.cuda())
    assert inferred.dtype == torch.float32 and torch.equal(inferred.cpu(), label_cases.one_hot(data))
    assert torch.equal(hip.label_one_hot(data.cuda(), 7).cpu(), label_cases.one_hot(data, 7))
    off = torch.cat([data.reshape(-1)[:1], data.reshape(-1)]).cuda()[1:].view(data.shape)  # one element off its allocation
    assert torch.equal(hip.label_one_hot(off, 5).cpu(), label_cases.one_hot(data, 5))


def test_one_hot_raises_on_values_outside_the_classes(hip):
    data = field(SHAPES[1], 0)
    with pytest.raises(RuntimeError, match="class values"):
        hip.label_one_hot(data.cuda(), 3)
    negative = data.clone()
    negative[0, 0, 4, 6, 65] = -1
    with pytest.raises(RuntimeError, match="class values"):
        hip.label_one_hot(negative.cuda(), 4)
    fractional = data.float()
    fractional[0, 0, 0, 0, 0] = 1.5
    with pytest.raises(RuntimeError, match="class values"):
        hip.label_one_hot(fractional.cuda(), 4)
    with pytest.raises(RuntimeError, match="class values"):
        tio.OneHot(num_classes=2)(_subjects(data))


def test_one_hot_class_round_trip(hip):
    data = field(SHAPES[0], 0)
    out = tio.OneHot()(_subjects(data))
    assert out.images["seg"].data.shape == (2, 4, 24, 20, 37) and torch.equal(out.images["seg"].data.cpu(), label_cases.one_hot(data))
    assert torch.equal(tio.apply_inverse_transform(out).images["seg"].data.cpu(), data.float())


# -- contour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES + [LARGE], ids=lambda s: "x".join(map(str, s)))
def test_contour(hip, shape, dtype):
    data = field(shape, 2, dtype)
    out = hip.label_contour(data.cuda())
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), label_cases.contour(data))


def test_contour_face_rule_and_channels(hip):
    """All background: only the faces are marked (the padding, -1, is smaller); all -1: nothing is."""
    zeros = torch.zeros(1, 1, 9, 10, 70, dtype=torch.int16)
    expected = torch.ones(1, 1, 9, 10, 70)
    expected[:, :, 1:-1, 1:-1, 1:-1] = 0
    assert torch.equal(hip.label_contour(zeros.cuda()).cpu(), expected)
    assert torch.equal(hip.label_contour((zeros - 1).cuda()).cpu(), torch.zeros(1, 1, 9, 10, 70))
    assert torch.equal(hip.label_contour((zeros - 1).float().cuda()).cpu(), torch.zeros(1, 1, 9, 10, 70))
    one = zeros.clone()
    one[0, 0, 4, 5, 64] = 3  # an interior voxel: marked because its neighbours are smaller; they are not
    expected[0, 0, 4, 5, 64] = 1
    assert torch.equal(hip.label_contour(one.cuda()).cpu(), expected)
    two_channels = field((2, 1, 6, 9, 66), 0).reshape(1, 2, 6, 9, 66)  # (B, C): every volume on its own
    assert torch.equal(hip.label_contour(two_channels.cuda()).cpu(), label_cases.contour(two_channels))
    out = tio.Contour()(_subjects(field(SHAPES[1], 0)))
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.contour(field(SHAPES[1], 0)))


# -- keep the largest component ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fully_connected", [True, False], ids=["26", "6"])
@pytest.mark.parametrize(("shape", "seed"), FIELDS, ids=IDS)
def test_keep_largest_on_fields(hip, shape, seed, fully_connected):
    data = field(shape, seed)
    assert not label_cases.has_tie(data, [1, 2, 3], fully_connected)  # a condition on the input: no tie rule enters
    expected = label_cases.keep_largest(data, [1, 2, 3], 0, fully_connected)
    assert not torch.equal(expected, data)
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1, 2, 3], fully_connected=fully_connected).cpu(), expected)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int8, torch.int32, torch.int64, torch.float32], ids=str)
def test_keep_largest_dtypes_background_and_label_choice(hip, dtype):
    data = field(SHAPES[0], 1, dtype)
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1, 2, 3]).cpu(), label_cases.keep_largest(data, [1, 2, 3]))
    only_two = hip.keep_largest_component(data.cuda(), [2], background=5).cpu()  # fragments of 1 and 3 stay; removed voxels become 5
    assert torch.equal(only_two, label_cases.keep_largest(data, [2], 5)) and bool((only_two == 5).any())
    assert torch.equal(only_two[data != 2], data[data != 2])
    with_zero = hip.keep_largest_component(data.cuda(), [0, 1, 2, 3], background=3, fully_connected=False).cpu()
    assert torch.equal(with_zero, label_cases.keep_largest(data, [0, 1, 2, 3], 3, False))
    assert torch.equal(hip.keep_largest_component(data.cuda(), []).cpu(), data)
    assert torch.equal(hip.keep_largest_component(data.cuda(), [9]).cpu(), data)


def test_keep_largest_refuses_other_dtypes_and_channels(hip):
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(tio.ops.EngineError, match="status -2"):
            hip.keep_largest_component(torch.zeros(1, 1, 2, 2, 2, dtype=dtype, device="cuda"), [1])
    with pytest.raises(RuntimeError, match="single-channel"):
        hip.keep_largest_component(torch.zeros(1, 2, 2, 2, 2, dtype=torch.int16, device="cuda"), [1])
    seg = torch.zeros(1, 2, 4, 4, 4, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="single-channel"):
        tio.KeepLargestComponent()(_subjects(seg))


def test_corner_contact_joins_at_26_and_not_at_6(hip):
    data = torch.zeros(1, 1, 6, 6, 70, dtype=torch.int16)
    data[0, 0, 0:2, 0:2, 62:64] = 1  # 8 voxels ending at (1, 1, 63) ...
    data[0, 0, 2:4, 2:4, 64:67] = 1  # ... 12 voxels starting at (2, 2, 64): they touch at that corner only
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1], fully_connected=True).cpu(), data)
    expected = data.clone()
    expected[0, 0, 0:2, 0:2, 62:64] = 0
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1], fully_connected=False).cpu(), expected)


@pytest.mark.parametrize("fully_connected", [True, False], ids=["26", "6"])
def test_rows_planes_and_batch_elements_do_not_wrap(hip, fully_connected):
    data = torch.zeros(2, 1, 3, 4, 66, dtype=torch.int16)
    data[0, 0, 0, 0, 60:] = 1  # ends at k = K - 1 ...
    data[0, 0, 0, 2, :3] = 1   # ... a shorter run starts at k = 0 two rows on (adjacent in memory to nothing of the first)
    data[0, 0, 1, 0, 64:] = 2  # ends the row (1, 0); (1, 1) starts with ...
    data[0, 0, 1, 1, :1] = 2   # ... one voxel: adjacent in memory, two rows apart in k
    data[0, 0, 2, 3, 10:] = 3  # the last row of element 0 ...
    data[1, 0, 0, 0, :20] = 3  # ... and the first row of element 1: each is its element's only (hence largest) component
    data[1, 0, 2, 0, 5:8] = 3
    expected = data.clone()
    expected[0, 0, 0, 2, :3] = 0
    expected[0, 0, 1, 1, :1] = 0
    expected[1, 0, 2, 0, 5:8] = 0
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1, 2, 3], fully_connected=fully_connected).cpu(), expected)


def serpentine() -> tuple[torch.Tensor, torch.Tensor]:
    """A one-voxel-wide path of the value 1 through (17, 17, 66): along K in every second row of every second plane, the rows
    and planes joined at alternating ends — ONE component of 63 rows whose first voxels lie far apart — plus a separate
    10-voxel piece of the same value and a blob of the value 2.  Returns the volume and what must come out of it."""
    data = torch.zeros(1, 1, 17, 17, 66, dtype=torch.int16)
    at_end = True  # the path arrives at k = K - 1 first
    for i in range(0, 13, 2):  # (planes 13 .. 16 stay free for the separate piece)
        rows = list(range(0, 17, 2)) if i % 4 == 0 else list(range(16, -1, -2))
        for n, j in enumerate(rows):
            data[0, 0, i, j, :] = 1
            if n + 1 < len(rows):
                data[0, 0, i, (j + rows[n + 1]) // 2, 65 if at_end else 0] = 1
                at_end = not at_end
        if i + 2 < 13:
            data[0, 0, i + 1, rows[-1], 65 if at_end else 0] = 1
            at_end = not at_end
    data[0, 0, 5, 5:8, 20:30] = 2  # in a plane the path only crosses at its ends
    data[0, 0, 15, 3, 30:40] = 1
    expected = data.clone()
    expected[0, 0, 15, 3, 30:40] = 0
    return data, expected


@pytest.mark.parametrize("fully_connected", [True, False], ids=["26", "6"])
def test_serpentine_stays_whole(hip, fully_connected):
    data, expected = serpentine()
    assert int((expected == 1).sum()) == 63 * 66 + 62
    assert torch.equal(hip.keep_largest_component(data.cuda(), [1, 2], fully_connected=fully_connected).cpu(), expected)


def test_tie_keeps_the_component_that_comes_first_in_c_order(hip):
    data = torch.zeros(2, 1, 8, 9, 70, dtype=torch.int16)
    data[0, 0, 5, 2:4, 3:8] = 1     # 10 voxels, first voxel (5, 2, 3)
    data[0, 0, 1, 6:8, 60:65] = 1   # 10 voxels, first voxel (1, 6, 60): earlier in C order although later in j and k
    data[0, 0, 7, 0, 0:9] = 1       # 9 voxels
    data[1, 0, 0, 8, 65:70] = 2     # element 1: the first of two equal blobs wins there too
    data[1, 0, 3, 0, 0:5] = 2
    expected = torch.zeros_like(data)
    expected[0, 0, 1, 6:8, 60:65] = 1
    expected[1, 0, 0, 8, 65:70] = 2
    for fully_connected in (True, False):
        assert torch.equal(hip.keep_largest_component(data.cuda(), [1, 2], fully_connected=fully_connected).cpu(), expected)
    assert torch.equal(label_cases.keep_largest(data, [1, 2]), expected)
    tied = field((1, 1, 1, 9, 130), 0)  # whatever ties a random field holds: the same rule as the restatement's
    assert torch.equal(hip.keep_largest_component(tied.cuda(), [0, 1, 2, 3], background=9).cpu(), label_cases.keep_largest(tied, [0, 1, 2, 3], 9))


def test_keep_largest_class_defaults(hip):
    data = field(SHAPES[0], 0)
    out = tio.KeepLargestComponent()(_subjects(data))
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.keep_largest(data, [1, 2, 3]))
    out = tio.KeepLargestComponent(background_label=2, fully_connected=False)(_subjects(data))
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.keep_largest(data, [0, 1, 3], 2, False))
    with pytest.raises(ValueError, match="cannot be represented"):
        tio.KeepLargestComponent(background_label=-1)(_subjects(data.to(torch.uint8)))


# -- golden file and pipeline ------------------------------------------------------------------------------------------------
def test_golden_file_through_the_classes(hip):
    golden = torch.load(GOLDEN)
    fresh = lambda key="field": _subjects(golden[key])  # noqa: E731
    seg = lambda batch: batch.images["seg"].data.cpu()  # noqa: E731
    assert torch.equal(seg(tio.RemapLabels({1: 2, 2: 1, 3: 7, 9: 4})(fresh())), golden["remap"])
    assert torch.equal(seg(tio.RemoveLabels([2, 3], background_label=6)(fresh())), golden["remove"])
    out = tio.SequentialLabels()(fresh("sparse"))
    assert torch.equal(seg(out), golden["sequential"]) and out.applied_transforms[-1].params == golden["sequential_params"]
    assert torch.equal(seg(tio.OneHot()(fresh())), golden["one_hot"].float())
    assert torch.equal(seg(tio.OneHot(num_classes=6)(fresh())), golden["one_hot_6"].float())
    assert torch.equal(seg(tio.Contour()(fresh())), golden["contour"].float())
    for fully_connected in (True, False):
        out = tio.KeepLargestComponent(fully_connected=fully_connected)(fresh())
        assert torch.equal(seg(out), golden[f"keep_largest_{int(fully_connected)}"])
    assert torch.equal(seg(tio.KeepLargestComponent([2], background_label=5)(fresh())), golden["keep_largest_label2_background5"])


def test_compose_of_three_on_a_subjects_batch(hip):
    data = field(SHAPES[0], 1)
    image = torch.rand(2, 1, 24, 20, 37)
    batch = _subjects(data, image)
    pipeline = tio.Compose([tio.RemapLabels({1: 2, 2: 1}), tio.KeepLargestComponent(), tio.OneHot()])
    out = pipeline(batch)
    remapped = label_cases.remap(data, {1: 2, 2: 1})
    kept = label_cases.keep_largest(remapped, [1, 2, 3])
    assert torch.equal(out.images["seg"].data.cpu(), label_cases.one_hot(kept))
    assert torch.equal(out.images["t1"].data.cpu(), image) and torch.equal(batch.images["seg"].data.cpu(), data)
    assert [entry.name for entry in out.applied_transforms] == ["RemapLabels", "KeepLargestComponent", "OneHot"]
    restored = tio.apply_inverse_transform(out, warn=False)
    assert torch.equal(restored.images["seg"].data.cpu(), label_cases.remap(kept, {2: 1, 1: 2}).float())
    assert torch.equal(restored.images["t1"].data.cpu(), image)
