"""GPU: one brick plan made AHEAD (`Engine.resample_plan`, `tio_resample3d_plan`) and handed to more than one call — the calls of
a `Compose` child (`Spatial._prefetch` makes one plan; the one-hot call of a label map in the "label" mode and the fused call
both take it), the chunks of `MAX_IMAGES` images of one call — and to calls it was not made for.

3 x 256^3 float32 (12 288 bricks: the smallest launch that plans by itself) rotated about every axis by 5 / 30 / 5 degrees: the
30-degree element's bricks have input boxes beyond the staging tile, which the exact-coordinate lean road lists (hint level 1,
`TIO_GEOM_LARGE_BOXES`: walked by `resample_lean_exact_multi_kernel` behind the main kernel) or stages in every block (level 2).
The list's length lives in the plan's header; a plan made ahead must list its bricks for every call it is handed to.

Unwritten voxels are made visible: the blocks the caching allocator hands out next are filled with NaN before every call, and
every output stays alive until its asserts are done (a freed correct result must not come back as a new output).
"""
from __future__ import annotations

import copy
import warnings

import pytest
import torch

import torchio_amd as tio
from parity_harness import nested_spheres
from test_gpu_large_boxes import _per_voxel
from test_gpu_large_boxes import _rotation_mappings
from torchio_amd import ops
from torchio_amd.transforms import spatial as sp

pytestmark = pytest.mark.gpu

SIZE, BATCH = 256, 3
SHAPE = (SIZE,) * 3
BRICKS = BATCH * (SIZE // 16) ** 3
ORDERS = {"large_second": [5, 30, 5], "large_first": [30, 5, 5]}  # degrees about every axis, per element
LEVELS = (0, 1, 2)
PRECISIONS = ("fast", "tight", "exact")
# channel 0's fill lies above the data (its minimum is a sampled value, not the fill), channel 1's below
FILL = torch.tensor([1.5, -0.25])


def _geometry(order: str, elastic: bool, device) -> dict:
    field = None
    if elastic:  # 7^3 control points, unit spacing: the exact elastic launch stays on the lean road
        field = ((torch.rand(BATCH, 7, 7, 7, 3, generator=torch.Generator().manual_seed(4)) - 0.5) * 15.0).to(device)
    return dict(
        out_shape=SHAPE, mapping=_rotation_mappings(ORDERS[order], SIZE).to(device), control_points=field,
        in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True,
    )


def _poison(shape, count: int = 1) -> None:
    """NaN in the blocks the caching allocator hands out next: a voxel the launch leaves unwritten stays NaN."""
    blocks = [torch.full(shape, float("nan"), device="cuda") for _ in range(count)]
    del blocks


def _resample(hip, images, geometry, *, precision, level, plan=None, channels=2):
    _poison((BATCH, channels, *SHAPE), len(images))
    fills = [FILL[:channels].cuda() for _ in images]
    return hip.resample3d(images, interps=["linear"] * len(images), fills=fills, precision=precision, large_boxes=level, plan=plan, **geometry)


def _plan_ahead(hip, geometry, *, precision, level):
    """The plan made on a side stream (as `Spatial._prefetch` makes it), the current stream ordered behind it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())  # (the geometry was uploaded on the current stream)
    with torch.cuda.stream(side):
        plan = hip.resample_plan(batch=BATCH, in_shape=SHAPE, precision=precision, large_boxes=level, **geometry)
        ready = side.record_event()
    torch.cuda.current_stream().wait_event(ready)
    if plan is not None:
        plan.record_stream(torch.cuda.current_stream())
    return plan


def _listed(plan) -> int:
    """Word 0 of the plan's header: the number of multi-pass bricks listed for the walkers (resample_plan.hpp: the plan)."""
    torch.cuda.synchronize()
    return int(plan[0])


def _check_listed(plan, level: int) -> int:
    listed = _listed(plan)
    if level == 1:
        assert 0 < listed < BRICKS, listed  # some bricks, not all: the walkers have work and the main kernel too
    elif level == 2:
        assert listed == 0  # (every block runs the pass logic: nothing is listed)
    return listed


class _Spy:
    """The engine's calls by name (`Engine._call`) and the plan each `tio_resample3d` was handed (geom.plan_dev)."""

    def __init__(self, hip):
        self.hip, self.names, self.plans = hip, [], []

    def __enter__(self):
        original_call, original_fn = self.hip._call, self.hip._fn["resample3d"]
        self._original_fn = original_fn

        def resample3d(geom, *args):
            self.plans.append(geom._obj.plan_dev)
            return original_fn(geom, *args)

        self.hip._call = lambda name, *args: (self.names.append(name), original_call(name, *args))[1]
        self.hip._fn["resample3d"] = resample3d
        return self

    def __exit__(self, *exc):
        del self.hip._call
        self.hip._fn["resample3d"] = self._original_fn


def _assert_oracle(out, want, precision: str, what) -> None:
    if precision == "exact":
        assert torch.equal(out, want), what
    else:  # (tight: fused lerps — the per-voxel bar of tests/test_gpu_large_boxes.py)
        assert _per_voxel(out, want) <= 1e-4, what


@pytest.fixture(scope="module")
def volume():
    """(3, 2, 256^3) float32 on the host and on the device: two channels — an exact launch without multi-pass bricks pairs them
    (resample_lean_exact_pair_kernel), one with them launches the main kernel and the walkers once per channel."""
    host = torch.rand(BATCH, 2, *SHAPE, generator=torch.Generator().manual_seed(5))
    yield host, host.cuda()


@pytest.fixture(scope="module")
def expected(oracle, volume):
    """The CPU oracle's result for a geometry (on the device, computed once per module)."""
    cache = {}

    def get(order: str, elastic: bool):
        if (order, elastic) not in cache:
            cache[order, elastic] = oracle.resample3d(
                [volume[0]], interps=["linear"], fills=[FILL], **_geometry(order, elastic, "cpu")
            )[0].cuda()
        return cache[order, elastic]

    yield get
    cache.clear()


def test_the_geometry_lists_some_bricks():
    for order in ORDERS:
        mappings = _rotation_mappings(ORDERS[order], SIZE).numpy()
        assert sp._expects_large_boxes(mappings, None, None, SHAPE, (1.0, 1.0, 1.0)) == 1
        assert sp._expects_large_boxes(mappings, [(7.5,) * 3] * BATCH, (7, 7, 7), SHAPE, (1.0, 1.0, 1.0)) == 1


@pytest.mark.parametrize("elastic", [False, True], ids=["affine", "elastic"])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("precision", ["exact", "tight"])
@pytest.mark.parametrize("level", LEVELS)
def test_reuse_of_one_plan_by_three_calls(hip, volume, expected, level, precision, order, elastic):
    """One plan made ahead, handed to three consecutive calls: each is the oracle's result (exact: bit for bit) and the call's own
    plan's (bit for bit), none plans again, and the header still lists the plan's bricks afterwards (cursor and done count at zero)."""
    torch.cuda.empty_cache()
    geometry = _geometry(order, elastic, "cuda")
    plan = _plan_ahead(hip, geometry, precision=precision, level=level)
    assert plan is not None
    listed = _check_listed(plan, level)
    with _Spy(hip) as spy:
        outs = [_resample(hip, [volume[1]], geometry, precision=precision, level=level, plan=plan)[0] for _ in range(3)]
    plain = _resample(hip, [volume[1]], geometry, precision=precision, level=level)[0]
    torch.cuda.synchronize()
    assert spy.names == ["resample3d"] * 3  # no resample3d_plan: the calls start from the plan made ahead
    assert spy.plans == [plan.data_ptr()] * 3
    want = expected(order, elastic)
    assert not plain.isnan().any()
    for n, out in enumerate(outs):
        assert not out.isnan().any(), f"call {n}: bricks not written"
        assert torch.equal(out, plain), f"call {n}: not the call's own plan's result"
        _assert_oracle(out, want, precision, f"call {n}")
    if level > 0:  # the walkers of the last call left the list as the planner wrote it, cursor and done count at zero
        assert _listed(plan) == listed and int(plan[1]) == 0 and int(plan[2]) == 0


@pytest.mark.parametrize("precision", ["exact", "tight"])
def test_chunks_of_one_call_share_the_plan(hip, oracle, precision):
    """Nine single-channel images in one `resample3d` call: two chunks of `MAX_IMAGES`, two `tio_resample3d` calls that start from
    the same level-1 plan.  Every image is the oracle's."""
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(8)
    hosts = [torch.rand(BATCH, 1, *SHAPE, generator=g) for _ in range(9)]
    wants = oracle.resample3d(hosts, interps=["linear"] * 9, fills=[FILL[:1]] * 9, **_geometry("large_second", False, "cpu"))
    images = [h.cuda() for h in hosts]
    geometry = _geometry("large_second", False, "cuda")
    plan = _plan_ahead(hip, geometry, precision=precision, level=1)
    _check_listed(plan, 1)
    with _Spy(hip) as spy:
        outs = _resample(hip, images, geometry, precision=precision, level=1, plan=plan, channels=1)
    torch.cuda.synchronize()
    assert spy.names == ["resample3d"] * 2 and spy.plans == [plan.data_ptr()] * 2
    for n, (out, want) in enumerate(zip(outs, wants, strict=True)):
        assert not out.isnan().any(), f"image {n}: bricks not written"
        _assert_oracle(out, want.cuda(), precision, f"image {n}")


@pytest.fixture(scope="module")
def without_plan(hip, volume):
    """Results of calls made without a plan, per (elastic, level, precision): the yardstick of every plan handed to them."""
    cache = {}
    single = volume[1][:, :1].contiguous()

    def get(elastic: bool, level: int, precision: str):
        if (elastic, level, precision) not in cache:
            geometry = _geometry("large_second", elastic, "cuda")
            cache[elastic, level, precision] = _resample(hip, [single], geometry, precision=precision, level=level, channels=1)[0]
        return single, cache[elastic, level, precision]

    yield get
    cache.clear()


@pytest.mark.parametrize("elastic", [False, True], ids=["affine", "elastic"])
@pytest.mark.parametrize("made_for", [(level, precision) for level in LEVELS for precision in PRECISIONS], ids=lambda m: f"{m[1]}{m[0]}")
def test_a_plan_serves_only_the_calls_it_was_made_for(hip, without_plan, made_for, elastic):
    """A plan made at one (hint level, precision) handed to calls at every (hint level, precision): the call it was made for takes
    it, every other call ignores it (its own plan: kDescMulti bricks are not dropped, a FAST kernel never reads a multi-pass
    descriptor) — and each result is that call's without a plan, bit for bit."""
    level, precision = made_for
    geometry = _geometry("large_second", elastic, "cuda")
    plan = _plan_ahead(hip, geometry, precision=precision, level=level)
    if precision == "fast" and level > 0:  # (a FAST launch with the hint takes the brick kernel's in-kernel boxes: no plan)
        assert plan is None
        return
    assert plan is not None
    _check_listed(plan, level)
    for call_level in LEVELS:
        for call_precision in PRECISIONS:
            data, plain = without_plan(elastic, call_level, call_precision)
            with _Spy(hip) as spy:
                out = _resample(hip, [data], geometry, precision=call_precision, level=call_level, plan=plan, channels=1)[0]
            torch.cuda.synchronize()
            matched = (call_level, call_precision) == made_for
            assert spy.plans == [plan.data_ptr() if matched else None], (call_level, call_precision)
            assert not out.isnan().any(), (call_level, call_precision)
            assert torch.equal(out, plain), (call_level, call_precision)
            del out


@pytest.mark.parametrize("elastic", [False, True], ids=["affine", "elastic"])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("precision", ["exact", "tight"])
@pytest.mark.parametrize("level", [1, 2])
def test_folded_minimum_of_multi_pass_bricks(hip, volume, expected, monkeypatch, level, precision, order, elastic):
    """The FOLD_MIN instantiations of the walkers (level 1) and of the one-launch form (level 2): element 0's minimum folded by bricks
    staged in passes ("large_first": element 0 is the rotated one) or not ("large_second") is `amin` of what was stored — without a
    plan and with one made ahead, twice — and the values are the oracle's."""
    monkeypatch.setenv("TIO_FOLDED_MIN", "1")
    torch.cuda.empty_cache()
    geometry = _geometry(order, elastic, "cuda")
    plan = _plan_ahead(hip, geometry, precision=precision, level=level)
    _check_listed(plan, level)
    outs = [_resample(hip, [volume[1]], geometry, precision=precision, level=level, plan=p)[0] for p in (None, plan, plan)]
    torch.cuda.synchronize()
    want = expected(order, elastic)
    for n, out in enumerate(outs):
        assert not out.isnan().any(), f"call {n}: bricks not written"
        folded = ops.folded_channel_min(out)
        assert folded is not None, n
        assert torch.equal(folded, out[0].amin(dim=(1, 2, 3))), (n, folded, out[0].amin(dim=(1, 2, 3)))
        _assert_oracle(out, want, precision, f"call {n}")


@pytest.fixture
def _restore():
    previous = tio.get_resample_precision()
    yield
    tio.set_resample_precision(previous)
    ops.set_ahead_stream(True)


def _subjects(kind: str):
    g = torch.Generator().manual_seed(13)
    if kind == "t1_and_label":
        return [tio.Subject(t1=tio.ScalarImage(torch.rand(1, *SHAPE, generator=g)), seg=tio.LabelMap(nested_spheres(SIZE))) for _ in range(BATCH)]
    return [tio.Subject(**{f"image{n}": tio.ScalarImage(torch.rand(1, *SHAPE, generator=g)) for n in range(9)}) for _ in range(BATCH)]


@pytest.mark.parametrize("precision", ["exact", "tight"])
@pytest.mark.parametrize("kind", ["t1_and_label", "nine_images"])
def test_public_compose_hands_its_plan_to_every_call(hip, monkeypatch, _restore, kind, precision):
    """The public API: `Compose[Affine, Blur]` draws ahead, so the Affine's plan is made on the side stream and handed to every
    gated call of the child — the one-hot call of a label map in the antialiased "label" mode and the fused call, or the two
    chunks of nine images.  With the hint at level 1 (the walkers' list) the outputs are those of the same pipeline without the
    side stream (every call plans for itself), bit for bit, and hold no NaN."""
    monkeypatch.setattr(sp, "_expects_large_boxes", lambda *args: 1)
    tio.set_resample_precision(precision)
    source = tio.SubjectsBatch.from_subjects(_subjects(kind)).to("cuda")
    names = list(source.images)
    results = {}
    for ahead in (True, False):
        ops.set_ahead_stream(ahead)
        pipeline = tio.Compose([
            tio.Affine(degrees=(25, 25), scales=(1.0, 1.0), translation=(3, 3), label_interpolation="label", antialias=True),
            tio.Blur(std=(0.5, 1.0)),
        ])
        assert pipeline._may_draw_ahead()
        torch.cuda.empty_cache()
        _poison((BATCH, 1, *SHAPE), 2 * len(names))
        _poison((BATCH, 5, *SHAPE))  # (the one-hot channels of the label map's five labels)
        torch.manual_seed(41)
        with _Spy(hip) as spy, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = pipeline(source)
        torch.cuda.synchronize()
        results[ahead] = (out, spy, [(t.name, copy.deepcopy(dict(t.params))) for t in out.applied_transforms])
    (out_a, spy_a, history_a), (out_b, spy_b, history_b) = results[True], results[False]
    assert history_a == history_b
    assert "resample3d_plan" in spy_a.names and "resample3d_plan" not in spy_b.names
    handed = [p for p in spy_a.plans if p is not None]
    assert len(handed) >= 2 and len(set(handed)) == 1, spy_a.plans  # ONE plan, more than one call
    assert all(p is None for p in spy_b.plans)
    for name in names:
        a, b = out_a.images[name].data, out_b.images[name].data
        if a.dtype.is_floating_point:
            assert not a.isnan().any(), f"{name}: bricks not written"
        assert torch.equal(a, b), name


def test_the_headline_launches_still_take_their_plans(hip, _restore):
    """The FAST mode (the benchmark's launches: no hint at these ranges): a `Compose` that draws ahead hands every resampling call the
    plan its child made ahead — the signature check drops none of them (each call would plan again on the data stream)."""
    tio.set_resample_precision("fast", allow_out_of_tolerance=True)
    g = torch.Generator().manual_seed(19)
    subjects = [tio.Subject(t1=tio.ScalarImage(torch.rand(1, *SHAPE, generator=g)), seg=tio.LabelMap(nested_spheres(SIZE))) for _ in range(BATCH)]
    source = tio.SubjectsBatch.from_subjects(subjects).to("cuda")
    pipeline = tio.Compose([tio.Affine(degrees=(-5, 5), translation=(-5, 5)), tio.ElasticDeformation(), tio.Blur(std=(0.5, 1.0))])
    assert pipeline._may_draw_ahead()
    torch.manual_seed(43)
    with _Spy(hip) as spy, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pipeline(source)
    torch.cuda.synchronize()
    assert spy.names.count("resample3d_plan") == 2 and spy.names.count("resample3d") == 2, spy.names
    assert all(p is not None for p in spy.plans) and len(set(spy.plans)) == 2, spy.plans
    assert not out.t1.data.isnan().any()
