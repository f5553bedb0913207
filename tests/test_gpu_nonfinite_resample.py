"""GPU: NaN / +inf / -inf voxels through every road of ``tio_resample3d``, against the CPU oracle (which
``test_nonfinite_host.py`` pins to stock ATen on such data).

A tap masked by a zero weight, a staged LDS cell that was never written, a 16-byte chunk that runs past a row's end and a
pass that holds only part of a box's planes all give the right answer on finite data (``0 * finite = 0``); a non-finite
voxel is the input that tells "times zero" from "not taken".  The volumes, the planted sites and the geometries are
``nonfinite_cases``'; every case asserts that its oracle output holds NaN, +inf and -inf and that the clean channel and
the clean batch element stay finite.

The forced roads and the switch that selects each:

==================  ===============================================================================  ==========
road                switches (all others cleared)                                                    plan bytes
==================  ===============================================================================  ==========
gather              TIO_RESAMPLE_PATH=gather                                                         0
brick               TIO_RESAMPLE_PATH=tile TIO_EXACT_PLAN=0 TIO_EXACT_LEAN=0                         0
                    (down3 / rot25: boxes beyond the tile, two / four passes or voxel by voxel)
planned_exact       TIO_RESAMPLE_PATH=tile TIO_EXACT_PLAN=2 TIO_EXACT_LEAN=0 (affine only)           > 0
lean_pair           TIO_EXACT_LEAN=2 (two channels: the pair kernel)                                 > 0
lean_single         TIO_EXACT_LEAN=2 TIO_LEAN_PAIR=0 (one launch per channel)                        > 0
lean_passes_listed  TIO_EXACT_LEAN=2, large_boxes=1 (TIO_GEOM_LARGE_BOXES: walkers, down3 / rot25)   > lean's
lean_passes_all     TIO_EXACT_LEAN=2, large_boxes=2 (TIO_GEOM_MOSTLY_LARGE_BOXES)                    > lean's
lean_no_passes      TIO_EXACT_LEAN=2 TIO_LEAN_MULTI=0, large_boxes=1 (voxel by voxel instead)        = lean's
tight_lean          precision="tight" TIO_FAST_KERNEL=planned (fused lerps on the lean kernel)       > 0
tight_lean_passes   the same with large_boxes=2 (down3 / rot25)                                      > lean's
tight_brick         precision="tight", nothing forced: a small launch stays on the brick kernel      0
nearest_exact       interp nearest, nothing forced (no fill rule: resample_nearest_exact_kernel)     -
nearest_kernel      interp nearest, TIO_NEAREST_EXACT=0 (resample_nearest_kernel; also what any      -
                    nearest image with a fill rule takes)
nearest_gather      interp nearest, TIO_NEAREST_KERNEL=0 (the gather kernel: the exact chain per     -
                    voxel, resample_exact_chain.hpp's sequence)
general dtypes      float16 / bfloat16 / float64: the brick kernel's any-dtype instantiation          -
==================  ===============================================================================  ==========

The lean roads need rows of 16 bytes and control cells at least a brick wide, so they run on the aligned shape with the
3 x 3 x 3 control grid; ``tio_resample3d_plan_bytes`` is asserted for every forced float road, so a switch that is
silently ignored cannot make a road's test vacuous.  ``precision="fast"`` is out of scope (its coordinates differ by
design).

Bars.  ``precision="exact"``: the oracle's bits, any NaN matching any NaN, over the whole output.  ``precision="tight"``:
a tolerance by contract, but the reference's coordinates, taps and fill decisions — every output in MUST (a planted voxel
under a non-zero weight) is non-finite, every output outside N (the oracle's non-finite set) is finite and inside
``test_gpu_tight.py``'s per-voxel bar, outputs in MAY = N \\ MUST (weight exactly zero) may be either.  Observed on the
MI355X for MAY: see ``test_tight_roads``.

Before every launch the same road runs once on a volume of NaN: a stale cell in LDS that meets a zero weight would show.
"""
from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

import nonfinite_cases as nc
from nonfinite_cases import ALIGNED, RAGGED

pytestmark = pytest.mark.gpu

#: every switch that takes part in the route choice (test_plan_bytes_routes.py): cleared for each case
SWITCHES = ("TIO_FAST_KERNEL", "TIO_EXACT_LEAN", "TIO_EXACT_PLAN", "TIO_PLANNED_LEAN", "TIO_LEAN_MULTI", "TIO_RESAMPLE_PATH",
            "TIO_RESAMPLE_EXACT", "TIO_TILE_ABLATE", "TIO_NEAREST_KERNEL", "TIO_NEAREST_EXACT", "TIO_LEAN_PAIR", "TIO_LEAN_LABEL",
            "TIO_LEAN_INTERLEAVE")

ALL = nc.GEOMETRIES
AFFINE_ONLY = ("identity", "half", "affine", "down3", "rot25")
LEAN = ("identity", "half", "affine", "elastic3", "down3", "rot25")
LARGE = ("down3", "rot25")

#: road -> (switches, precision, large_boxes, shapes, geometries, plan: "none" | "plain" | "multi")
ROADS = {
    "gather": ({"TIO_RESAMPLE_PATH": "gather"}, "exact", 0, (RAGGED, ALIGNED), ALL, "none"),
    "brick": ({"TIO_RESAMPLE_PATH": "tile", "TIO_EXACT_PLAN": "0", "TIO_EXACT_LEAN": "0"}, "exact", 0, (RAGGED, ALIGNED), ALL, "none"),
    "planned_exact": ({"TIO_RESAMPLE_PATH": "tile", "TIO_EXACT_PLAN": "2", "TIO_EXACT_LEAN": "0"}, "exact", 0, (RAGGED, ALIGNED), AFFINE_ONLY, "plain"),
    "lean_pair": ({"TIO_EXACT_LEAN": "2"}, "exact", 0, (ALIGNED,), LEAN, "plain"),
    "lean_single": ({"TIO_EXACT_LEAN": "2", "TIO_LEAN_PAIR": "0"}, "exact", 0, (ALIGNED,), LEAN, "plain"),
    "lean_passes_listed": ({"TIO_EXACT_LEAN": "2"}, "exact", 1, (ALIGNED,), LARGE, "multi"),
    "lean_passes_all": ({"TIO_EXACT_LEAN": "2"}, "exact", 2, (ALIGNED,), LARGE, "multi"),
    "lean_no_passes": ({"TIO_EXACT_LEAN": "2", "TIO_LEAN_MULTI": "0"}, "exact", 1, (ALIGNED,), LARGE, "plain"),
    "tight_lean": ({"TIO_FAST_KERNEL": "planned"}, "tight", 0, (ALIGNED,), LEAN, "plain"),
    "tight_lean_passes": ({"TIO_FAST_KERNEL": "planned"}, "tight", 2, (ALIGNED,), LARGE, "multi"),
    "tight_brick": ({}, "tight", 0, (RAGGED, ALIGNED), ("identity", "affine", "elastic"), "none"),
}
NEAREST_ROADS = {
    "nearest_exact": {},
    "nearest_kernel": {"TIO_NEAREST_EXACT": "0"},
    "nearest_gather": {"TIO_NEAREST_KERNEL": "0"},
}


def _shape_id(shape) -> str:
    return "ragged" if shape == RAGGED else "aligned"


def _road_cases(roads):
    return [pytest.param(road, shape, name, id=f"{road}-{_shape_id(shape)}-{name}")
            for road in roads for shape in ROADS[road][3] for name in ROADS[road][4]]


@pytest.fixture()
def switches(monkeypatch):
    """Clears every route switch, sets the case's own (conftest.py reparses the library's switches on each write)."""

    def use(env: dict) -> None:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        from torchio_amd import ops

        ops.reload_env()

    yield use
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    from torchio_amd import ops

    ops.reload_env()


def _to_device(kwargs: dict) -> dict:
    moved = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kwargs.items()}
    moved["fills"] = [None if f is None else f.cuda() for f in kwargs["fills"]]
    return moved


@functools.lru_cache(maxsize=None)
def _expected(oracle, name, shape, with_fill, channel, interp="linear"):
    """The oracle's output of one case, computed once and shared (never written to)."""
    case = nc.resample_case(name, shape, with_fill, channel, interp)
    out = oracle.resample3d([case["volume"]], **case["kwargs"])[0]
    nc.assert_case_is_not_vacuous(out, channel)
    return out


@functools.lru_cache(maxsize=None)
def _sets(oracle, name, shape, with_fill, channel):
    return nc.must_and_may(oracle, nc.resample_case(name, shape, with_fill, channel))


def _plan_bytes(hip, case, precision, large_boxes) -> int:
    kw = _to_device(case["kwargs"])
    geom, keep_alive = hip._resample_geom(
        nc.BATCH, tuple(case["volume"].shape[2:]), tuple(kw["out_shape"]), kw["mapping"], kw["control_points"], kw["in_spacing"],
        kw["out_spacing"], kw["affine_first"], None, None, None, precision, large_boxes)
    size = int(hip._fn["resample3d_plan_bytes"](C.byref(geom)))
    del keep_alive
    return size


def _assert_road(hip, case, precision, large_boxes, plan) -> None:
    got = _plan_bytes(hip, case, precision, large_boxes)
    if plan == "none":
        assert got == 0, f"the launch starts from a plan of {got} bytes: the switches did not keep it off the planned roads"
        return
    assert got > 0, "the launch does not start from a plan: the switches did not force the planned road"
    plain = _plan_bytes(hip, case, precision, 0)
    assert (got > plain) if plan == "multi" else (got == plain), (got, plain)


def _launch(hip, case, precision, large_boxes):
    """The case on the device, behind a throw-away launch of the same road on a volume of NaN."""
    kw = _to_device(case["kwargs"])
    hip.resample3d([torch.full_like(case["volume"], nc.NAN).cuda()], precision=precision, large_boxes=large_boxes, **kw)
    out = hip.resample3d([case["volume"].cuda()], precision=precision, large_boxes=large_boxes, **kw)[0]
    torch.cuda.synchronize()
    return out.cpu()


def _describe(want, got) -> str:
    differ = ~((nc.bits(want) == nc.bits(got)) | (want.isnan() & got.isnan()))
    where = differ.nonzero()[:6].tolist()
    return f"{int(differ.sum())} outputs differ, first at {where}: oracle {[float(want[tuple(w)]) for w in where]}, hip {[float(got[tuple(w)]) for w in where]}"


EXACT_ROADS = [road for road, spec in ROADS.items() if spec[1] == "exact"]
TIGHT_ROADS = [road for road, spec in ROADS.items() if spec[1] == "tight"]


@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("road,shape,name", _road_cases(EXACT_ROADS))
def test_exact_roads(oracle, hip, switches, road, shape, name, with_fill, channel):
    env, precision, large_boxes, _, _, plan = ROADS[road]
    switches(env)
    case = nc.resample_case(name, shape, with_fill, channel)
    want = _expected(oracle, name, shape, with_fill, channel)
    _assert_road(hip, case, precision, large_boxes, plan)
    got = _launch(hip, case, precision, large_boxes)
    assert nc.same_bits_or_both_nan(want, got), _describe(want, got)


def _per_voxel_beyond(want, got, finite) -> int:
    """test_gpu_tight.py's bar over the finite outputs: |d| <= 1e-4 max(|ref|, 1e-3 range), range of the finite reference."""
    want, got = want.double(), got.double()
    value_range = float(want[finite].max() - want[finite].min())
    rel = (want - got).abs() / want.abs().clamp_min(1e-3 * value_range)
    return int((rel[finite] > 1e-4).sum())


@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("road,shape,name", _road_cases(TIGHT_ROADS))
def test_tight_roads(oracle, hip, switches, road, shape, name, with_fill, channel):
    """MUST non-finite, everything outside N finite and inside the per-voxel bar, MAY either.

    Observed on the MI355X (printed per case): MAY is empty in every geometry but the identity (the other coordinates carry no
    weight of exactly zero); under the identity it holds 40 outputs on the aligned and 60 on the ragged shape, and all of them
    are NaN on the lean kernel (fused lerps), its pass variant and the brick kernel alike — what exact mode gives."""
    env, precision, large_boxes, _, _, plan = ROADS[road]
    switches(env)
    case = nc.resample_case(name, shape, with_fill, channel)
    want = _expected(oracle, name, shape, with_fill, channel)
    n, must, may = _sets(oracle, name, shape, with_fill, channel)
    _assert_road(hip, case, precision, large_boxes, plan)
    got = _launch(hip, case, precision, large_boxes)
    print(f"tight MAY: {road} {_shape_id(shape)} {name} fill={with_fill} channel={channel}: {int(may.sum())} outputs in MAY, "
          f"{int((~torch.isfinite(got))[may].sum())} of them non-finite, {int(got.isnan()[may].sum())} NaN")
    assert not bool(torch.isfinite(got)[must].any()), f"{int(torch.isfinite(got)[must].sum())} outputs under a non-zero weight are finite"
    assert bool(torch.isfinite(got)[~n].all()), f"{int((~torch.isfinite(got))[~n].sum())} non-finite outputs outside the oracle's set"
    assert _per_voxel_beyond(want, got, ~n) == 0
    if road == "tight_brick":  # (a small tight launch is the exact brick kernel)
        assert nc.same_bits_or_both_nan(want, got), _describe(want, got)


@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("shape", nc.SHAPES, ids=_shape_id)
@pytest.mark.parametrize("road", list(NEAREST_ROADS))
def test_nearest_roads(oracle, hip, switches, road, shape, name, with_fill):
    switches(NEAREST_ROADS[road])
    case = nc.resample_case(name, shape, with_fill, 0, "nearest")
    want = _expected(oracle, name, shape, with_fill, 0, "nearest")
    got = _launch(hip, case, "exact", 0)
    assert nc.same_bits_or_both_nan(want, got), _describe(want, got)


OVERFLOW = {torch.float16: 1.0e6, torch.bfloat16: 3.4e38, torch.float64: 1.0e6}  # finite in float32, infinite once stored (not float64)


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64], ids=["float16", "bfloat16", "float64"])
def test_storage_dtypes(oracle, hip, switches, dtype, interp):
    """The general-dtype road on the ragged shape; the fill value of channel 0 is finite in float32 and overflows when it is
    stored to a half type."""
    switches({})
    volume, _ = nc.poisoned(RAGGED, dtype)
    kwargs = dict(nc.geometry("affine", RAGGED), interps=[interp], fills=[torch.tensor([OVERFLOW[dtype], 0.5])])
    want = oracle.resample3d([volume], **kwargs)[0]
    found = nc.classes(want[0, 0])
    assert all(found.values()) and bool(torch.isfinite(want[1, 1]).all()) and bool(torch.isfinite(want[0, 1]).all()), found
    if dtype != torch.float64:
        assert bool((want[1, 0] == nc.PINF).any()), "the fill value did not overflow on the store"
    kw = _to_device(kwargs)
    hip.resample3d([torch.full_like(volume, nc.NAN).cuda()], **kw)
    got = hip.resample3d([volume.cuda()], **kw)[0].cpu()
    assert got.dtype == dtype and nc.same_bits_or_both_nan(want, got), _describe(want, got)


@pytest.mark.parametrize("env", [{}, {"TIO_EXACT_LEAN": "2"}, {"TIO_RESAMPLE_PATH": "gather"}], ids=["default", "lean", "gather"])
def test_label_maps_beside_a_poisoned_image(oracle, hip, switches, env):
    """One call: a poisoned float32 image (linear), a clean int16 map in "label" mode and a clean uint8 nearest map — the
    label outputs are the oracle's and those of the call with a clean image."""
    switches(env)
    volume, clean = nc.poisoned(ALIGNED)
    t1, t1_clean = volume[:, :1].contiguous(), clean[:, :1].contiguous()
    seg = nc._data((nc.BATCH, 1, *ALIGNED), torch.int16, 53)
    mask = nc._data((nc.BATCH, 1, *ALIGNED), torch.uint8, 54)
    kwargs = dict(nc.geometry("elastic3", ALIGNED), interps=["linear", "label", "nearest"], fills=[torch.tensor([-1.0]), None, None],
                  label_tables=[None, torch.unique(seg).double(), None], pad_labels=[0.0, 0.0, 0.0])
    want = oracle.resample3d([t1, seg, mask], **kwargs)
    assert all(nc.classes(want[0][0]).values()) and bool(torch.isfinite(want[0][1]).all())
    kw = _to_device(kwargs)
    kw["label_tables"] = [None, kwargs["label_tables"][1].cuda(), None]
    got = hip.resample3d([t1.cuda(), seg.cuda(), mask.cuda()], **kw)
    got_clean = hip.resample3d([t1_clean.cuda(), seg.cuda(), mask.cuda()], **kw)
    torch.cuda.synchronize()
    assert nc.same_bits_or_both_nan(want[0], got[0].cpu()), _describe(want[0], got[0].cpu())
    for index in (1, 2):
        assert torch.equal(want[index], got[index].cpu()) and torch.equal(got[index], got_clean[index])


@pytest.mark.parametrize("name", ["affine", "elastic", "elastic_cp_first"])
@pytest.mark.parametrize("interp,order", [("cubic", 3), ("seventh", 7)])
def test_spline_images_with_a_planted_coefficient(oracle, hip, switches, interp, order, name):
    """A NaN, a +inf and a -inf coefficient: the non-finite set is the oracle's, the finite values are its bits."""
    switches({})
    shape = (30, 26, 34)
    coefficients = nc._data((nc.BATCH, nc.CHANNELS, *shape), torch.float32, 8)
    for site, value in (((0, 0, 0), nc.NAN), ((15, 15, 15), nc.PINF), ((16, 16, 33), nc.NINF), ((29, 25, 33), nc.PINF), ((8, 20, 16), nc.NINF)):
        coefficients[(0, 0, *site)] = value
    kwargs = dict(nc.geometry(name, shape), interps=[interp], fills=[None])
    want = oracle.resample3d([coefficients], **kwargs)[0]
    nc.assert_case_is_not_vacuous(want, 0)
    got = hip.resample3d([coefficients.cuda()], **_to_device(kwargs))[0].cpu()
    assert torch.equal(torch.isfinite(want), torch.isfinite(got)) and torch.equal(want.isnan(), got.isnan())
    finite = torch.isfinite(want)
    assert torch.equal(nc.bits(want)[finite], nc.bits(got)[finite])
    assert int(finite[0, 0].sum()) > 0


PASSTHROUGH_ROADS = {
    "gather": ({"TIO_RESAMPLE_PATH": "gather"}, "exact", "linear"),
    "brick": ({"TIO_RESAMPLE_PATH": "tile", "TIO_EXACT_PLAN": "0", "TIO_EXACT_LEAN": "0"}, "exact", "linear"),
    "planned_exact": ({"TIO_RESAMPLE_PATH": "tile", "TIO_EXACT_PLAN": "2", "TIO_EXACT_LEAN": "0"}, "exact", "linear"),
    "lean_pair": ({"TIO_EXACT_LEAN": "2"}, "exact", "linear"),
    "lean_single": ({"TIO_EXACT_LEAN": "2", "TIO_LEAN_PAIR": "0"}, "exact", "linear"),
    "tight_lean": ({"TIO_FAST_KERNEL": "planned"}, "tight", "linear"),
    "nearest_exact": ({}, "exact", "nearest"),
    "nearest_kernel": ({"TIO_NEAREST_EXACT": "0"}, "exact", "nearest"),
    "nearest_gather": ({"TIO_NEAREST_KERNEL": "0"}, "exact", "nearest"),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("road", list(PASSTHROUGH_ROADS))
def test_passthrough_rows_keep_their_bits(hip, switches, road, dtype):
    """A gated element is a copy: NaN payloads (0x7FC00001, 0x7F800001, 0xFFC00000), -0.0, the infinities and subnormals
    come out as they went in, on every road (float16 rows take the general-dtype instantiations of the same switches)."""
    env, precision, interp = PASSTHROUGH_ROADS[road]
    switches(env)
    data = nc.payload_volume((3, nc.CHANNELS, *ALIGNED), dtype, 61)
    kwargs = dict(nc.geometry("affine", ALIGNED), interps=[interp], fills=[torch.tensor(nc.FILL)])
    kwargs["mapping"] = torch.cat([kwargs["mapping"], kwargs["mapping"][:1]])
    kw = _to_device(kwargs)
    out = hip.resample3d([data.cuda()], precision=precision, passthrough=torch.tensor([0, 1, 0], dtype=torch.uint8).cuda(), **kw)[0].cpu()
    assert torch.equal(nc.bits(out[1]), nc.bits(data[1]))
    assert not torch.equal(nc.bits(out[0]), nc.bits(data[0]))  # (the other rows were resampled)
