"""CPU: the oracle on volumes with NaN / +inf / -inf voxels against stock ATen, so that the GPU tests
(``test_gpu_nonfinite_resample.py``, ``test_gpu_nonfinite_movers.py``) compare the kernels with something independent.

* ``oracle.resample3d`` against ``aten_pipeline.resample`` (``F.grid_sample(padding_mode="zeros")`` on the data and on a volume
  of ones, then ``where``): the set of non-finite outputs and the set of NaN outputs are equal in every geometry of
  ``nonfinite_cases``; at the identity and the half-voxel shift, whose coordinates are exact in both float32 chains, the
  finite values are equal too.  Nearest images go through ``F.grid_sample(mode="nearest")`` on the same grid.
* every case is shown not to be vacuous: each planted site that the geometry keeps in view gives non-finite outputs (at every
  output voxel whose 2 x 2 x 2 footprint strictly contains it, read off ATen's own grid), all three classes are present, the
  identity has taps of weight zero (``MAY``), and the clean channel and the clean element stay finite.
* ``oracle.interpolate3d`` against ``F.interpolate``, ``oracle.pad3d`` against ``F.pad``, and ``oracle.bspline_prefilter``:
  the recursion runs along lines, so a (element, channel) line without a planted voxel is the clean run's bit for bit.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import aten_pipeline
import nonfinite_cases as nc

#: geometries ``aten_pipeline._grid`` restates (it adds the displacement to the affine image of the voxel: ``affine_first``)
ATEN_GEOMETRIES = tuple(g for g in nc.GEOMETRIES if g != "elastic_cp_first")
EXACT_COORDINATES = ("identity", "half")


def _aten_grids(case) -> torch.Tensor:
    """ATen's normalised grids ``(B, Io, Jo, Ko, 3)`` for a case: ``aten_pipeline._grid`` where the output grid is the input's,
    the same construction on the output's voxel grid for the down-sampling geometry (affine only)."""
    kw = case["kwargs"]
    in_shape, out_shape = tuple(case["volume"].shape[2:]), tuple(kw["out_shape"])
    control = kw["control_points"]
    if in_shape == out_shape:
        return torch.stack([aten_pipeline._grid(in_shape, kw["mapping"][n], None if control is None else control[n], "cpu")
                            for n in range(nc.BATCH)])
    assert control is None
    axes = [torch.arange(n, dtype=torch.float32) for n in out_shape]
    coords = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    homogeneous = torch.cat([coords, torch.ones_like(coords[..., :1])], dim=-1).reshape(-1, 4)
    sizes = torch.tensor([max(n - 1, 1) for n in in_shape], dtype=torch.float32)
    return torch.stack([2 * (homogeneous @ kw["mapping"][n].T).reshape(*out_shape, 3) / sizes - 1 for n in range(nc.BATCH)])


def _aten_resample(case, interp: str) -> torch.Tensor:
    kw = case["kwargs"]
    data, fill = case["volume"], kw["fills"][0]
    if interp == "linear" and tuple(data.shape[2:]) == tuple(kw["out_shape"]):
        return aten_pipeline.resample(data, kw["mapping"], kw["control_points"], fill)
    grids = _aten_grids(case).permute(0, 3, 2, 1, 4)
    volume = data.permute(0, 1, 4, 3, 2)
    out = F.grid_sample(volume, grids, mode="bilinear" if interp == "linear" else "nearest", padding_mode="zeros", align_corners=True)
    if fill is not None:  # (the in-bounds weight is trilinear for nearest data too)
        mask = F.grid_sample(torch.ones_like(volume), grids, mode="bilinear", padding_mode="zeros", align_corners=True)
        out = torch.where(mask > 0.5, out, fill.view(1, -1, 1, 1, 1))
    return out.permute(0, 1, 4, 3, 2)


def _voxels_that_see(case, site, interp: str) -> torch.Tensor:
    """Output voxels of element 0 (boolean mask) whose footprint strictly contains *site* and whose in-bounds weight is 1 to within 1e-3 per axis (kept under a fill rule), from
    ATen's grid: 1e-3 voxel inside the 2 x 2 x 2 cell (linear) or the rounding cell (nearest), so that no float32 rounding
    decides."""
    in_shape = case["volume"].shape[2:]
    grid = _aten_grids(case)[0]
    sees = torch.ones(grid.shape[:3], dtype=torch.bool)
    reach = (1.0 if interp == "linear" else 0.5) - 1e-3
    for axis in range(3):
        x = (grid[..., axis] + 1) / 2 * max(in_shape[axis] - 1, 1)
        sees &= ((x - site[axis]).abs() < reach) & (x > -1e-3) & (x < in_shape[axis] - 1 + 1e-3)
    return sees


@pytest.mark.parametrize("channel", [0, 1])
@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("name", nc.GEOMETRIES)
@pytest.mark.parametrize("shape", nc.SHAPES, ids=["ragged", "aligned"])
def test_oracle_resampling_of_non_finite_voxels_is_atens(oracle, shape, name, interp, with_fill, channel):
    case = nc.resample_case(name, shape, with_fill, channel, interp)
    got = oracle.resample3d([case["volume"]], **case["kwargs"])[0]
    nc.assert_case_is_not_vacuous(got, channel)
    if name not in ATEN_GEOMETRIES:
        return
    want = _aten_resample(case, interp)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want)), "the sets of non-finite outputs differ"
    assert torch.equal(got.isnan(), want.isnan()), "the sets of NaN outputs differ"
    if name in EXACT_COORDINATES:
        assert nc.same_bits_or_both_nan(got, want)
    # every planted site in view reaches the output
    seen = 0
    for site, _ in nc.planted_sites(shape, thick=name == "down3"):
        sees = _voxels_that_see(case, site, interp)
        seen += int(sees.any())
        assert not bool(torch.isfinite(got[0, channel][sees]).any()), f"site {site}: an output voxel that samples it is finite"
    if not (name == "half" and interp == "nearest"):  # (every coordinate a rounding tie: the cells' interiors are empty)
        assert seen >= (4 if interp == "linear" else 3), f"only {seen} planted sites in view"


@pytest.mark.parametrize("shape", nc.SHAPES, ids=["ragged", "aligned"])
@pytest.mark.parametrize("name", nc.GEOMETRIES)
def test_must_and_may_split_the_non_finite_set(oracle, shape, name):
    """MUST (non-zero weight) and MAY (weight exactly zero) partition the non-finite set; the identity mapping has both:
    the planted voxel itself, and the neighbours whose second tap it is."""
    n, must, may = nc.must_and_may(oracle, nc.resample_case(name, shape, False, 0))
    assert int(must.sum()) > 0 and bool(((must | may) == n).all()) and not bool((must & may).any())
    if name == "identity":
        assert int(may.sum()) > 0
        # weight 1 on the voxel itself, 0 on the seven others (or a few ulps: the coordinate goes through the normalised grid)
        assert int(must.sum()) >= len(nc.planted_sites(shape))
    if name == "half":
        assert int(may.sum()) == 0  # every weight is 1/8


def _poisoned_small(value: float) -> tuple[torch.Tensor, torch.Tensor]:
    clean = nc._data((2, 2, 13, 9, 20), torch.float32, 91)
    data = clean.clone()
    data[0, 1, 0, 0, 0] = value
    data[0, 1, 6, 4, 19] = value
    data[0, 1, 12, 8, 7] = -value
    return data, clean


@pytest.mark.parametrize("value", [nc.PINF, nc.NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_oracle_interpolate3d_is_f_interpolate(oracle, mode, value):
    data, _ = _poisoned_small(value)
    for out_shape in [(20, 9, 7), (5, 18, 33), (13, 9, 20), (25, 17, 39)]:
        got = oracle.interpolate3d(data, out_shape, mode)
        want = F.interpolate(data, size=out_shape, mode="trilinear", align_corners=True) if mode == "linear" else F.interpolate(data, size=out_shape, mode="nearest")
        assert not bool(torch.isfinite(got).all()), "the planted voxels are out of view"
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)) and torch.equal(got.isnan(), want.isnan())
        finite = torch.isfinite(want)
        torch.testing.assert_close(got[finite], want[finite], rtol=2e-6, atol=2e-7)  # (trilinear: within 1 ulp of the fma order)
        assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[0, 0]).all())


@pytest.mark.parametrize("value", [nc.PINF, nc.NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
def test_oracle_pad3d_is_f_pad(oracle, mode, value):
    data, _ = _poisoned_small(value)
    got = oracle.pad3d(data, (2, 5, 0, 3, 4, 1), mode, fill=-3.0)
    want = F.pad(data, (4, 1, 0, 3, 2, 5), mode=mode, **({"value": -3.0} if mode == "constant" else {}))
    assert torch.equal(nc.bits(got), nc.bits(want))
    assert int((~torch.isfinite(got)).sum()) >= 3


@pytest.mark.parametrize("value", [nc.PINF, nc.NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("order", [2, 3, 4, 5, 6, 7])
def test_oracle_bspline_prefilter_keeps_a_planted_voxel_on_its_lines(oracle, order, value):
    data, clean = _poisoned_small(value)
    got, want = oracle.bspline_prefilter(data, order), oracle.bspline_prefilter(clean, order)
    assert not bool(torch.isfinite(got[0, 1]).any()), "the recursion along three axes carries a non-finite voxel to the whole channel"
    for b, c in ((0, 0), (1, 0), (1, 1)):
        assert torch.equal(nc.bits(got[b, c]), nc.bits(want[b, c]))
    # one axis at a time: every (element, channel) is one line
    for axis in range(3):
        shape = [2, 2, 1, 1, 1]
        shape[2 + axis] = 23
        line_clean = nc._data(tuple(shape), torch.float32, 95)
        line = line_clean.clone()
        line.reshape(4, 23)[2, 11] = value
        got, want = oracle.bspline_prefilter(line, order), oracle.bspline_prefilter(line_clean, order)
        assert not bool(torch.isfinite(got.reshape(4, 23)[2]).any())
        keep = [0, 1, 3]
        assert torch.equal(nc.bits(got.reshape(4, 23)[keep]), nc.bits(want.reshape(4, 23)[keep]))
