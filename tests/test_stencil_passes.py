"""What the separable stencil's dispatcher launches, asked on the CPU through ``tio_separable_conv3d_passes``.

The entry point runs the launcher's own decision function and enqueues nothing, so these tests need no GPU.  They pin

* the label of every case of the geometry sweep (``tests/stencil_geometry_cases.py``): kernel family, segments x rows, K tiles,
  radius class and stages per pass — what ``tests/test_gpu_stencil_geometry.py`` then runs on the device;
* that every workload geometry (256^3 batches of 1 .. 64, 512^3, 240 x 240 x 155) has a thin case with the same launch, so the
  sweep is not vacuous and a moved threshold fails here until the sweep moves with it;
* the refusal of a pass with more than 65 535 lines, before any launch;
* the CPU oracle itself against a float64 correlation, within the derived rounding bound, for every sweep case — the anchor of
  the bit-for-bit comparisons on the GPU.
"""
from __future__ import annotations

import os

import pytest
import torch

from torchio_amd import _lib

from stencil_geometry_cases import SWEEP, SWITCHES, WORKLOADS, Pass, bound_factor, expected_bias_passes, make_inputs, reference64
from stencil_geometry_cases import reported_passes, within_bound


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _report(fn, case, monkeypatch, **kw):
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    fn["reload_env"]()  # (tests/conftest.py reloads on writes as well; explicit here: the report below depends on it)
    try:
        return reported_passes(fn, case.shape, case.radius, dtype=case.dtype, has_skip=case.skip_row is not None, **kw)
    finally:
        for name in case.env:
            monkeypatch.delenv(name, raising=False)
        fn["reload_env"]()


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep_case_launches_what_it_is_labelled_with(fn, monkeypatch, name):
    case = SWEEP[name]
    passes, stages = _report(fn, case, monkeypatch)
    assert [p.key() for p in passes] == [p.key() for p in case.passes], name
    assert [s["last"] for s in stages] == [0] * (len(passes) - 1) + [1]
    assert all(s["pre_bias"] == 0 and s["post_noise"] == 0 and s["fma"] == 0 for s in stages)
    assert [s["radius"] for s in stages] == [case.radius[p.axis] for p in passes]
    # the segments tile the line: the last one is not empty and nothing is left over
    for p in passes:
        if p.axis < 2:
            n = case.shape[2 + p.axis]
            assert (p.segments - 1) * p.rows < n <= p.segments * p.rows
    # the stages of tio_blur_fused: bias on the I pass's loads, noise on the stores of the pass with the K stage, fused
    # multiply-adds in the marching passes only
    if not case.fused_form:
        for kw in ({"bias": True}, {"noise": 1}, {"noise": 2}):
            assert _report(fn, case, monkeypatch, **kw) == -5, (name, kw)  # TIO_ERR_UNSUPPORTED_CONFIG
        return
    for noise in (0, 1, 2):
        got, st = reported_passes(fn, case.shape, case.radius, bias=True, noise=noise, fast=False)
        assert [p.key() for p in got] == [p.key() for p in expected_bias_passes(case)], (name, noise)
        assert [s["pre_bias"] for s in st] == [1, 0] and [s["post_noise"] for s in st] == [0, noise]
    got, st = reported_passes(fn, case.shape, case.radius, fast=True)
    assert [p.key() for p in got] == [p.key() for p in case.passes]
    assert [s["fma"] for s in st] == [int(p.family == "march") for p in got]
    assert reported_passes(fn, case.shape, case.radius, bias=True, has_skip=True) == -5  # no fused form with skipped rows


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_every_workload_geometry_has_a_thin_case_with_the_same_launch(fn, name):
    shape, radius, axis, thin_name, rows_too = WORKLOADS[name]
    thin = SWEEP[thin_name]
    assert thin.seam_axis == axis and not thin.env
    (passes, stages), (thin_passes, thin_stages) = reported_passes(fn, shape, radius), reported_passes(fn, thin.shape, thin.radius)
    index = [p.axis for p in passes].index(axis)
    thin_index = [p.axis for p in thin_passes].index(axis)
    big, small = passes[index], thin_passes[thin_index]
    assert (big.family, big.segments, big.radius_class, big.radius_k > 0, big.k_tiles > 1) == (
        small.family, small.segments, small.radius_class, small.radius_k > 0, small.k_tiles > 1), (big, small)
    flags = ("pre_bias", "post_noise", "fma", "last")
    assert [stages[index][f] for f in flags] == [thin_stages[thin_index][f] for f in flags]
    if rows_too:
        assert big.rows == small.rows, (big, small)
    # with the stages of tio_blur_fused riding along (where the workload has the fused form at all)
    fused, thin_fused = reported_passes(fn, shape, radius, bias=True, noise=2, fast=True), reported_passes(
        fn, thin.shape, thin.radius, bias=True, noise=2, fast=True)
    assert (fused == -5) == (thin_fused == -5)
    if fused != -5:
        big, small = fused[0][index], thin_fused[0][thin_index]
        assert (big.family, big.segments, big.rows, big.radius_class) == (small.family, small.segments, small.rows, small.radius_class)
        assert [fused[1][index][f] for f in flags] == [thin_fused[1][thin_index][f] for f in flags]


def test_the_workload_table_states_what_the_issue_lists(fn):
    """The figures of the workloads themselves (I pass), so that the table above cannot drift along with the dispatcher."""
    def i_pass(shape, radius):
        return reported_passes(fn, shape, radius)[0][0]

    for batch, march, ring in ((1, (8, 32), (4, 64)), (3, (8, 32), (4, 64)), (8, (4, 64), (2, 128)), (16, (2, 128), (1, 256)),
                               (32, (1, 256), (1, 256)), (64, (1, 256), (1, 256))):
        shape = (batch, 1, 256, 256, 256)
        p = i_pass(shape, (4, 4, 4))
        assert (p.family, p.segments, p.rows) == ("march", *march), (batch, p)
        p = i_pass(shape, (12, 12, 4))
        assert (p.family, p.segments, p.rows) == ("ring", *ring), (batch, p)
    p = i_pass((1, 2, 512, 512, 512), (4, 4, 4))
    assert (p.family, p.segments, p.rows, p.k_tiles) == ("march", 4, 128, 2)
    p = i_pass((1, 2, 512, 512, 512), (12, 12, 4))
    assert (p.family, p.segments, p.rows, p.k_tiles) == ("ring", 2, 256, 2)
    # 240 x 240 x 155: K is no multiple of 4 — the generic kernels, whatever the counts; at K = 156 the counts decide
    p = i_pass((8, 4, 240, 240, 155), (4, 4, 4))
    assert (p.family, p.segments, p.rows) == ("line", 8, 32)
    p = i_pass((8, 4, 240, 240, 156), (4, 4, 4))
    assert (p.family, p.segments, p.rows) == ("march", 2, 120)
    p = i_pass((8, 4, 240, 240, 156), (12, 12, 4))
    assert (p.family, p.segments, p.rows) == ("ring", 1, 240)


def test_switches_and_alignment_move_the_choice(fn, monkeypatch):
    shape, radius = (32, 1, 256, 16, 8), (4, 3, 5)
    passes, _ = reported_passes(fn, shape, radius)
    assert [p.family for p in passes] == ["march", "march"] and passes[1].radius_k == 5
    monkeypatch.setenv("TIO_CONV_RING", "1")
    fn["reload_env"]()
    passes, _ = reported_passes(fn, shape, radius)
    assert [(p.family, p.segments, p.rows) for p in passes] == [("ring", 4, 64), ("ring", 1, 16)] and passes[1].radius_k == 5
    monkeypatch.delenv("TIO_CONV_RING")
    monkeypatch.setenv("TIO_CONV_NO_FUSE", "1")
    fn["reload_env"]()
    passes, _ = reported_passes(fn, shape, radius)
    assert [p.family for p in passes] == ["march", "march", "k_v4"] and all(p.radius_k == 0 for p in passes)
    assert reported_passes(fn, shape, radius, bias=True) == -5
    monkeypatch.delenv("TIO_CONV_NO_FUSE")
    fn["reload_env"]()
    # a misaligned input, or another dtype at both ends: the generic kernels
    passes, _ = reported_passes(fn, shape, radius, aligned=False)
    assert [p.family for p in passes] == ["line", "line", "k"]
    assert reported_passes(fn, shape, radius, aligned=False, noise=1) == -5
    passes, _ = reported_passes(fn, shape, radius, dtype=torch.float16)
    assert [p.family for p in passes] == ["line", "march", "k"]  # only the middle pass is float32 at both ends
    assert reported_passes(fn, shape, (0, 0, 0)) == ([], [])
    assert reported_passes(fn, shape, (0, 0, 49)) == -1 and b"radius" in fn["last_error"]()


def test_a_pass_with_more_than_65535_lines_is_refused_before_any_launch(fn):
    """The generic kernels enumerate the lines of a pass — (the other non-K axis, or I for the K pass) x B x C — along grid.z;
    the dispatcher applies that limit to every family and refuses the call as a whole."""
    at_limit, beyond = (255, 257, 1, 4, 4), (256, 256, 1, 4, 4)
    passes, _ = reported_passes(fn, at_limit, (0, 1, 1))
    assert [p.key() for p in passes] == [Pass(1, "march", 1, 4, 1, 1, 1).key()]
    passes, stages = reported_passes(fn, at_limit, (0, 1, 1), dtype=torch.float64)
    assert [p.family for p in passes] == ["line", "k"] and [s["grid"][2] for s in stages] == [65535, 65535]
    for dtype in (torch.float32, torch.float64):
        assert reported_passes(fn, beyond, (0, 1, 1), dtype=dtype) == -1
        assert b"too large" in fn["last_error"]()
        assert reported_passes(fn, beyond, (0, 0, 1), dtype=dtype) == -1  # the K pass alone: I x B x C lines
    # the limit is on the lines of each pass: with the I axis active its lines are J x B x C
    assert reported_passes(fn, at_limit, (1, 1, 1)) == -1


# -- the oracle against float64 ----------------------------------------------------------------------------------------------
def test_bound_factor_is_the_stated_formula():
    u = 2.0**-24
    g = lambda k: k * u / (1 - k * u)  # noqa: E731
    assert bound_factor((4, 0, 0)) == pytest.approx(g(10), rel=1e-12)
    assert bound_factor((16, 12, 8)) == pytest.approx((1 + g(34)) * (1 + g(26)) * (1 + g(18)) - 1, rel=1e-9)
    assert bound_factor((0, 0, 0)) == 0.0


def test_float64_reference_on_a_hand_computed_line():
    data = torch.tensor([1.0, -2.0, 4.0, 8.0]).reshape(1, 1, 4, 1, 1)
    taps = torch.zeros(1, 3, 8)
    taps[0, 0, :3] = torch.tensor([0.5, 0.25, 0.125])  # asymmetric: tap 0 weighs the row BEFORE the output
    out = reference64(data, taps, (1, 0, 0)).flatten().tolist()
    assert out == [0.5 * 1 + 0.25 * 1 + 0.125 * -2, 0.5 * 1 + 0.25 * -2 + 0.125 * 4, 0.5 * -2 + 0.25 * 4 + 0.125 * 8,
                   0.5 * 4 + 0.25 * 8 + 0.125 * 8]


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_oracle_is_within_the_float64_bound(oracle, name):
    case = SWEEP[name]
    data, taps, skip = make_inputs(name)
    got = oracle.separable_conv3d(data, taps, list(case.radius), skip=skip)
    ref = reference64(data, taps, case.radius, skip)
    scale = reference64(data, taps, case.radius, skip, absolute=True)
    ok, ratio = within_bound(got, ref, scale, case.radius, skip)
    print(f"{name}: oracle error / bound = {ratio:.3f}")
    assert ok, f"{name}: oracle error is {ratio:.3f} of the float64 bound"
    assert 0.0 < ratio  # (float32 sums of 3 .. 33 terms do round: an error of exactly zero means nothing was compared)
    if skip is not None:
        assert torch.equal(got[skip.bool()], data[skip.bool()])
