"""The separable stencil at every launch geometry its dispatcher can choose, on thin volumes.

The cases and their labels are those of ``tests/stencil_geometry_cases.py`` (``tests/test_stencil_passes.py`` shows on the CPU
that they reach the segmentations of the 256^3 workloads).  Per case:

1. the dispatcher reports the labelled passes (in this process, under the case's switches);
2. ``separable_conv3d`` equals the CPU oracle bit for bit;
3. it lies within the derived float32 rounding bound of a float64 correlation;
4. with one ``inf`` ``radius`` rows before the first seam and one ``radius + 1`` rows after it, the non-finite outputs are the
   oracle's and every finite value is equal — a halo that is a row short, or a window that is a row off, shows here;
5. ``blur_fused`` with a bias field, with Philox noise and with explicit draws equals, in exact mode, the chain
   ``bias_field_apply -> separable_conv3d -> add_noise`` of the same engine bit for bit (whose conv step equals the oracle);
   in fast mode it stays within ``2e-6 * max|exact|`` of it, and the plain fast form within the float64 bound.
"""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from stencil_geometry_cases import SWEEP, TAP_STRIDE, expected_bias_passes, make_inputs, plant_infs, reference64, reported_passes
from stencil_geometry_cases import within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_same_with_non_finite(expected: torch.Tensor, got: torch.Tensor, what: str) -> None:
    finite = torch.isfinite(expected)
    assert not bool(finite.all()), f"{what}: the planted values reached no output"
    assert torch.equal(finite, torch.isfinite(got)), f"{what}: another set of non-finite outputs"
    assert torch.equal(expected[finite], got[finite]), f"{what}: finite values differ"


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_stencil_geometry(oracle, hip, monkeypatch, name):
    import torchio_amd as tio

    case = SWEEP[name]
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)  # (tests/conftest.py: a write to a TIO_* variable reloads the library's switches)
    fn = hip._fn
    radius = list(case.radius)
    data, taps, skip = make_inputs(name)
    # 1. the launch is the labelled one
    passes, _ = reported_passes(fn, case.shape, case.radius, has_skip=skip is not None)
    assert [p.key() for p in passes] == [p.key() for p in case.passes]
    # 2. bit for bit against the oracle
    expected = oracle.separable_conv3d(data, taps, radius, skip=skip)
    x_dev, taps_dev, skip_dev = data.to(DEV), taps.to(DEV), None if skip is None else skip.to(DEV)
    got = hip.separable_conv3d(x_dev, taps_dev, radius, skip=skip_dev).cpu()
    differing = int((got != expected).sum())
    print(f"{name}: {differing} of {got.numel()} voxels differ from the oracle")
    assert torch.equal(got, expected), f"{name}: {differing} voxels differ from the oracle"
    # 3. within the float64 bound
    ref = reference64(data, taps, case.radius, skip)
    scale = reference64(data, taps, case.radius, skip, absolute=True)
    ok, ratio = within_bound(got, ref, scale, case.radius, skip)
    print(f"{name}: error / float64 bound = {ratio:.3f}")
    assert ok, f"{name}: {ratio:.3f} of the float64 bound"
    # 4. non-finite values around the first seam
    poisoned = plant_infs(case, data)
    assert int((~torch.isfinite(poisoned)).sum()) == 2
    _assert_same_with_non_finite(oracle.separable_conv3d(poisoned, taps, radius, skip=skip),
                                 hip.separable_conv3d(poisoned.to(DEV), taps_dev, radius, skip=skip_dev).cpu(), name)
    # 5. the stages of blur_fused
    if not case.fused_form:
        assert hip.blur_fused(x_dev, taps_dev, radius, bias_coarse=None, noise=(0.0, 1.0, 5)) is None
        return
    b, c = case.shape[:2]
    g = torch.Generator().manual_seed(len(name))
    coarse = ((torch.rand((b, c, 7, 3, 2), generator=g) - 0.5) * 0.6).to(DEV)  # seven planes along I: the cell cache is crossed
    draws = torch.randn(case.shape, generator=g).to(DEV)
    mean, std = (torch.linspace(-3.0, 3.0, b), torch.linspace(0.5, 20.0, b)) if case.per_element_taps else (1.5, 12.0)
    seed = 0x1234_5678_9ABC_DEF0 + len(name)
    plain = hip.separable_conv3d(x_dev, taps_dev, radius) if skip is not None else got.to(DEV)
    plain_cpu = plain.cpu()
    if skip is not None:  # (blur_fused has no skipped rows)
        ref, scale = reference64(data, taps, case.radius), reference64(data, taps, case.radius, absolute=True)
    got_bias, stages = reported_passes(fn, case.shape, case.radius, bias=True, noise=2)
    assert [p.key() for p in got_bias] == [p.key() for p in expected_bias_passes(case)]
    assert [(s["pre_bias"], s["post_noise"]) for s in stages] == [(1, 0), (0, 2)]
    biased = hip.bias_field_apply(x_dev, coarse)
    blurred = hip.separable_conv3d(biased, taps_dev, radius)
    assert torch.equal(blurred.cpu(), oracle.separable_conv3d(biased.cpu(), taps, radius)), "the chain's conv step against the oracle"
    forms = {
        "plain": (None, None, plain),
        "bias": (coarse, None, blurred),
        "philox": (None, (mean, std, seed), hip.add_noise(plain, mean, std, philox_seed=seed)),
        "bias+draws": (coarse, (mean, std, draws), hip.add_noise(blurred, mean, std, base1=draws)),
        "bias+philox": (coarse, (mean, std, seed), hip.add_noise(blurred, mean, std, philox_seed=seed)),
    }
    previous = tio.get_stencil_precision()
    try:
        for form, (bias, noise, chain) in forms.items():
            tio.set_stencil_precision("exact")
            exact = hip.blur_fused(x_dev, taps_dev, radius, bias_coarse=bias, noise=noise)
            assert exact is not None, form
            differing = int((exact != chain).sum())
            print(f"{name}: blur_fused[{form}]: {differing} voxels differ from the chain")
            assert torch.equal(exact, chain), f"{name}: blur_fused[{form}] differs from the chain in {differing} voxels"
            tio.set_stencil_precision("fast")
            fast = hip.blur_fused(x_dev, taps_dev, radius, bias_coarse=bias, noise=noise)
            assert fast is not None, form
            gap, bar = float((fast - exact).abs().max()), 2e-6 * float(exact.abs().max())
            print(f"{name}: blur_fused[{form}]: fast - exact = {gap:.3e}, bar {bar:.3e}")
            assert gap <= bar, f"{name}: blur_fused[{form}]: fast mode {gap:.3e} from exact, bar {bar:.3e}"
            if form == "plain":
                assert torch.equal(exact.cpu(), plain_cpu)
                ok, ratio = within_bound(fast.cpu(), ref, scale, case.radius)
                print(f"{name}: fast error / float64 bound = {ratio:.3f}")
                assert ok, f"{name}: fast mode at {ratio:.3f} of the float64 bound"
    finally:
        tio.set_stencil_precision(previous)


# -- the limit of 65 535 lines per pass -----------------------------------------------------------------------------------------
def _line_limit_inputs(shape):
    g = torch.Generator().manual_seed(65535)
    data = torch.randn(shape, generator=g) * 100.0
    taps = torch.zeros((1, 3, TAP_STRIDE))
    for axis in (1, 2):
        w = torch.rand(3, generator=g, dtype=torch.float64) + 0.05
        taps[0, axis, :3] = (w / w.sum()).to(torch.float32)
    return data, taps


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32_march", "float64_generic"])
def test_a_pass_of_65535_lines_runs(oracle, hip, dtype):
    """B * C * I = 255 * 257 * 1 lines in the J pass and in the K pass: the last grid the generic kernels can enumerate along z
    (float64 runs them; float32 takes the marching kernel under the same rule)."""
    shape, radius = (255, 257, 1, 4, 4), [0, 1, 1]
    data, taps = _line_limit_inputs(shape)
    data = data.to(dtype)
    passes, stages = reported_passes(hip._fn, shape, radius, dtype=dtype)
    assert [p.family for p in passes] == (["march"] if dtype == torch.float32 else ["line", "k"])
    if dtype == torch.float64:
        assert [s["grid"][2] for s in stages] == [65535, 65535]
    expected = oracle.separable_conv3d(data, taps, radius)
    got = hip.separable_conv3d(data.to(DEV), taps.to(DEV), radius).cpu()
    assert torch.equal(got, expected)
    if dtype == torch.float32:
        ref, scale = reference64(data, taps, radius), reference64(data, taps, radius, absolute=True)
        ok, ratio = within_bound(got, ref, scale, radius)
        assert ok, ratio


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_a_pass_of_65536_lines_is_refused_and_writes_nothing(hip, dtype):
    from torchio_amd import _abi, ops

    shape, radius = (256, 256, 1, 4, 4), [0, 1, 1]
    assert reported_passes(hip._fn, shape, radius, dtype=dtype) == -1
    data, taps = _line_limit_inputs(shape)
    x, taps_dev = data.to(dtype).to(DEV), taps.to(DEV)
    with pytest.raises(ops.EngineError, match=r"tio_separable_conv3d failed with status -1: tio_separable_conv3d: volume too large"):
        hip.separable_conv3d(x, taps_dev, radius)
    # the C entry point itself, on buffers of ours: nothing may have been written
    sentinel = -12345.0
    y = torch.full_like(x, sentinel)
    tmp = torch.full((2, *shape), sentinel, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    status = hip._fn["separable_conv3d"](
        C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(tmp.data_ptr()), ops.dtype_code(dtype), shape[0], shape[1],
        (C.c_int32 * 3)(*shape[2:]), C.c_void_p(taps_dev.data_ptr()), 0, TAP_STRIDE, (C.c_int32 * 3)(*radius), None,
        hip._stream(x))
    assert status == -1 != _abi.OK
    assert b"tio_separable_conv3d" in hip._fn["last_error"]()
    torch.cuda.synchronize()
    assert bool((y == sentinel).all()) and bool((tmp == sentinel).all())
    # the K pass alone has I * B * C lines as well
    with pytest.raises(ops.EngineError, match="tio_separable_conv3d"):
        hip.separable_conv3d(x, taps_dev, [0, 0, 1])
