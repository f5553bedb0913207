"""The fused J + K marching kernels against the separate launches, at every compile-time radius and every K tier.

The fused J + K instantiations of ``conv_march_kernel`` live in a translation unit of their own (``stencil_fused.hip``, built
without the SLP vectoriser) and are reached through a launcher of their own.  What can go wrong in such a split — a launch routed
to another instantiation, a helper that exists twice with a difference — shows at the smallest shapes where the marching loop
itself can go wrong, so these pass before the split as well:

* B = 2 with per-instance taps, means and standard deviations, one channel, 37 x 37 x 256 and 37 x 37 x 8: 37 is prime and
  above 2W for every window (W = 2R + 1 <= 17): the wave-uniform early return is taken inside the unrolled body for every R and the
  window wraps more than twice; K = 256 fills all 64 lanes of the K stage, K = 8 leaves 62 idle and the replicated edges of both
  sides sit next to each other;
* J radius 1 .. 8 (every compile-time radius) x K radius 1, 4, 5, 6, 7, 8 (every tier and both sides of each boundary);
* noise none / Philox / explicit draws, BiasField on and off, stencil precision exact and fast.

``tio_blur_fused`` is held BIT FOR BIT to the separate launches ``bias_field_apply -> separable_conv3d -> add_noise``.  The
fused multiply-add taps of the fast precision exist only inside ``tio_blur_fused``, so there the separate stencil launch is
``tio_blur_fused`` without stages, held to ``2e-6 * max|exact|`` of the exact one (the bar of ``test_gpu_stencil_geometry``), on
the small shape also to the float32 rounding bound of a float64 correlation, and required to DIFFER from the exact one (a fast
launch routed to an exact instantiation would pass everything else).  In exact mode the result is the CPU oracle's bit for bit
as well: the oracle's stencil on the engine's bias output (the two ``expf`` differ) and the oracle's ``add_noise`` on the
engine's draws (Philox: ``philox_normal``, the stream the kernels draw from; the hardware log2 and sqrt are not libm's).
"""
from __future__ import annotations

import pytest
import torch

from stencil_geometry_cases import TAP_STRIDE, reference64, reported_passes, within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = {"k256": (2, 1, 37, 37, 256), "k8": (2, 1, 37, 37, 8)}
K_RADII = (1, 4, 5, 6, 7, 8)
SEED = 0x0FED_CBA9_8765_4321

_shared: dict = {}


def _inputs(hip, shape_name):
    """Per shape, once: data, bias field, biased data, draws, Philox draws and noise parameters (device), and host copies."""
    if shape_name not in _shared:
        shape = SHAPES[shape_name]
        g = torch.Generator().manual_seed(1000 + shape[4])
        data = torch.randn(shape, generator=g) * 100.0 + (torch.arange(shape[3], dtype=torch.float32) * 3.0 - shape[3]).reshape(1, 1, 1, -1, 1)
        coarse = ((torch.rand((shape[0], shape[1], 7, 3, 2), generator=g) - 0.5) * 0.6).to(DEV)  # seven planes along I: cells are crossed
        draws = torch.randn(shape, generator=g)
        x = data.to(DEV)
        biased = hip.bias_field_apply(x, coarse)
        philox = hip.philox_normal(shape, SEED, 0, DEV)
        _shared[shape_name] = {
            "data": data, "x": x, "coarse": coarse, "biased": biased, "biased_cpu": biased.cpu(), "draws": draws.to(DEV), "draws_cpu": draws,
            "philox_cpu": philox.cpu(), "mean": torch.tensor([-3.0, 3.0]), "std": torch.tensor([0.5, 20.0]),
        }
    return _shared[shape_name]


def _taps(radius, seed):
    """Per-instance asymmetric taps that sum to one (a reversed or shifted tap order shows, which a Gaussian would hide)."""
    g = torch.Generator().manual_seed(seed)
    taps = torch.zeros((2, 3, TAP_STRIDE), dtype=torch.float32)
    for axis, r in enumerate(radius):
        w = torch.rand((2, 2 * r + 1), generator=g, dtype=torch.float64) + 0.05
        taps[:, axis, : 2 * r + 1] = (w / w.sum(dim=1, keepdim=True)).to(torch.float32)
    return taps


def _same(got, expected, what):
    differing = int((got != expected).sum())
    assert differing == 0, f"{what}: {differing} of {got.numel()} voxels differ"


@pytest.mark.parametrize("rj", range(1, 9))
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_fused_jk_equals_the_separate_launches(oracle, hip, shape_name, rj):
    import torchio_amd as tio

    shape = SHAPES[shape_name]
    s = _inputs(hip, shape_name)
    mean, std = s["mean"], s["std"]
    previous = tio.get_stencil_precision()
    try:
        for rk in K_RADII:
            radius = [(rj + rk) % 6 + 1, rj, rk]  # the I pass marches as well, with and without the bias field (radius <= 6)
            taps = _taps(radius, 100 * rj + rk)
            taps_dev = taps.to(DEV)
            for fast in (False, True):  # the launch is the fused J + K instantiation of this radius, with these stages
                for noise_on in (0, 1, 2):
                    passes, stages = reported_passes(hip._fn, shape, radius, bias=True, noise=noise_on, fast=fast)
                    assert [(p.axis, p.family, p.radius_class, p.radius_k) for p in passes] == [(0, "march", radius[0], 0), (1, "march", rj, rk)]
                    assert [(t["pre_bias"], t["post_noise"], t["fma"]) for t in stages] == [(1, 0, int(fast)), (0, noise_on, int(fast))]
            for bias in (False, True):
                what = f"{shape_name} radius {radius} bias {bias}"
                source, source_cpu = (s["biased"], s["biased_cpu"]) if bias else (s["x"], s["data"])
                coarse = s["coarse"] if bias else None
                # -- exact: the separate launches, and the oracle
                tio.set_stencil_precision("exact")
                blurred = hip.separable_conv3d(source, taps_dev, radius)
                blurred_oracle = oracle.separable_conv3d(source_cpu, taps, radius)
                chains = {
                    "none": (None, blurred, blurred_oracle),
                    "philox": ((mean, std, SEED), hip.add_noise(blurred, mean, std, philox_seed=SEED),
                               oracle.add_noise(blurred_oracle, mean, std, base1=s["philox_cpu"])),
                    "draws": ((mean, std, s["draws"]), hip.add_noise(blurred, mean, std, base1=s["draws"]),
                              oracle.add_noise(blurred_oracle, mean, std, base1=s["draws_cpu"])),
                }
                exact_plain = None
                for form, (noise, chain, chain_oracle) in chains.items():
                    exact = hip.blur_fused(s["x"], taps_dev, radius, bias_coarse=coarse, noise=noise)
                    assert exact is not None, f"{what} {form}: no fused form"
                    _same(exact, chain, f"{what} noise {form}: exact blur_fused against the separate launches")
                    _same(exact.cpu(), chain_oracle, f"{what} noise {form}: exact blur_fused against the oracle")
                    if form == "none":
                        exact_plain = exact
                # -- fast: the stages around the fused launch without stages, and that launch against the exact one
                tio.set_stencil_precision("fast")
                fast_plain = hip.blur_fused(source, taps_dev, radius)
                assert fast_plain is not None, what
                gap, bar = float((fast_plain - exact_plain).abs().max()), 2e-6 * float(exact_plain.abs().max())
                print(f"{what}: fast - exact = {gap:.3e}, bar {bar:.3e}")
                assert gap <= bar, f"{what}: fast mode {gap:.3e} from exact, bar {bar:.3e}"
                assert gap > 0.0, f"{what}: the fast launch gave the exact one's bits: it ran no fused multiply-add"
                if shape_name == "k8":
                    ref, scale = reference64(source_cpu, taps, radius), reference64(source_cpu, taps, radius, absolute=True)
                    ok, ratio = within_bound(fast_plain.cpu(), ref, scale, radius)
                    print(f"{what}: fast error / float64 bound = {ratio:.3f}")
                    assert ok, f"{what}: fast mode at {ratio:.3f} of the float64 bound"
                fast_chains = {
                    "none": (None, fast_plain),
                    "philox": ((mean, std, SEED), hip.add_noise(fast_plain, mean, std, philox_seed=SEED)),
                    "draws": ((mean, std, s["draws"]), hip.add_noise(fast_plain, mean, std, base1=s["draws"])),
                }
                for form, (noise, chain) in fast_chains.items():
                    got = hip.blur_fused(s["x"], taps_dev, radius, bias_coarse=coarse, noise=noise)
                    assert got is not None, f"{what} {form}: no fused form"
                    _same(got, chain, f"{what} noise {form}: fast blur_fused against bias_field_apply -> blur_fused -> add_noise")
    finally:
        tio.set_stencil_precision(previous)
