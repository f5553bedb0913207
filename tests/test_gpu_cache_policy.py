"""GPU: the cache policy "stream" changes no bit (``torchio_amd/csrc/common.hpp``: ``launch_streams``).

A marching stencil pass that writes more than the Infinity Cache holds (256 MiB) takes the kernel whose once-touched rows are
loaded and stored nontemporal (``stencil_march.hpp``: ``conv_stream_march_kernel``).  Nothing of that size belongs in a test, so
``TIO_STREAM_BYTES=0`` makes every launch stream here, and a huge value none; both runs must agree bit for bit.

(The resampler's exact-coordinate kernels keep the default policy: nontemporal output stores were measured and lost,
``profiles/cache_policy.md``.  They are the producers of the Compose below, on the planned road — the Affine launch from 48^3 on;
the ElasticDeformation launch with 7^3 control points from 100^3 on, the smallest cube with 16-byte rows whose control cells are
a brick wide, ``n - 1 >= 16 * 6`` — so the Compose runs at 100^3, and the road is asserted through the plan report.)
"""
from __future__ import annotations

import copy

import pytest
import torch

import torchio_amd as tio
from parity_harness import nested_spheres
from stencil_geometry_cases import TAP_STRIDE, reported_passes
from test_gpu_resample_planned import starts_from_a_plan
from torchio_amd import ops, streams

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEVER = str(2**62)  # a threshold no launch exceeds

CUBE = 100


@pytest.fixture
def modes():
    """The library's process-wide modes and switches, put back whatever a test set."""
    previous = (tio.get_noise_rng(), tio.get_resample_precision(), tio.get_stencil_precision(), streams._AHEAD_ENABLED)
    yield
    tio.set_noise_rng(previous[0])
    tio.set_resample_precision(previous[1])
    tio.set_stencil_precision(previous[2])
    ops.set_ahead_stream(previous[3])
    ops.reload_env()  # (monkeypatch has put the environment back by the time the next test starts; this one reads it again anyway)


def _policy(monkeypatch, threshold: str) -> None:
    monkeypatch.setenv("TIO_STREAM_BYTES", threshold)
    monkeypatch.setenv("TIO_EXACT_LEAN", "2")  # (the exact-coordinate kernels for launches below the planned roads' 12 288 bricks too)
    ops.reload_env()


def _assert_lean_road(hip, which: str, cube: int, precision: str) -> None:
    geometry = dict(out_shape=(cube,) * 3, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True)
    mapping = torch.eye(3, 4).repeat(2, 1, 1).cuda()
    field = torch.zeros(2, 7, 7, 7, 3, device=DEV) if which == "elastic" else None
    data = torch.zeros(2, 1, cube, cube, cube, device=DEV)
    assert starts_from_a_plan(hip, [data], precision=precision, mapping=mapping, control_points=field, **geometry), (which, cube, precision)


def _run(transform, batch, seed: int):
    torch.manual_seed(seed)
    out = transform(copy.deepcopy(batch))
    torch.cuda.synchronize()
    return {name: image.data for name, image in out.images.items()}, [copy.deepcopy(dict(t.params)) for t in out.applied_transforms]


#: launch radii (I, J, K): every compile-time radius 2 .. 6 of the I pass and of the J pass, every K radius 2 .. 6
STENCIL_RADII = [(2, 3, 4), (3, 4, 5), (4, 5, 6), (5, 6, 2), (6, 2, 3)]
STENCIL_SHAPE = (2, 1, 40, 24, 32)


def _taps(radius, generator) -> torch.Tensor:
    """Per-element taps: element 0 uses the launch radii, element 1 radii one smaller (its outer taps are zero), asymmetric, sum one."""
    taps = torch.zeros((2, 3, TAP_STRIDE), dtype=torch.float32)
    for element in range(2):
        for axis, r in enumerate(radius):
            own = r - element
            w = torch.rand(2 * own + 1, generator=generator, dtype=torch.float64) + 0.05
            taps[element, axis, r - own : r + own + 1] = (w / w.sum()).to(torch.float32)
    return taps


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("radius", STENCIL_RADII, ids=lambda r: "r%d%d%d" % r)
def test_streaming_stencil_equals_the_default_policy(hip, modes, monkeypatch, radius, precision):
    """``tio_blur_fused`` with a bias field and Philox noise on 2 x 1 x 40 x 24 x 32: the marching I + bias pass and the fused
    J + K + noise pass (asserted through ``tio_separable_conv3d_passes``), streaming against not streaming."""
    g = torch.Generator().manual_seed(sum(radius))
    data = (torch.randn(STENCIL_SHAPE, generator=g) * 100.0).to(DEV)
    taps = _taps(radius, g).to(DEV)
    coarse = ((torch.rand((2, 1, 7, 3, 2), generator=g) - 0.5) * 0.6).to(DEV)
    noise = (torch.tensor([-3.0, 3.0]), torch.tensor([0.5, 20.0]), 0x1234_5678_9ABC_DEF0 + sum(radius))
    tio.set_stencil_precision(precision)
    passes, stages = reported_passes(hip._fn, STENCIL_SHAPE, radius, bias=True, noise=1, fast=precision == "fast")
    assert [(p.axis, p.family, p.radius_class, p.radius_k) for p in passes] == [(0, "march", radius[0], 0), (1, "march", radius[1], radius[2])]
    assert [(s["pre_bias"], s["post_noise"], s["fma"]) for s in stages] == [(1, 0, int(precision == "fast")), (0, 1, int(precision == "fast"))]
    _policy(monkeypatch, NEVER)
    plain = hip.blur_fused(data, taps, list(radius), bias_coarse=coarse, noise=noise)
    _policy(monkeypatch, "0")
    streamed = hip.blur_fused(data, taps, list(radius), bias_coarse=coarse, noise=noise)
    torch.cuda.synchronize()
    assert plain is not None and streamed is not None
    assert torch.equal(plain, streamed)
    assert bool(torch.isfinite(plain).all()) and not torch.equal(plain, data)


def _compose():
    return tio.Compose([
        tio.Affine(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5)),
        tio.ElasticDeformation(),
        tio.BiasField(),
        tio.Blur(std=(0.5, 2)),
        tio.Noise(),
    ])


_COMPOSE_PLAIN: dict = {}  # seed -> the run with the default policy (computed once, shared, never written)


@pytest.mark.parametrize("ahead", [False, True], ids=["plan_on_the_data_stream", "plan_on_the_side_stream"])
def test_consumers_read_what_streaming_stores_wrote(hip, modes, monkeypatch, ahead):
    """``Compose[Affine, ElasticDeformation, BiasField, Blur, Noise]`` on 2 x (float32 + int16) of 100^3, ten seeds: the fused
    J + K + noise pass reads what the streaming stores of the I + bias pass just wrote on the same stream, the I + bias pass
    streams through what the resampler (on the planned road, asserted) just wrote.  Once more with the resampler's
    brick plan made on the side stream.  Each run equals the run with the default policy bit for bit."""
    tio.set_noise_rng("philox")
    tio.set_resample_precision("tight")
    tio.set_stencil_precision("fast")
    g = torch.Generator().manual_seed(11)
    subjects = [tio.Subject(t1=tio.ScalarImage(torch.rand(1, CUBE, CUBE, CUBE, generator=g)),
                            seg=tio.LabelMap(nested_spheres(CUBE))) for _ in range(2)]
    batch = tio.SubjectsBatch.from_subjects(subjects).to(DEV)
    seeds = range(100, 110)
    if not _COMPOSE_PLAIN:
        ops.set_ahead_stream(False)
        _policy(monkeypatch, NEVER)
        for seed in seeds:
            _COMPOSE_PLAIN[seed] = _run(_compose(), batch, seed)
    ops.set_ahead_stream(ahead)
    _policy(monkeypatch, "0")
    for which in ("affine", "elastic"):
        _assert_lean_road(hip, which, CUBE, "tight")
    for seed in seeds:
        streamed, params = _run(_compose(), batch, seed)
        plain, plain_params = _COMPOSE_PLAIN[seed]
        assert params == plain_params, seed
        for name in plain:
            assert torch.equal(plain[name], streamed[name]), (seed, name)
        assert not torch.equal(streamed["t1"], batch.images["t1"].data)


def test_threshold_of_the_host_side_decision(hip, modes, monkeypatch):
    """``tio_launch_streams`` alone (nothing is allocated or launched): without an override a launch streams when it writes more
    than 256 MiB — the bench's 8 x 256^3 float32 volumes do, a 64^3 subject, a patch and a batch of exactly 256 MiB do not."""
    decide = hip._fn["launch_streams"]
    monkeypatch.delenv("TIO_STREAM_BYTES", raising=False)
    ops.reload_env()
    mib = 2**20
    assert decide(8 * 256**3 * 4) == 1 and decide(256 * mib + 1) == 1 and decide(2**40) == 1
    assert decide(256 * mib) == 0 and decide(4 * 256**3 * 4) == 0 and decide(64**3 * 4) == 0 and decide(0) == 0
    monkeypatch.setenv("TIO_STREAM_BYTES", "0")
    ops.reload_env()
    assert decide(1) == 1 and decide(64**3 * 4) == 1 and decide(0) == 0
    monkeypatch.setenv("TIO_STREAM_BYTES", NEVER)
    ops.reload_env()
    assert decide(8 * 256**3 * 4) == 0 and decide(2**40) == 0
    monkeypatch.setenv("TIO_STREAM_BYTES", str(32 * mib))
    ops.reload_env()
    assert decide(32 * mib) == 0 and decide(32 * mib + 1) == 1
