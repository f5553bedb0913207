"""Volumes with NaN / +inf / -inf voxels and the geometries they are resampled through: shared by ``test_nonfinite_host.py``
(pins the oracle against stock ATen on the CPU) and the two GPU modules (``test_gpu_nonfinite_resample.py``,
``test_gpu_nonfinite_movers.py``).  CPU tensors only; no test functions.

Why non-finite voxels: a tap that is masked by a zero WEIGHT instead of by a select gives ``0 * finite = 0`` and no
finite input can tell the two apart; neither can it show a staged cell that was never written but meets a zero weight.
``F.grid_sample(padding_mode="zeros")`` adds ``value * weight`` for every in-bounds tap, including a tap whose weight is
exactly 0, and skips the out-of-bounds ones: ``inf * 0`` is NaN at the neighbours of an infinite voxel under an identity
mapping and nowhere beyond the 2 x 2 x 2 footprint.

The planted sites (per shape): both volume corners, both sides of a 16-voxel brick seam, two row ends with the first
voxel of the row behind each (what a 16-byte chunk that runs past a row of ``K % 4 != 0`` voxels would pick up), and two interior
voxels with even indices.  The
values are assigned so that the oracle's output holds all three classes in every geometry below (asserted by every test
that uses a case): +inf survives only where no tap of the same output voxel has a zero weight or a NaN / -inf value, so it
sits on interior sites of its own.
"""
from __future__ import annotations

import functools
import math

import torch

from case_inputs import _control_points
from case_inputs import _data
from case_inputs import _mapping

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
SENTINEL = 1.0e30  # finite: replaces the planted values to find the taps with a non-zero weight (`must_and_may`)

RAGGED, ALIGNED = (40, 37, 75), (64, 48, 96)  # K % 4 != 0: scalar staging, partial bricks; K % 4 == 0: 16-byte staging
SHAPES = (RAGGED, ALIGNED)
BATCH, CHANNELS = 2, 2


def planted_sites(shape, thick: bool = False) -> list[tuple[tuple[int, int, int], float]]:
    """``[((i, j, k), value), ...]``: the sites of the module docstring with their values.  *thick*: every site widened to
    a 4 x 4 x 4 block around it, clipped to the volume (later sites overwrite earlier ones) — a geometry that samples
    every third voxel looks past most single voxels, and a nearest image past a block narrower than the sampling step."""
    i, j, k = shape
    sites = [
        ((0, 0, 0), NAN),
        ((i - 1, j - 1, k - 1), NINF),
        ((15, 15, 15), NINF),  # last voxel of the first brick ...
        ((16, 16, 16), PINF),  # ... and the first of the next one, on every axis
        ((24, 9, k - 1), NAN),  # the last voxel of a row ...
        ((24, 10, 0), PINF),  # ... and the first voxel of the next row
        ((30, 20, k - 1), PINF),  # a second row end, the other way round
        ((30, 21, 0), NINF),
        ((22, 30, 40), NAN),  # interior sites with even indices: what a nearest image sees under a half-voxel shift, whose
        ((34, 12, 52), NINF),  # ties round to even
    ]
    if not thick:
        return sites
    block = [-1, 0, 1, 2]
    wide = [((a + da, b + db, c + dc), value) for (a, b, c), value in sites for da in block for db in block for dc in block]
    return [(site, value) for site, value in wide if all(0 <= x < n for x, n in zip(site, shape))]


def poisoned(shape, dtype=torch.float32, sites=None, *, channel: int = 0, seed: int = 21) -> tuple[torch.Tensor, torch.Tensor]:
    """``(volume, clean)``, both ``(2, 2, I, J, K)`` from ``case_inputs._data``: *volume* carries the planted values in
    element 0, channel *channel* only; element 1 and the other channel stay clean, so cross-talk between the two channels
    of the pair kernel, or between batch elements, is visible."""
    clean = _data((BATCH, CHANNELS, *shape), dtype, seed)
    volume = clean.clone()
    for site, value in planted_sites(shape) if sites is None else sites:
        volume[(0, channel, *site)] = value
    return volume, clean


def with_sentinel(volume: torch.Tensor, value: float = SENTINEL) -> torch.Tensor:
    """*volume* with every non-finite voxel replaced by the finite *value*."""
    return torch.where(torch.isfinite(volume), volume, torch.full_like(volume, value))


# -- geometries -------------------------------------------------------------------------------------------------------
def _identity(batch):
    return torch.eye(3, 4).repeat(batch, 1, 1)


def _rotation(shape, degrees, batch):
    """A rotation by *degrees* about every axis, about the volume's centre, shifted by 1.5 voxels (``case_inputs._rotation_mapping``
    for a volume that is no cube): from about 25 degrees a brick's input box exceeds the staging tile."""
    angle = math.radians(degrees)
    c, s = math.cos(angle), math.sin(angle)
    rx = torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float64)
    ry = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    rz = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64)
    rotation = rz @ ry @ rx
    centre = torch.tensor([(n - 1) / 2.0 for n in shape], dtype=torch.float64)
    shift = centre - rotation @ centre + 1.5
    return torch.cat([rotation, shift[:, None]], dim=1).to(torch.float32)[None].repeat(batch, 1, 1)


#: seed of the random mappings.  Recorded: with this seed no coordinate of the affine / elastic geometries lies within
#: float32 rounding of an integer at a planted site, so the oracle's chain and stock ATen's pick the same taps
#: (test_nonfinite_host.py asserts the set equalities; a seed that parks one there is replaced, the assertion stays)
MAPPING_SEED, CONTROL_SEED = 22, 23

GEOMETRIES = ("identity", "half", "affine", "elastic", "elastic_cp_first", "elastic3", "down3", "rot25")


def geometry(name: str, shape) -> dict:
    """The geometry keywords of ``Engine.resample3d`` for one named case on a ``(2, 2, *shape)`` volume.

    identity / half (all axes + 0.5): exact coordinates in every float32 chain; affine: ``_mapping(scale=0.05, shift=1.5)``;
    elastic: the same with ``_control_points((7, 7, 7), amplitude=3.0)``, ``elastic_cp_first`` composes the other way round;
    elastic3: a 3 x 3 x 3 control grid (cells at least a brick wide: what the planned lean road asks for); down3: the
    down-sampling by 3 of ``test_tile_oversize_boxes_split_or_fall_back`` (boxes beyond the staging tile: passes, or voxel
    by voxel); rot25: 25 degrees about every axis (``test_gpu_large_boxes.py``: two / four passes)."""
    out_shape, out_spacing, control, affine_first = tuple(shape), (1.0, 1.0, 1.0), None, True
    if name == "identity":
        mapping = _identity(BATCH)
    elif name == "half":
        mapping = _identity(BATCH)
        mapping[:, :, 3] = 0.5
    elif name in ("affine", "elastic", "elastic_cp_first", "elastic3"):
        mapping = _mapping(BATCH, MAPPING_SEED, scale=0.05, shift=1.5)
        if name != "affine":
            control = _control_points(BATCH, (3, 3, 3) if name == "elastic3" else (7, 7, 7), CONTROL_SEED, amplitude=3.0)
        affine_first = name != "elastic_cp_first"
    elif name == "down3":
        mapping = _mapping(BATCH, 42, scale=0.05, shift=2.0)
        mapping[:, :, :3] *= 3.0
        out_shape, out_spacing = tuple(-(-n // 3) for n in shape), (3.0, 3.0, 3.0)
    elif name == "rot25":
        mapping = _rotation(shape, 25.0, BATCH)
    else:
        raise KeyError(name)
    return dict(out_shape=out_shape, mapping=mapping, control_points=control, in_spacing=(1.0, 1.0, 1.0), out_spacing=out_spacing,
                affine_first=affine_first)


FILL = (-1.0, 0.5)


def resample_kwargs(name: str, shape, with_fill: bool, interp: str = "linear") -> dict:
    return dict(geometry(name, shape), interps=[interp], fills=[torch.tensor(FILL) if with_fill else None])


# -- comparison helpers -------------------------------------------------------------------------------------------------
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer view of a tensor (same element size): comparisons on it see NaN payloads and the sign of zero."""
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def same_bits_or_both_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal bit for bit, except that any NaN matches any NaN (arithmetic does not define a produced NaN's payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((bits(a) == bits(b)) | (a.isnan() & b.isnan())).all())


def classes(t: torch.Tensor) -> dict:
    """How many NaN, +inf and -inf values a tensor holds."""
    return {"nan": int(t.isnan().sum()), "+inf": int((t == PINF).sum()), "-inf": int((t == NINF).sum())}


def assert_case_is_not_vacuous(expected: torch.Tensor, channel: int) -> None:
    """What every parametrised case asserts of its oracle output: all three classes present, in element 0's poisoned
    channel only."""
    found = classes(expected[0, channel])
    assert all(found.values()), f"a class is missing from the oracle's output: {found}"
    assert bool(torch.isfinite(expected[0, 1 - channel]).all()), "the clean channel is not finite"
    assert bool(torch.isfinite(expected[1]).all()), "the clean element is not finite"


def must_and_may(oracle, case: dict) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(N, MUST, MAY)`` as boolean masks over the output of ``case = dict(volume=, clean=, kwargs=)``.

    N: where the oracle's output of the poisoned volume is not finite.  MUST: where its output changes against the clean run
    when the planted values are replaced by the finite sentinel 1e30 — the taps with a non-zero weight; a kernel of any
    interpolation order gives a non-finite value there.  MAY = N without MUST: the planted voxel is an in-bounds tap of weight
    exactly 0 (``0 * inf``).  Only the oracle is run: no weight is restated here."""
    run = lambda data: oracle.resample3d([data], **case["kwargs"])[0]  # noqa: E731
    n = ~torch.isfinite(run(case["volume"]))
    must = run(with_sentinel(case["volume"])) != run(case["clean"])
    assert bool((must & ~n).sum() == 0), "a tap with a non-zero weight gave a finite output"
    return n, must, n & ~must


@functools.lru_cache(maxsize=None)
def resample_case(name: str, shape, with_fill: bool, channel: int, interp: str = "linear") -> dict:
    """One cached case (the tensors are shared between tests: leave them unchanged)."""
    volume, clean = poisoned(shape, torch.float32, planted_sites(shape, thick=name == "down3"), channel=channel)
    return dict(volume=volume, clean=clean, kwargs=resample_kwargs(name, shape, with_fill, interp), channel=channel)


# -- bit patterns for the pure moves ----------------------------------------------------------------------------------
#: float32 patterns a move must carry unchanged: a quiet NaN with a payload, a signalling NaN, the negative quiet NaN,
#: -0.0, the infinities, the smallest and the largest float32 subnormal, a float16 subnormal's float32 value
PAYLOADS_F32 = (0x7FC00001, 0x7F800001, 0xFFC00000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x007FFFFF, 0x33800000)
PAYLOADS_F16 = (0x7E01, 0x7C01, 0xFE00, 0x8000, 0x7C00, 0xFC00, 0x0001, 0x03FF)
PAYLOADS_BF16 = (0x7FC1, 0x7F81, 0xFFC0, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x007F)
PAYLOADS_F64 = (0x7FF8000000000001, 0x7FF0000000000001, -0x0008000000000000, -0x8000000000000000, 0x7FF0000000000000,
                -0x0010000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF)
PAYLOADS = {torch.float32: PAYLOADS_F32, torch.float16: PAYLOADS_F16, torch.bfloat16: PAYLOADS_BF16, torch.float64: PAYLOADS_F64}


def payload_volume(shape, dtype, seed: int) -> torch.Tensor:
    """Seeded data of *dtype* with the payload table written over every seventh voxel, cyclically: built on the integer
    view, so no arithmetic touches the patterns."""
    data = _data(shape, dtype, seed)
    view = bits(data).reshape(-1)
    table = torch.tensor(PAYLOADS[dtype], dtype=torch.int64).to(view.dtype)
    where = torch.arange(0, view.numel(), 7)
    view[where] = table[torch.arange(where.numel()) % table.numel()]
    return view.view(dtype).reshape(shape)
