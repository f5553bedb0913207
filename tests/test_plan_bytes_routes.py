"""Which resampling calls start from a brick plan, and which plan layout: ``tio_resample3d_plan_bytes`` on the CPU.

``tio_resample3d_plan_bytes`` makes no GPU call: it runs the dispatcher's route choice for one float32 trilinear image
and answers the size of the plan that geometry's launch would start from (0: no plan).  The table below crosses the
precision modes, the large-box hints, control points, spacing, sizes on both sides of the planned-brick threshold and the
``TIO_*`` switches that move a call from one road to another; the expected integers were recorded from the library
before the dispatcher was split into route choice and launch helpers (``tests/golden/make_plan_bytes_routes.py`` writes
``tests/golden/plan_bytes_routes.json``) and must not move.  Every non-zero value is also checked against the layout

    [header: 16 ints] [batch x 16 floats] [bricks x 16-int descriptors]                       (no multi-pass bricks)
    ... [bricks x 4 pass boxes x 8 ints] [list of multi-pass bricks, padded to 4]              (multi-pass bricks)

so the recorded file cannot pin a typo.  The pointers in the geometry are fakes (non-null, 16-byte aligned): nothing
dereferences them.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import pytest

from torchio_amd import _abi, _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_bytes_routes.json")

PLAN_HEADER_INTS, DESC_INTS, PASS_INTS, PASSES_PER_BRICK = 16, 16, 8, 4  # resample_plan.hpp / resample_tile.hpp

#: every switch that takes part in the route choice: cleared for each case, then the case's own are set
SWITCHES = ("TIO_FAST_KERNEL", "TIO_EXACT_LEAN", "TIO_EXACT_PLAN", "TIO_PLANNED_LEAN", "TIO_LEAN_MULTI", "TIO_RESAMPLE_PATH",
            "TIO_RESAMPLE_EXACT", "TIO_TILE_ABLATE", "TIO_NEAREST_KERNEL")

PRECISIONS = {"exact": _abi.PRECISION_EXACT, "fast": _abi.PRECISION_FAST, "tight": _abi.PRECISION_TIGHT}
FLAGS = {"none": 0, "large": _abi.GEOM_LARGE_BOXES, "mostly_large": _abi.GEOM_MOSTLY_LARGE_BOXES}

#: name -> (batch, shape, control grid or None, spacing, norm_shape)
GEOMETRIES = {
    "b8_256_affine": (8, (256, 256, 256), None, 1.0, 0),
    "b8_256_cp7": (8, (256, 256, 256), (7, 7, 7), 1.0, 0),
    "b8_256_cp20_narrow_cells": (8, (256, 256, 256), (20, 20, 20), 1.0, 0),  # cells narrower than a 16-voxel brick
    "b8_256_cp7_spacing2": (8, (256, 256, 256), (7, 7, 7), 2.0, 0),
    "b8_256_affine_spacing2": (8, (256, 256, 256), None, 2.0, 0),
    "b8_256x256x254_affine": (8, (256, 256, 254), None, 1.0, 0),  # K not divisible by 4: no 16-byte rows
    "b8_256_affine_norm9000": (8, (256, 256, 256), None, 1.0, 9000),  # divisor above 8192: the long division
    "b2_64_affine": (2, (64, 64, 64), None, 1.0, 0),  # 128 bricks: far below the planned-brick threshold
    "b2_64_cp7": (2, (64, 64, 64), (7, 7, 7), 1.0, 0),
    "b3_256_affine": (3, (256, 256, 256), None, 1.0, 0),  # 12 288 bricks: exactly the threshold
    "b3_256x256x240_affine": (3, (256, 256, 240), None, 1.0, 0),  # 11 520 bricks: just below it
}

#: the switches at their non-default values
SWITCH_SETTINGS = (
    {"TIO_FAST_KERNEL": "brick"}, {"TIO_FAST_KERNEL": "planned"},
    {"TIO_EXACT_LEAN": "0"}, {"TIO_EXACT_LEAN": "2"},
    {"TIO_EXACT_PLAN": "0"}, {"TIO_EXACT_PLAN": "2"},
    {"TIO_EXACT_LEAN": "0", "TIO_EXACT_PLAN": "0"}, {"TIO_EXACT_LEAN": "0", "TIO_EXACT_PLAN": "2"},
    {"TIO_PLANNED_LEAN": "0"}, {"TIO_LEAN_MULTI": "0"},
    {"TIO_RESAMPLE_PATH": "gather"}, {"TIO_RESAMPLE_PATH": "tile"},
)
SWITCH_GEOMETRIES = ("b8_256_affine", "b8_256_cp7", "b2_64_affine", "b8_256x256x254_affine")
SWITCH_FLAGS = ("none", "large")


def _cases():
    table = {}
    for g in GEOMETRIES:
        for p in PRECISIONS:
            for f in FLAGS:
                table[f"{g}-{p}-{f}"] = (g, p, f, {})
    for env in SWITCH_SETTINGS:
        tag = ",".join(f"{k[4:]}={v}" for k, v in env.items())
        for g in SWITCH_GEOMETRIES:
            for p in PRECISIONS:
                for f in SWITCH_FLAGS:
                    table[f"{g}-{p}-{f}-{tag}"] = (g, p, f, env)
    return table


CASES = _cases()


def make_geom(geometry: str, precision: str, flags: str) -> _abi.ResampleGeom:
    batch, shape, cp_shape, spacing, norm = GEOMETRIES[geometry]
    geom = _abi.ResampleGeom()
    geom.batch = batch
    geom.in_shape[:] = shape
    geom.out_shape[:] = shape
    geom.affine_first = 1
    geom.mapping_dev = 0x10000  # fake, 16-byte aligned, never read
    geom.mapping_batched = 1
    if cp_shape is not None:
        geom.control_points_dev = 0x20000
        geom.cp_batched = 1
        geom.cp_shape[:] = cp_shape
    geom.in_spacing[:] = (spacing,) * 3
    geom.out_spacing[:] = (spacing,) * 3
    geom.norm_shape[:] = (norm,) * 3
    geom.precision = PRECISIONS[precision]
    geom.flags = FLAGS[flags]
    return geom


def plan_bytes(case_id: str) -> int:
    """The real ``tio_resample3d_plan_bytes`` for one case, under that case's switches (the environment is restored)."""
    geometry, precision, flags, env = CASES[case_id]
    _, fn = _lib.load()
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}
    try:
        os.environ.update(env)
        fn["reload_env"]()
        return int(fn["resample3d_plan_bytes"](C.byref(make_geom(geometry, precision, flags))))
    finally:
        for name, value in saved.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value
        fn["reload_env"]()


def layout_bytes(case_id: str, multi: bool) -> int:
    batch, shape, _, _, _ = GEOMETRIES[CASES[case_id][0]]
    bricks = batch * ((shape[0] + 15) // 16) * ((shape[1] + 15) // 16) * ((shape[2] + 15) // 16)
    ints = PLAN_HEADER_INTS + batch * 16 + bricks * DESC_INTS
    if multi:
        ints += bricks * PASS_INTS * PASSES_PER_BRICK + ((bricks + 3) & ~3)
    return ints * 4


def _recorded() -> dict:
    with open(GOLDEN, encoding="utf-8") as handle:
        return json.load(handle)


def test_recorded_table_matches_and_discriminates():
    recorded = _recorded()
    assert set(recorded) == set(CASES)
    zero = sum(1 for v in recorded.values() if v == 0)
    assert 3 * zero >= len(recorded), f"only {zero} of {len(recorded)} cases without a plan"
    assert 3 * (len(recorded) - zero) >= len(recorded), f"only {len(recorded) - zero} of {len(recorded)} cases with a plan"
    assert recorded["b8_256_affine-exact-none"] == (16 + 8 * 16 + 32768 * 16) * 4 == 2097728


@pytest.mark.parametrize("case_id", sorted(CASES))
def test_plan_bytes(case_id):
    expected = _recorded()[case_id]
    got = plan_bytes(case_id)
    assert got == expected, f"{case_id}: tio_resample3d_plan_bytes = {got}, recorded {expected}"
    if got == 0:
        return
    _, precision, flags, env = CASES[case_id]
    # multi-pass bricks: only the exact-coordinate road lists them, only on a large-box hint, never under TIO_LEAN_MULTI=0
    may_be_multi = flags != "none" and precision != "fast" and env.get("TIO_LEAN_MULTI") != "0"
    allowed = {layout_bytes(case_id, False)} | ({layout_bytes(case_id, True)} if may_be_multi else set())
    assert got in allowed, f"{case_id}: {got} bytes is not a plan layout of this geometry ({sorted(allowed)})"
