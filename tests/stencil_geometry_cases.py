"""Launch geometries of the separable stencil: the cases of ``tests/test_stencil_passes.py`` (CPU) and
``tests/test_gpu_stencil_geometry.py`` (GPU), their inputs, their float64 reference and its error bound.

The dispatcher (``plan_conv`` in ``torchio_amd/csrc/stencil.hip``) picks the kernel family and the number of marching segments
per line from COUNTS: for the register-window marching kernel

    strips = ceil(K / 256) * other * B * C,  want = clamp(ceil(8192 / strips), 1, max(1, n / 32)),
    len = ceil(n / want),  segments = ceil(n / len),

for the LDS-ring kernel 4 / 2 / 1 segments at ``lines < 2048``, ``< 4096``, ``>= 4096`` (a candidate length rounded up to 16 rows
decides the count; the kernel then cuts the line into ``ceil(n / segments)`` rows).  ``strips`` is a product, so a THIN volume
(K = 8, J = 16) with many batch elements and channels gets the segmentation of a 256^3 batch at a hundredth of the voxels.

Every case is LABELLED by hand with what it is there for (family, segments x rows, K tiles, stages per pass); the CPU test
asserts the labels through ``tio_separable_conv3d_passes``, and that every workload geometry has a thin case with the same
launch — move a threshold and these tests say which geometry lost its cover.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from fractions import Fraction

import torch

from torchio_amd import _abi

FAMILY_NAMES = {_abi.CONV_LINE: "line", _abi.CONV_K: "k", _abi.CONV_K_V4: "k_v4", _abi.CONV_MARCH: "march", _abi.CONV_RING: "ring"}
TAP_STRIDE = 40  # >= 2 * 16 + 1


@dataclass(frozen=True)
class Pass:
    """The label of one launch.  ``segments`` / ``rows``: pieces per line along the axis and output rows per piece (but the
    last piece); ``radius_class``: compile-time radius of the marching instantiation (0: the family has none); ``radius_k``:
    radius of the fused K stage (0: none)."""

    axis: int
    family: str
    segments: int = 0
    rows: int = 0
    k_tiles: int = 1
    radius_class: int = 0
    radius_k: int = 0

    def key(self):
        return (self.axis, self.family, self.segments, self.rows, self.k_tiles, self.radius_class, self.radius_k)


@dataclass(frozen=True)
class Case:
    shape: tuple  # (B, C, I, J, K)
    radius: tuple  # (rI, rJ, rK)
    passes: tuple  # labels of tio_separable_conv3d's launches
    seam_axis: int  # the axis whose segmentation the case is about (0 = I, 1 = J)
    per_element_taps: bool = False
    skip_row: int | None = None  # a batch row copied through (neither first nor last)
    env: dict = field(default_factory=dict)
    dtype: torch.dtype = torch.float32
    #: label of the I pass when a bias field rides along (None: the plain label, with the bias stage)
    bias_i_pass: Pass | None = None
    fused_form: bool = True  # tio_blur_fused exists for this case


def _ij(shape, radius, swap):
    """The case in its I orientation, or with I and J swapped (shape and radii alike)."""
    if not swap:
        return shape, radius
    b, c, i, j, k = shape
    return (b, c, j, i, k), (radius[1], radius[0], radius[2])


def _thin(shape, long_radius, short_radius, rk, swap, long_label, *, short_rows, bias_i_pass=None, **kw):
    """A thin fused case: the long axis (I, or J when *swap*) carries ``long_label = (family, segments, rows)``, the short one is
    marched in one piece, the K stage rides on the J pass."""
    shape5, radius = _ij(shape, (long_radius, short_radius, rk), swap)
    family, segments, rows = long_label
    long_pass = dict(family=family, segments=segments, rows=rows, radius_class=long_radius if family == "march" else 0)
    short_pass = dict(family="march", segments=1, rows=short_rows, radius_class=short_radius)
    first, second = (short_pass, long_pass) if swap else (long_pass, short_pass)
    return Case(shape5, radius, (Pass(0, **first), Pass(1, radius_k=rk, **second)), seam_axis=1 if swap else 0,
                bias_i_pass=bias_i_pass, **kw)


def _sweep() -> dict:
    t = {}
    # -- the marching kernel: every segmentation the workloads get, both orientations --------------------------------------
    s = (64, 2, 256, 16, 8)  # 4 x 64: 8 x 256^3, the benchmark
    t["march_4x64_r4_I"] = _thin(s, 4, 2, 1, False, ("march", 4, 64), short_rows=16, per_element_taps=True, skip_row=17)
    t["march_4x64_r8_J"] = _thin(s, 8, 2, 3, True, ("march", 4, 64), short_rows=16)
    # 2 x 128 (16 x 256^3) and 1 x 256, the long single march (>= 32 x 256^3).  At K = 8, J = 16 these counts need B * C >= 256,
    # and then the OTHER pass has 256 * B * C > 65 535 lines, which the dispatcher refuses: the thin shapes run with the one
    # axis active, and a shape with fewer, longer lines (B * C = 128, K = 4) runs all three passes at the same segmentation.
    one = lambda shape, r, swap, label: Case(  # noqa: E731
        *_ij(shape, (r, 0, 0), swap), (Pass(1 if swap else 0, label[0], label[1], label[2], 1, r if label[0] == "march" else 0),),
        seam_axis=1 if swap else 0, fused_form=False)
    s = (64, 4, 256, 16, 8)
    t["march_2x128_r6_I_alone"] = one(s, 6, False, ("march", 2, 128))
    t["march_2x128_r1_J_alone"] = one(s, 1, True, ("march", 2, 128))
    s = (128, 4, 256, 16, 8)
    t["march_1x256_r4_I_alone"] = one(s, 4, False, ("march", 1, 256))
    t["march_1x256_r7_J_alone"] = one(s, 7, True, ("march", 1, 256))
    s = (32, 4, 256, 32, 4)
    t["march_2x128_r6_I"] = _thin(s, 6, 1, 1, False, ("march", 2, 128), short_rows=32)
    t["march_2x128_r1_J"] = _thin(s, 1, 2, 2, True, ("march", 2, 128), short_rows=32)
    s = (32, 4, 256, 64, 4)
    t["march_1x256_r4_I"] = _thin(s, 4, 1, 1, False, ("march", 1, 256), short_rows=64)
    t["march_1x256_r7_J"] = _thin(s, 7, 1, 1, True, ("march", 1, 256), short_rows=64)
    s = (32, 1, 256, 16, 8)  # 8 x 32: 1 or 3 x 256^3 — every radius class of the issue, both orientations
    for r, (rs, rk) in {1: (2, 8), 4: (3, 5), 6: (1, 7), 7: (3, 2), 8: (2, 6)}.items():
        ring_i = Pass(0, "ring", 4, 64) if r >= 7 else None  # with a bias field the I pass leaves the marching kernel at 7
        t[f"march_8x32_r{r}_I"] = _thin(s, r, rs, rk, False, ("march", 8, 32), short_rows=16, bias_i_pass=ring_i,
                                        per_element_taps=r == 7)
        t[f"march_8x32_r{r}_J"] = _thin(s, r, rs, rk, True, ("march", 8, 32), short_rows=16, per_element_taps=r == 6)
    # radius class 5, the one class the shapes above leave out: its plain and its bias-on-load instantiation, exact and fused
    # multiply-add, at the small shape of test_gpu_stencil_fused_codegen (37 is prime and above two windows: one march of 37 rows)
    t["march_1x37_r5_I"] = _thin((2, 1, 37, 37, 8), 5, 2, 3, False, ("march", 1, 37), short_rows=37, per_element_taps=True)
    s = (64, 2, 250, 16, 8)  # 4 x 63, last segment 61
    t["march_4x63_ragged_r6_I"] = _thin(s, 6, 2, 1, False, ("march", 4, 63), short_rows=16)
    t["march_4x63_ragged_r4_J"] = _thin(s, 4, 1, 4, True, ("march", 4, 63), short_rows=16)
    s = (8, 1, 97, 16, 8)  # 3 x 33, last segment 31: want clamped by n / 32
    t["march_3x33_ragged_r8_I"] = _thin(s, 8, 1, 1, False, ("march", 3, 33), short_rows=16, per_element_taps=True, skip_row=3,
                                        bias_i_pass=Pass(0, "ring", 4, 25))
    t["march_3x33_ragged_r6_J"] = _thin(s, 6, 1, 5, True, ("march", 3, 33), short_rows=16, skip_row=5)
    s = (8, 1, 65, 8, 8)  # 2 x 33, last segment 32
    t["march_2x33_r7_I"] = _thin(s, 7, 2, 2, False, ("march", 2, 33), short_rows=8, bias_i_pass=Pass(0, "ring", 3, 22))
    t["march_2x33_r1_J"] = _thin(s, 1, 2, 6, True, ("march", 2, 33), short_rows=8)
    # two K tiles (K = 260 > 256): the K pass stays a launch of its own, the J pass carries nothing
    t["march_4x32_two_k_tiles_r4_I"] = Case(
        (1, 1, 128, 4, 260), (4, 1, 2),
        (Pass(0, "march", 4, 32, 2, 4), Pass(1, "march", 1, 4, 2, 1), Pass(2, "k_v4", k_tiles=2)), seam_axis=0, fused_form=False)
    t["march_4x32_two_k_tiles_r6_J"] = Case(
        (1, 1, 4, 128, 260), (1, 6, 8),
        (Pass(0, "march", 1, 4, 2, 1), Pass(1, "march", 4, 32, 2, 6), Pass(2, "k_v4", k_tiles=2)), seam_axis=1, fused_form=False)
    # J and K marched separately (TIO_CONV_NO_FUSE)
    t["march_8x32_no_fuse_r4_J"] = Case(
        (32, 1, 16, 256, 8), (2, 4, 3),
        (Pass(0, "march", 1, 16, 1, 2), Pass(1, "march", 8, 32, 1, 4), Pass(2, "k_v4")), seam_axis=1,
        env={"TIO_CONV_NO_FUSE": "1"}, fused_form=False)
    # -- the LDS-ring kernel (radii 9 - 16) ---------------------------------------------------------------------------------
    s = (64, 2, 256, 16, 8)  # 2 x 128: 8 x 256^3
    t["ring_2x128_r9_I"] = _thin(s, 9, 1, 1, False, ("ring", 2, 128), short_rows=16, per_element_taps=True, skip_row=40)
    t["ring_2x128_r12_J"] = _thin(s, 12, 1, 1, True, ("ring", 2, 128), short_rows=16)
    # 1 x 256 (16 x 256^3 and beyond): one axis on the thin shapes, three passes on the shapes with fewer, longer lines (above)
    t["ring_1x256_r16_I_alone"] = one((64, 4, 256, 16, 8), 16, False, ("ring", 1, 256))
    t["ring_1x256_r9_J_alone"] = one((64, 4, 256, 16, 8), 9, True, ("ring", 1, 256))
    t["ring_1x256_many_lines_r9_I_alone"] = one((128, 4, 256, 16, 8), 9, False, ("ring", 1, 256))
    s = (32, 4, 256, 32, 4)
    t["ring_1x256_r16_I"] = _thin(s, 16, 1, 1, False, ("ring", 1, 256), short_rows=32)
    t["ring_1x256_r9_J"] = _thin(s, 9, 1, 2, True, ("ring", 1, 256), short_rows=32)
    t["ring_1x256_many_lines_r9_I"] = _thin((32, 4, 256, 64, 4), 9, 1, 1, False, ("ring", 1, 256), short_rows=64)
    s = (32, 1, 256, 16, 8)  # 4 x 64: 1 or 3 x 256^3
    t["ring_4x64_r16_I"] = _thin(s, 16, 2, 3, False, ("ring", 4, 64), short_rows=16)
    t["ring_4x64_r12_J"] = _thin(s, 12, 3, 4, True, ("ring", 4, 64), short_rows=16, per_element_taps=True)
    s = (8, 1, 97, 16, 8)  # four segments from a candidate length of 32 rows: the kernel cuts 25, 25, 25, 22
    t["ring_4x25_ragged_r12_I"] = _thin(s, 12, 1, 1, False, ("ring", 4, 25), short_rows=16)
    t["ring_4x25_ragged_r16_J"] = _thin(s, 16, 2, 8, True, ("ring", 4, 25), short_rows=16, skip_row=2)
    s = (8, 1, 12, 16, 8)  # a line shorter than one 16-row step
    t["ring_1x12_short_r9_I"] = _thin(s, 9, 2, 1, False, ("ring", 1, 12), short_rows=16)
    t["ring_1x12_short_r9_J"] = _thin(s, 9, 1, 1, True, ("ring", 1, 12), short_rows=16)
    # -- the generic kernels: K not a multiple of 4 keeps every pass off the 16-byte kernels -----------------------------------
    t["line_8x32_k_odd_r4_I"] = Case(
        (2, 2, 240, 8, 71), (4, 2, 1), (Pass(0, "line", 8, 32, 2), Pass(1, "line", 1, 32, 2), Pass(2, "k")), seam_axis=0,
        fused_form=False)
    return t


SWEEP = _sweep()

#: the workloads: name -> ((B, C, I, J, K), radius, axis looked at, the thin case with the same launch on its seam axis,
#: whether rows per segment must match as well)
WORKLOADS = {
    "1x256^3_march": ((1, 1, 256, 256, 256), (4, 4, 4), 0, "march_8x32_r4_I", True),
    "3x256^3_march": ((3, 1, 256, 256, 256), (4, 4, 4), 0, "march_8x32_r4_I", True),
    "3x256^3_march_J": ((3, 1, 256, 256, 256), (4, 4, 4), 1, "march_8x32_r4_J", True),
    "8x256^3_march": ((8, 1, 256, 256, 256), (4, 4, 4), 0, "march_4x64_r4_I", True),
    "8x256^3_march_J": ((8, 1, 256, 256, 256), (2, 8, 3), 1, "march_4x64_r8_J", True),
    "16x256^3_march": ((16, 1, 256, 256, 256), (6, 6, 6), 0, "march_2x128_r6_I", True),
    "32x256^3_march": ((32, 1, 256, 256, 256), (4, 4, 4), 0, "march_1x256_r4_I", True),
    "64x256^3_march_J": ((64, 1, 256, 256, 256), (7, 7, 7), 1, "march_1x256_r7_J", True),
    "1x256^3_ring": ((1, 1, 256, 256, 256), (16, 16, 8), 0, "ring_4x64_r16_I", True),
    "3x256^3_ring_J": ((3, 1, 256, 256, 256), (12, 12, 4), 1, "ring_4x64_r12_J", True),
    "8x256^3_ring": ((8, 1, 256, 256, 256), (9, 9, 1), 0, "ring_2x128_r9_I", True),
    "16x256^3_ring": ((16, 1, 256, 256, 256), (16, 16, 1), 0, "ring_1x256_r16_I", True),
    "32x256^3_ring": ((32, 1, 256, 256, 256), (9, 9, 1), 0, "ring_1x256_many_lines_r9_I", True),
    # 4 x 128 rows: the thin case has the four segments and the two K tiles, at 32 rows
    "2ch_512^3_march": ((1, 2, 512, 512, 512), (4, 4, 4), 0, "march_4x32_two_k_tiles_r4_I", False),
    # K = 155 is no multiple of 4: this workload never reaches a 16-byte kernel, whatever its line count
    "8x4x240x240x155": ((8, 4, 240, 240, 155), (4, 4, 4), 0, "line_8x32_k_odd_r4_I", True),
}

SWITCHES = ("TIO_CONV_RING", "TIO_CONV_NO_FUSE")


# -- the dispatcher's report ------------------------------------------------------------------------------------------------
def reported_passes(fn, shape, radius, *, dtype=torch.float32, aligned=True, has_skip=False, bias=False, noise=0, fast=False):
    """``tio_separable_conv3d_passes`` as a list of :class:`Pass` plus the stage flags per pass, or the negative status."""
    from torchio_amd.ops import dtype_code

    out = (_abi.ConvPass * 3)()
    shape3 = (C.c_int32 * 3)(*shape[2:])
    radius3 = (C.c_int32 * 3)(*radius)
    n = fn["separable_conv3d_passes"](dtype_code(dtype), shape[0], shape[1], shape3, radius3, int(aligned), int(has_skip), int(bias),
                                      int(noise), int(fast), out)
    if n < 0:
        return n
    passes, stages = [], []
    for p in out[:n]:
        passes.append(Pass(p.axis, FAMILY_NAMES[p.family], p.segments, p.rows_per_segment, p.k_tiles, p.radius_class, p.radius_k))
        stages.append({"pre_bias": p.pre_bias, "post_noise": p.post_noise, "fma": p.fma, "last": p.last, "radius": p.radius,
                       "grid": tuple(p.grid), "lds_bytes": p.lds_bytes})
    return passes, stages


def expected_bias_passes(case: Case) -> tuple:
    """The labels of ``tio_blur_fused`` with a bias field: the I pass may change family (``Case.bias_i_pass``)."""
    if case.bias_i_pass is None:
        return case.passes
    return (case.bias_i_pass,) + tuple(case.passes[1:])


def first_seam(case: Case) -> int:
    """Index of the first row of the second segment along the case's seam axis (the middle of the line when there is one segment)."""
    label = next(p for p in case.passes if p.axis == case.seam_axis)
    n = case.shape[2 + case.seam_axis]
    return label.rows if label.segments > 1 else n // 2


# -- inputs -------------------------------------------------------------------------------------------------------------------
def make_inputs(name: str):
    """``(data, taps, skip)`` on the CPU: signed data (``randn * 100`` plus a ramp along the seam axis), asymmetric random taps
    that sum to one (a reversed or shifted tap order shows, which a Gaussian would hide), a skip flag on one inner batch row."""
    case = SWEEP[name]
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    b, c, *spatial = case.shape
    data = torch.randn(case.shape, generator=g, dtype=torch.float32) * 100.0
    n = spatial[case.seam_axis]
    ramp_shape = [1, 1, 1, 1, 1]
    ramp_shape[2 + case.seam_axis] = n
    data += (torch.arange(n, dtype=torch.float32) * 3.0 - n).reshape(ramp_shape)
    rows = b if case.per_element_taps else 1
    taps = torch.zeros((rows, 3, TAP_STRIDE), dtype=torch.float32)
    for axis, r in enumerate(case.radius):
        w = torch.rand((rows, 2 * r + 1), generator=g, dtype=torch.float64) + 0.05
        taps[:, axis, : 2 * r + 1] = (w / w.sum(dim=1, keepdim=True)).to(torch.float32)
    skip = None
    if case.skip_row is not None:
        assert 0 < case.skip_row < b - 1
        skip = torch.zeros(b, dtype=torch.uint8)
        skip[case.skip_row] = 1
    return data.to(case.dtype), taps, skip


def plant_infs(case: Case, data: torch.Tensor) -> torch.Tensor:
    """One ``inf`` ``radius`` rows before the first seam (the far tap of the seam row — the first row of the second segment —
    reaches it: the halo must hold it) and one ``radius + 1`` rows after it (one row beyond the reach of the row in front of the
    seam: a tap too many, or a window that is one row off, shows).  Different lines, in a batch row that is not skipped."""
    seam, r = first_seam(case), case.radius[case.seam_axis]
    n = case.shape[2 + case.seam_axis]
    out = data.clone()
    b = 0 if case.skip_row != 0 else 1
    for row, (other, k) in ((seam - r, (1, 1)), (seam + r, (2, case.shape[4] - 2))):
        index = [b, case.shape[1] - 1, other, other, k]
        index[2 + case.seam_axis] = min(max(row, 0), n - 1)
        out[tuple(index)] = float("inf")
    return out


# -- the float64 reference and the bound --------------------------------------------------------------------------------------
def _correlate_axis64(x: torch.Tensor, w: torch.Tensor, r: int, dim: int) -> torch.Tensor:
    """Replicate-padded correlation of float64 ``x`` along ``dim`` with the taps ``w`` (rows, 2r + 1), float64, plain sums."""
    n = x.shape[dim]
    index = torch.arange(-r, n + r).clamp_(0, n - 1)
    padded = x.index_select(dim, index)
    acc = torch.zeros_like(x)
    for t in range(2 * r + 1):
        window = padded.narrow(dim, t, n)
        if w.shape[0] == 1:
            acc.add_(window, alpha=float(w[0, t]))
        else:
            acc.addcmul_(window, w[:, t].reshape(-1, 1, 1, 1, 1))
    return acc


def reference64(data: torch.Tensor, taps: torch.Tensor, radius, skip=None, *, absolute: bool = False) -> torch.Tensor:
    """The three replicate-padded correlations in float64 with the float32 tap values; ``absolute``: of ``|data|`` with
    ``|taps|`` — the quantity ``A`` the rounding bound scales with.  Skipped rows are the data themselves."""
    x = data.to(torch.float64)
    w = taps.to(torch.float64)
    if absolute:
        x, w = x.abs(), w.abs()
    out = x
    for axis, r in enumerate(radius):
        if r > 0:
            out = _correlate_axis64(out, w[:, axis], r, 2 + axis)
    if skip is not None:
        rows = skip.bool()
        out[rows] = x[rows]
    return out


def bound_factor(radius) -> float:
    """``(1 + g(W_I + 1)) (1 + g(W_J + 1)) (1 + g(W_K + 1)) - 1`` over the active axes, ``g(k) = k u / (1 - k u)``, ``u = 2^-24``:
    every pass is a sequential float32 sum of ``W = 2R + 1`` rounded products from zero (W roundings of products, W of sums, the
    first sum exact: at most W + 1 roundings on any term), and a pass's input carries the passes' before it.  With fused
    multiply-adds a term sees fewer roundings: the same bound holds.  Exact rational arithmetic, rounded once."""
    u = Fraction(1, 2**24)
    product = Fraction(1)
    for r in radius:
        if r > 0:
            k = 2 * r + 2
            product *= 1 + k * u / (1 - k * u)
    return float(product - 1)


def within_bound(result: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, radius, skip=None):
    """``(ok, worst ratio)`` of ``|result - ref| <= bound_factor * scale`` per voxel (skipped rows must be exact copies)."""
    err = (result.to(torch.float64) - ref).abs()
    limit = scale * bound_factor(radius)
    if skip is not None:
        limit[skip.bool()] = 0.0
    ok = bool((err <= limit).all())
    ratio = float((err / limit.clamp_min(1e-300)).max()) if limit.numel() else 0.0
    return ok, ratio
