"""GPU: NaN / +inf / -inf voxels and NaN payloads through the data movers and the intensity kernels.

* pure moves (``flip3d``, ``permute3d``, ``pad3d``, ``swap_patches``, ``patch_accumulate`` in crop mode): the expected
  result is computed with torch on the INTEGER view of the same tensor, which cannot alter a bit, and compared on the integer
  view (``torch.equal`` on floats never sees a NaN payload, nor the sign of a zero);
* ``interpolate3d``, ``axis_gather_lerp``, ``bspline_prefilter``, ``patch_accumulate`` (average / hann): against the oracle,
  bit for bit with any NaN matching any NaN, and untouched lines / voxels bit-equal to the clean run;
* the stencil (``separable_conv3d``, ``blur_fused`` with and without its bias and noise stages), ``bias_field_apply`` and
  ``add_noise``: equal NaN / +inf / -inf sets and the existing parity bars on the finite part;
* ``Compose[Affine, ElasticDeformation, BiasField, Blur, Noise]`` end to end in the library's default mode.

The k-space family is out of scope: the reference's FFT spreads a non-finite voxel over the whole volume.
"""
from __future__ import annotations

import copy

import pytest
import torch
import torch.nn.functional as F

import nonfinite_cases as nc
from case_inputs import _data
from case_inputs import _taps
from parity_harness import use_engine

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOATS = [torch.float32, torch.float16, torch.bfloat16, torch.float64]
FLOAT_IDS = ["float32", "float16", "bfloat16", "float64"]


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(nc.bits(a), nc.bits(b))


def _on_bits(data: torch.Tensor, fn) -> torch.Tensor:
    """*fn* applied to the integer view of *data*, viewed back: a move that no arithmetic can touch."""
    return fn(nc.bits(data)).contiguous().view(data.dtype)


def _same_classes(want: torch.Tensor, got: torch.Tensor) -> bool:
    return bool(torch.equal(want.isnan(), got.isnan()) and torch.equal(want == nc.PINF, got == nc.PINF) and torch.equal(want == nc.NINF, got == nc.NINF))


# -- pure moves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_flip3d_moves_bits(hip, dtype):
    data = nc.payload_volume((3, 2, 7, 9, 11), dtype, 101)
    for axes in ([0], [1], [2], [0, 2], [0, 1, 2], []):
        got = hip.flip3d(data.to(DEV), axes).cpu()
        assert _same_bits(got, _on_bits(data, lambda v: torch.flip(v, [2 + a for a in axes]) if axes else v)), axes
    flags = torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=torch.uint8)
    got = hip.flip3d(data.to(DEV), per_element=flags).cpu()
    assert _same_bits(got, _on_bits(data, lambda v: torch.stack([torch.flip(v[0], [1, 3]), v[1], torch.flip(v[2], [2])])))


@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_permute3d_moves_bits(hip, dtype):
    data = nc.payload_volume((2, 2, 9, 33, 18), dtype, 102)  # (more than one 32-wide transpose tile on one axis)
    for perm, flips in (((0, 1, 2), ()), ((2, 1, 0), ()), ((1, 2, 0), (0,)), ((0, 2, 1), (1, 2)), ((2, 0, 1), (0, 1, 2)), ((1, 0, 2), (2,))):
        got = hip.permute3d(data.to(DEV), perm, flips).cpu()
        want = _on_bits(data, lambda v: (torch.flip(v, [2 + a for a in flips]) if flips else v).permute(0, 1, 2 + perm[0], 2 + perm[1], 2 + perm[2]))
        assert _same_bits(got, want), (perm, flips)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_pad3d_moves_bits(hip, dtype, mode):
    data = nc.payload_volume((2, 3, 6, 9, 11), dtype, 103)
    padding = (2, 5, 0, 3, 4, 1)
    got = hip.pad3d(data.to(DEV), padding, mode, fill=0.0).cpu()
    if mode == "constant":
        want = _on_bits(data, lambda v: F.pad(v, (4, 1, 0, 3, 2, 5), value=0))  # (+0.0 is the all-zero pattern)
    else:  # (F.pad has no integer kernels for these modes) it moves the voxels' float64 INDICES, exact, and the bits follow them
        index = torch.arange(data.numel(), dtype=torch.float64).reshape(1, -1, *data.shape[2:])
        moved = F.pad(index, (4, 1, 0, 3, 2, 5), mode=mode).long().reshape(2, 3, 13, 12, 16)
        want = nc.bits(data).reshape(-1)[moved.reshape(-1)].reshape(moved.shape).view(dtype)
    assert _same_bits(got, want)


@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_pad3d_constants_that_are_not_finite(hip, dtype):
    """A NaN constant, and per-element constants NaN / -inf / -0.0: the border holds them, the interior keeps its bits."""
    data = nc.payload_volume((3, 2, 5, 6, 7), dtype, 105)
    padding = (1, 2, 3, 0, 0, 4)
    inner = (slice(None), slice(None), slice(1, 6), slice(3, 9), slice(0, 7))
    got = hip.pad3d(data.to(DEV), padding, "constant", fill=nc.NAN).cpu()
    assert _same_bits(got[inner], data)
    border = torch.ones(got.shape, dtype=torch.bool)
    border[inner] = False
    assert bool(got[border].isnan().all())
    fills = torch.tensor([nc.NAN, nc.NINF, -0.0])
    got = hip.pad3d(data.to(DEV), padding, fill_per_element=fills.to(DEV)).cpu()
    assert _same_bits(got[inner], data)
    assert bool(got[0][border[0]].isnan().all()) and bool((got[1][border[1]] == nc.NINF).all())
    assert _same_bits(got[2][border[2]], torch.full_like(got[2][border[2]], -0.0))


@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_swap_patches_moves_bits(hip, dtype):
    data = nc.payload_volume((2, 2, 12, 14, 17), dtype, 106)
    patch = (4, 5, 6)
    pairs = [((0, 0, 0), (8, 9, 11)), ((2, 3, 1), (3, 4, 2)), ((8, 0, 5), (1, 9, 11))]  # (the second pair overlaps itself)
    got = hip.swap_patches(data.to(DEV), pairs, patch).cpu()

    def swaps(v):
        v = v.clone()
        for a, b in pairs:
            sa = tuple(slice(o, o + p) for o, p in zip(a, patch))
            sb = tuple(slice(o, o + p) for o, p in zip(b, patch))
            first, second = v[(..., *sa)].clone(), v[(..., *sb)].clone()
            v[(..., *sa)] = second
            v[(..., *sb)] = first
        return v

    assert _same_bits(got, _on_bits(data, swaps))


@pytest.mark.parametrize("dtype", FLOATS, ids=FLOAT_IDS)
def test_patch_accumulate_crop_moves_bits(hip, dtype):
    patches = nc.payload_volume((3, 2, 8, 8, 8), dtype, 107)
    placements = [((0, 0, 0), (0, 0, 0), (8, 8, 8)), ((6, 5, 4), (2, 1, 0), (6, 7, 8)), ((10, 8, 8), (0, 0, 3), (6, 8, 5))]
    out = nc.payload_volume((2, 16, 16, 16), dtype, 108)
    want_bits = nc.bits(out).clone()
    for n, (dst, src, extent) in enumerate(placements):
        d = tuple(slice(o, o + e) for o, e in zip(dst, extent))
        s = tuple(slice(o, o + e) for o, e in zip(src, extent))
        want_bits[(slice(None), *d)] = nc.bits(patches)[(n, slice(None), *s)]
    device_out = out.to(DEV)
    hip.patch_accumulate(device_out, None, patches.to(DEV), placements, "crop")
    assert torch.equal(nc.bits(device_out.cpu()), want_bits)


# -- interpolation ----------------------------------------------------------------------------------------------------
def _poisoned_small(dtype=torch.float32):
    clean = _data((2, 2, 13, 9, 20), dtype, 91)
    data = clean.clone()
    data[0, 1, 0, 0, 0] = nc.NAN
    data[0, 1, 6, 4, 19] = nc.PINF
    data[0, 1, 12, 8, 7] = nc.NINF
    data[0, 1, 6, 5, 0] = nc.NINF
    return data, clean


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64], ids=["float32", "float16", "float64"])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_interpolate3d(oracle, hip, mode, dtype):
    data, clean = _poisoned_small(dtype)
    for out_shape in [(20, 9, 7), (5, 18, 33), (13, 9, 20), (25, 17, 39)]:
        want = oracle.interpolate3d(data, out_shape, mode)
        got = hip.interpolate3d(data.to(DEV), out_shape, mode)
        assert not bool(torch.isfinite(want).all()) and bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[0, 0]).all())
        assert nc.same_bits_or_both_nan(want, got.cpu()), out_shape
        if dtype != torch.float32:
            continue
        # stock ATen on the device as a second witness.  Its kernel is not the host's: it copies when the shapes are equal (no
        # `inf * 0` at a clamped border tap) and rounds the source coordinate differently, so where a planted voxel is a tap of
        # weight zero - or within coordinate rounding (1e-6) of zero - the two ATen builds disagree with each other (measured on
        # the MI355X: 13 x 9 x 20 -> 20 x 9 x 7 and -> 13 x 9 x 20; the oracle and the kernel follow the host's).  What both
        # agree on is asserted: an output that a planted voxel reaches with a weight above 1e-3 on the device (its answer moves
        # by more than 1e27 when the voxel holds the sentinel 1e30) is non-finite; an output that is finite in both ATen builds
        # is finite and inside the existing bar.
        def aten(volume):
            if mode == "linear":
                return F.interpolate(volume.to(DEV), size=out_shape, mode="trilinear", align_corners=True)
            return F.interpolate(volume.to(DEV), size=out_shape, mode="nearest")

        device = aten(data)
        strong = (aten(nc.with_sentinel(data)) - aten(clean)).abs() >= 1e-3 * nc.SENTINEL
        assert int(strong.sum()) >= 1 and not bool(torch.isfinite(device)[strong].any())
        assert not bool(torch.isfinite(got)[strong].any())
        far = torch.isfinite(device) & torch.isfinite(want.to(DEV))
        assert bool(torch.isfinite(got)[far].all())
        torch.testing.assert_close(got[far], device[far], rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("blend", [False, True])
def test_axis_gather_lerp(oracle, hip, dtype, axis, blend):
    clean = _data((3, 2, 10, 12, 14), dtype, 92)
    data = clean.clone()
    data[0, 0, 3, 4, 5], data[0, 0, 9, 11, 13], data[2, 1, 0, 0, 0], data[1, 0, 5, 5, 5] = nc.NAN, nc.PINF, nc.NINF, nc.NAN
    length = data.shape[2 + axis]
    g = torch.Generator().manual_seed(93)
    lower = torch.randint(0, length, (3, length), generator=g, dtype=torch.int32)
    upper = torch.randint(0, length, (3, length), generator=g, dtype=torch.int32) if blend else None
    weight = torch.rand(3, length, generator=g) if blend else None
    if blend:  # weights of exactly 0 and 1: the other tap is still multiplied in the reference's lerp
        weight[:, ::3], weight[:, 1::3] = 0.0, 1.0
    active = torch.tensor([1, 0, 1], dtype=torch.uint8)
    want = oracle.axis_gather_lerp(data, axis, lower, upper, weight, active)
    got = hip.axis_gather_lerp(data.to(DEV), axis, lower, upper, weight, active).cpu()
    assert not bool(torch.isfinite(want[0]).all())
    assert nc.same_bits_or_both_nan(want, got)
    assert _same_bits(got[1], data[1])  # the inactive element keeps its NaN


@pytest.mark.parametrize("order", [2, 3, 4, 5, 6, 7])
def test_bspline_prefilter(oracle, hip, order):
    data, clean = _poisoned_small()
    want, got = oracle.bspline_prefilter(data, order), hip.bspline_prefilter(data.to(DEV), order).cpu()
    got_clean = hip.bspline_prefilter(clean.to(DEV), order).cpu()
    assert nc.same_bits_or_both_nan(want, got)
    for b, c in ((0, 0), (1, 0), (1, 1)):  # (the recursion along three axes carries a planted voxel to its whole channel)
        assert _same_bits(got[b, c], got_clean[b, c])
    for axis in range(3):  # one axis at a time: every (element, channel) is one line
        shape = [2, 2, 1, 1, 1]
        shape[2 + axis] = 23
        line_clean = _data(tuple(shape), torch.float32, 95)
        for value in (nc.NAN, nc.PINF):
            line = line_clean.clone()
            line.reshape(4, 23)[2, 11] = value
            want, got = oracle.bspline_prefilter(line, order), hip.bspline_prefilter(line.to(DEV), order).cpu()
            got_clean = hip.bspline_prefilter(line_clean.to(DEV), order).cpu()
            assert nc.same_bits_or_both_nan(want, got)
            assert _same_bits(got.reshape(4, 23)[[0, 1, 3]], got_clean.reshape(4, 23)[[0, 1, 3]])


# -- the aggregator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("mode", ["average", "hann"])
def test_patch_accumulate_with_one_poisoned_patch(oracle, hip, mode, dtype):
    """Overlapping 8^3 patches in a 16 x 16 x 12 volume, patch 2 holds a NaN, a +inf and a -inf: the accumulators are the
    oracle's; outside that patch's footprint they are the clean run's bits."""
    g = torch.Generator().manual_seed(109)
    clean = (torch.rand(5, 2, 8, 8, 8, generator=g) * 2 - 0.5).to(dtype)
    patches = clean.clone()
    patches[2, 0, 0, 0, 0], patches[2, 0, 7, 7, 7], patches[2, 1, 3, 4, 5] = nc.NAN, nc.PINF, nc.NINF
    origins = [(0, 0, 0), (8, 8, 4), (4, 4, 2), (8, 0, 0), (0, 8, 4)]
    placements = [(o, (0, 0, 0), (8, 8, 8)) for o in origins]
    windows = [torch.hann_window(10, periodic=False)[1:-1].float() for _ in range(3)] if mode == "hann" else None

    def run(engine, batch, device):
        out = torch.zeros(2, 16, 16, 12, dtype=dtype, device=device)
        weight = torch.zeros_like(out)
        engine.patch_accumulate(out, weight, batch.to(device), placements, mode, None if windows is None else [w.to(device) for w in windows])
        return out.cpu(), weight.cpu()

    want, want_weight = run(oracle, patches, "cpu")
    got, got_weight = run(hip, patches, DEV)
    got_clean, _ = run(hip, clean, DEV)
    assert all(nc.classes(want).values())
    assert nc.same_bits_or_both_nan(want, got) and _same_bits(want_weight, got_weight)
    outside = torch.ones(got.shape, dtype=torch.bool)
    outside[:, 4:12, 4:12, 2:10] = False
    assert bool(torch.isfinite(got[outside]).all()) and torch.equal(nc.bits(got)[outside], nc.bits(got_clean)[outside])


# -- the stencil --------------------------------------------------------------------------------------------------------
STENCIL_SHAPE = (2, 1, 21, 37, 128)
#: sigmas -> radii (4, rj, rk): inside the fused J + K pass (<= 8 both), on its limit, beyond it on J, on K (LDS loop), and
#: beyond 16 on K (the generic kernels)
STENCIL_SIGMAS = {"fused": (1.2, 1.5, 2.0), "limit": (1.2, 2.6, 2.6), "j9": (1.2, 3.0, 1.0), "k11": (1.2, 1.0, 3.5), "k18": (1.2, 0.5, 6.0)}


def _stencil_volume():
    """One +inf and one NaN voxel on either side of the seams at J = 16 and K = 64 (far enough apart on I that the largest
    radius keeps some outputs that see only one of them), and a -inf voxel in a corner of element 1."""
    clean = _data(STENCIL_SHAPE, torch.float32, 110)
    data = clean.clone()
    data[0, 0, 4, 15, 63], data[0, 0, 16, 16, 64], data[1, 0, 20, 36, 127] = nc.PINF, nc.NAN, nc.NINF
    return data, clean


@pytest.mark.parametrize("name", list(STENCIL_SIGMAS))
def test_separable_conv3d_and_blur_fused(oracle, hip, name):
    import torchio_amd as tio

    data, _ = _stencil_volume()
    taps, radius = _taps(1, [STENCIL_SIGMAS[name]], 48)
    want = oracle.separable_conv3d(data, taps, radius)
    assert all(nc.classes(want).values()) and int(torch.isfinite(want).sum()) > want.numel() // 2
    got = hip.separable_conv3d(data.to(DEV), taps.to(DEV), radius).cpu()
    assert nc.same_bits_or_both_nan(want, got)
    previous = tio.get_stencil_precision()
    try:
        tio.set_stencil_precision("exact")
        exact = hip.blur_fused(data.to(DEV), taps.to(DEV), radius)
        tio.set_stencil_precision("fast")
        fast = hip.blur_fused(data.to(DEV), taps.to(DEV), radius)
    finally:
        tio.set_stencil_precision(previous)
    if name in ("fused", "limit"):
        assert exact is not None and fast is not None
    if exact is not None:
        assert nc.same_bits_or_both_nan(want, exact.cpu())
    if fast is not None:
        fast, finite = fast.cpu(), torch.isfinite(want)
        assert _same_classes(want, fast)
        assert float((want[finite] - fast[finite]).abs().max()) <= 2e-6 * float(want[finite].abs().max())


@pytest.mark.parametrize("noise", ["none", "philox", "draws"])
@pytest.mark.parametrize("bias", [False, True])
def test_blur_fused_with_its_stages(oracle, hip, bias, noise):
    """The oracle's unfused sequence (bias field from the device: its exp is another library's) on the same volume."""
    import torchio_amd as tio

    data, _ = _stencil_volume()
    taps, radius = _taps(1, [STENCIL_SIGMAS["fused"]], 48)
    g = torch.Generator().manual_seed(111)
    coarse = (torch.rand((2, 1, 7, 3, 2), generator=g) - 0.5) * 0.6
    draws = torch.randn(STENCIL_SHAPE, generator=g)
    mean, std, seed = torch.tensor([-3.0, 3.0]), torch.tensor([0.5, 20.0]), 4321
    x = data.to(DEV)
    source = hip.bias_field_apply(x, coarse.to(DEV)).cpu() if bias else data
    want = oracle.separable_conv3d(source, taps, radius)
    if noise == "philox":
        want = oracle.add_noise(want, mean, std, base1=hip.philox_normal(STENCIL_SHAPE, seed, 0, DEV).cpu())
    elif noise == "draws":
        want = oracle.add_noise(want, mean, std, base1=draws)
    how = {"none": None, "philox": (mean, std, seed), "draws": (mean, std, draws.to(DEV))}[noise]
    assert all(nc.classes(want).values())
    previous = tio.get_stencil_precision()
    try:
        tio.set_stencil_precision("exact")
        exact = hip.blur_fused(x, taps.to(DEV), radius, bias_coarse=coarse.to(DEV) if bias else None, noise=how)
        tio.set_stencil_precision("fast")
        fast = hip.blur_fused(x, taps.to(DEV), radius, bias_coarse=coarse.to(DEV) if bias else None, noise=how)
    finally:
        tio.set_stencil_precision(previous)
    assert exact is not None and fast is not None
    assert nc.same_bits_or_both_nan(want, exact.cpu())
    fast, finite = fast.cpu(), torch.isfinite(want)
    assert _same_classes(want, fast)
    assert float((want[finite] - fast[finite]).abs().max()) <= 2e-6 * float(want[finite].abs().max())


# -- bias field and noise -------------------------------------------------------------------------------------------------
def _poisoned_intensity(dtype):
    clean = _data((3, 2, 18, 21, 68), dtype, 18)
    data = clean.clone()
    data[0, 0, 0, 0, 0], data[0, 1, 17, 20, 67], data[1, 0, 9, 10, 33], data[2, 1, 4, 4, 4] = nc.NAN, nc.PINF, nc.NINF, nc.PINF
    return data


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16], ids=["float32", "float64", "float16"])
@pytest.mark.parametrize("divide", [False, True])
def test_bias_field_apply(oracle, hip, dtype, divide):
    data = _poisoned_intensity(dtype)
    g = torch.Generator().manual_seed(19)
    coarse = 0.5 * torch.randn(3, 2, 4, 5, 6, generator=g)
    skip = torch.tensor([0, 0, 1], dtype=torch.uint8)
    want = oracle.bias_field_apply(data, coarse, divide=divide, skip=skip)
    got = hip.bias_field_apply(data.to(DEV), coarse.to(DEV), divide=divide, skip=skip.to(DEV)).cpu()
    assert all(nc.classes(want).values()) and _same_classes(want, got)
    finite = torch.isfinite(want)
    rtol = {torch.float32: 2e-6, torch.float64: 2e-6, torch.float16: 2e-3}[dtype]
    torch.testing.assert_close(got[finite], want[finite], rtol=rtol, atol=0)
    assert _same_bits(got[2], data[2])  # the skipped element is a copy


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("rician", [False, True])
def test_add_noise_with_explicit_draws(oracle, hip, rician, dtype):
    data = _poisoned_intensity(dtype)
    g = torch.Generator().manual_seed(21)
    base1, base2 = torch.randn(data.shape, generator=g), torch.randn(data.shape, generator=g)
    mean, std = torch.tensor([0.1, 0.0, -0.2]), torch.tensor([0.25, 0.0, 0.5])
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8)
    want = oracle.add_noise(data, mean, std, rician=rician, base1=base1, base2=base2, keep=keep)
    got = hip.add_noise(data.to(DEV), mean, std, rician=rician, base1=base1.to(DEV), base2=base2.to(DEV), keep=keep.to(DEV)).cpu()
    assert int((~torch.isfinite(want)).sum()) == 4 and _same_classes(want, got)  # (Rician: sqrt(inf^2 + n^2) = +inf for -inf too)
    finite = torch.isfinite(want)
    if rician:
        torch.testing.assert_close(got[finite], want[finite], rtol=1e-6, atol=1e-7)
    else:
        assert torch.equal(got[finite], want[finite])
    assert _same_bits(got[1], data[1])


# -- end to end -----------------------------------------------------------------------------------------------------------
def test_compose_end_to_end(oracle, hip):
    """Compose[Affine, ElasticDeformation, BiasField, Blur, Noise] in the library's default mode, 2 x 32^3, one NaN and one +inf
    voxel, against the same seed through the oracle: equal non-finite sets, the finite part inside the golden fixtures' bar for
    this pipeline (2e-6 of max(|ref|, 1)).  Element 0 holds the NaN, so ``default_pad_value="minimum"`` fills with NaN in both."""
    import torchio_amd as tio
    from parity_harness import benchmark_compose

    g = torch.Generator().manual_seed(7)
    subjects = [tio.Subject(t1=tio.ScalarImage(torch.rand(1, 32, 32, 32, generator=g))) for _ in range(2)]
    subjects[0].t1.data[0, 10, 11, 12] = nc.NAN
    subjects[1].t1.data[0, 20, 9, 16] = nc.PINF
    transform = benchmark_compose()
    torch.manual_seed(8)
    with use_engine(oracle):
        want = transform(tio.SubjectsBatch.from_subjects(copy.deepcopy(subjects))).t1.data
    torch.manual_seed(8)
    got = transform(tio.SubjectsBatch.from_subjects(copy.deepcopy(subjects)).to(DEV)).t1.data.cpu()
    assert 0 < int(torch.isfinite(want).sum()) < want.numel()
    assert _same_classes(want, got)
    finite = torch.isfinite(want)
    rel = (want[finite].double() - got[finite].double()).abs() / want[finite].double().abs().clamp_min(1.0)
    assert float(rel.max()) <= 2e-6, float(rel.max())
