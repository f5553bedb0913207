"""GPU: every entry point on a tensor whose offsets pass 2^31 bytes, 2^32 bytes, 2^31 elements and (one-byte types) 2^32
elements (``large_offset_cases.py``: the shapes, the analytic inputs, the crossings, the slicing).

Two legs per case.  (a) the WHOLE result of the one big call, ``torch.equal`` on the device against an expected tensor: for
movers and label operations that is torch indexing applied per batch slice to the analytic input, for float arithmetic the
same entry point on batch slices that stay below every threshold (the rest of the suite pins those to references).  (b)
something that is not this library's HIP code at the crossings: the movers' leg (a) already is; float arithmetic is held to
the float64 references and bars the suite owns, on 4096-element windows round each crossing; the stencil's and the resampler's
crossing volumes go through the CPU oracle.  Reductions run on ONE channel of more than 2^32 (float32: 2^31) voxels, with the
facts that matter planted behind the last threshold, against int64 / float64 torch reductions taken chunk by chunk.  The
comparisons walk the batch slice by slice, so no test holds a second full-size tensor; every case frees its memory at the end.
What is covered and what is not, per entry point: DESIGN.md, section 9.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intensity_pointwise_cases as pointwise
import label_cases
import large_offset_cases as big
import swap_histogram_cases

pytestmark = pytest.mark.gpu

MOVER_DTYPES = [torch.uint8, torch.float32]
MOVER_IDS = ["uint8", "float32"]
GIB = {torch.uint8: 4.11, torch.float32: 4.30}  # the input of shape_for(dtype), GiB


@pytest.fixture(autouse=True)
def _free_device_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"[large] {request.node.name}: peak device memory {torch.cuda.max_memory_allocated() / 1024**3:.1f} GiB")
    big.release()


def _input(dtype, wide=False):
    shape = big.shape_for(dtype, wide)
    found = big.crossings(shape, dtype)
    assert len(found) == (3 if wide and dtype.itemsize > 1 else 2), found  # 2^31 and 2^32 bytes (one-byte types: elements); wide: 2^31 elements too
    return big.distinct(shape, dtype, "cuda")


def _each_slice(out: torch.Tensor, expected_of, step: int, what: str) -> None:
    """Leg (a): ``out[a:b]`` against ``expected_of(a, b)`` for consecutive batch slices, bit for bit, the whole tensor."""
    for begin in range(0, out.shape[0], step):
        end = min(begin + step, out.shape[0])
        expected = expected_of(begin, end)
        part = out[begin:end]
        assert big.same(part, expected), f"{what}, batch elements {begin}:{end}: {big.first_difference(part, expected)}"
        del expected


# ==== movers and label operations ===========================================================================================
@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_flip3d(hip, dtype):
    big.needs_gib(3 * GIB[dtype])
    data = _input(dtype)
    out = hip.flip3d(data, axes=(0, 2))
    _each_slice(out, lambda a, b: torch.flip(data[a:b], [2, 4]), 1, "flip3d axes (0, 2)")
    del out
    flags = torch.tensor([[(b >> axis) & 1 for axis in range(3)] for b in range(1, data.shape[0] + 1)], dtype=torch.uint8)
    out = hip.flip3d(data, per_element=flags.cuda())
    _each_slice(out, lambda a, b: torch.flip(data[a:b], [2 + axis for axis in range(3) if flags[a, axis]]), 1, "flip3d per element")


def _pad_index(extent: int, before: int, after: int, mode: str) -> torch.Tensor:
    """Source index of every output position along one axis, written from F.pad's definition of each mode."""
    q = torch.arange(-before, extent + after)
    if mode == "circular":
        return q % extent
    if mode == "reflect":
        q = q.abs()
        return torch.where(q >= extent, 2 * (extent - 1) - q, q)
    return q.clamp(0, extent - 1)  # replicate; constant: overwritten below


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_pad3d(hip, dtype, mode):
    big.needs_gib(3.2 * GIB[dtype])
    data = _input(dtype)
    padding = (3, 2, 1, 4, 2, 2)  # K stays a multiple of 4: 424 = 8 * 53, and the output's crossings move off the input's
    fills = (torch.arange(data.shape[0]) * 5 + 9).to(dtype)
    out = hip.pad3d(data, padding, mode, fill=7.0) if mode != "constant" else hip.pad3d(data, padding, mode, fill_per_element=fills.cuda())
    assert big.crossings(out.shape, dtype)
    index = [_pad_index(data.shape[2 + d], padding[2 * d], padding[2 * d + 1], mode).cuda() for d in range(3)]

    def expected(a, b):
        e = data[a:b].index_select(2, index[0]).index_select(3, index[1]).index_select(4, index[2])
        if mode == "constant":
            inner = e[:, :, 3:-2, 1:-4, 2:-2].clone()
            e[:] = fills[a].item()
            e[:, :, 3:-2, 1:-4, 2:-2] = inner
        return e

    _each_slice(out, expected, 1, f"pad3d {mode}")


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_interpolate3d_nearest(hip, dtype):
    big.needs_gib(3.2 * GIB[dtype])
    data = _input(dtype)
    out_shape = (407, 397, 424)
    out = hip.interpolate3d(data, out_shape, "nearest")
    assert big.crossings(out.shape, dtype)
    # ATen on one batch element at a time (below 2^31 bytes as float32): exact, the values are integers below 2^24
    _each_slice(out, lambda a, b: F.interpolate(data[a:b].float(), size=out_shape, mode="nearest").to(dtype), 1, "interpolate3d nearest")


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_axis_gather(hip, dtype, axis):
    big.needs_gib(3 * GIB[dtype])
    data = _input(dtype)
    batch, length = data.shape[0], data.shape[2 + axis]
    lower = (torch.arange(length)[None] * 3 + torch.arange(batch)[:, None] * 11) % length  # a different permutation-like table per element
    active = torch.tensor([b % 4 != 1 for b in range(batch)])
    out = hip.axis_gather_lerp(data, axis, lower, active=active.to(torch.uint8))
    table = lower.cuda()
    _each_slice(out, lambda a, b: data[a:b].index_select(2 + axis, table[a]) if active[a] else data[a:b], 1, f"axis_gather_lerp axis {axis}")


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_patch_gather(hip, dtype):
    """The channels of one ``(C, I, J, K)`` volume pass the thresholds; every patch holds all channels, and the corners are
    laid so that each crossing (its i and j) lies inside a patch."""
    big.needs_gib(1.5 * GIB[dtype])
    shape = big.shape_for(dtype)
    data = _input(dtype).reshape(shape[0] * shape[1], *shape[2:])
    patch = (8, 6, shape[4])
    limit = [s - p for s, p in zip(shape[2:], patch)]
    corners = [[min(i, limit[0]), min(j, limit[1]), 0] for _, _, (_, i, j, _) in big.crossings(shape, dtype)] + [[0, 0, 0], limit]
    out = hip.patch_gather(data, torch.tensor(corners, dtype=torch.int32), patch)
    expected = torch.stack([data[:, i : i + patch[0], j : j + patch[1], k : k + patch[2]] for i, j, k in corners])
    assert big.same(out, expected), big.first_difference(out, expected)


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_swap_patches(hip, dtype):
    big.needs_gib(3 * GIB[dtype])
    data = _input(dtype)
    patch = (40, 30, 100)
    locations = [swap_histogram_cases.random_locations(data.shape[2:], patch, 3, 70 + b) for b in range(data.shape[0])]
    out = hip.swap_patches(data, locations, patch)
    _each_slice(out, lambda a, b: swap_histogram_cases.swap_sequential(data[a:b], locations[a:b], patch), 1, "swap_patches")


@pytest.mark.parametrize("mode, dtype", [("crop", torch.uint8), ("crop", torch.float32), ("average", torch.float32), ("hann", torch.float32)],
                         ids=["crop-uint8", "crop-float32", "average-float32", "hann-float32"])
def test_patch_accumulate(hip, mode, dtype):
    """Patches of all channels written at the rows that hold a crossing: the accumulator's channel offsets pass the thresholds.
    The expected accumulator is the same sum in torch, patch after patch (one addition per voxel and patch: the same bits)."""
    big.needs_gib(2.5 * GIB[dtype])
    shape = big.shape_for(dtype)
    channels = shape[0] * shape[1]
    volume = shape[2:]
    patch = (8, 6, volume[2])
    spots = [(min(i, volume[0] - 8), min(j, volume[1] - 6), 0) for _, _, (_, i, j, _) in big.crossings(shape, dtype)] + [(volume[0] - 8, volume[1] - 6, 0)]
    spots.append((spots[0][0] + 3 if spots[0][0] + 11 <= volume[0] else spots[0][0] - 3, spots[0][1], 0))  # overlaps the first
    patches = big.distinct((len(spots), channels, *patch), dtype, "cuda")
    placements = [(spot, (0, 0, 0), patch) for spot in spots]
    out = torch.zeros((channels, *volume), dtype=dtype, device="cuda")
    expected = torch.zeros_like(out)
    weights = torch.zeros_like(out) if mode != "crop" else None
    expected_weights = torch.zeros_like(out) if mode != "crop" else None
    hann = [torch.hann_window(p + 2, periodic=False)[1:-1].cuda() for p in patch] if mode == "hann" else None
    hip.patch_accumulate(out, weights, patches, placements, mode, windows=hann)
    for n, (i, j, k) in enumerate(spots):
        where = (slice(None), slice(i, i + patch[0]), slice(j, j + patch[1]), slice(k, k + patch[2]))
        if mode == "crop":
            expected[where] = patches[n]
        elif mode == "average":
            expected[where] += patches[n]
            expected_weights[where] += 1
        else:
            window = hann[0][:, None, None] * hann[1][None, :, None] * hann[2][None, None, :]
            expected[where] += patches[n] * window
            expected_weights[where] += window
    assert big.same(out, expected), big.first_difference(out, expected)
    if weights is not None:
        assert big.same(weights, expected_weights), big.first_difference(weights, expected_weights)


@pytest.mark.parametrize("disk_type, dtype", [(2, torch.uint8), (16, torch.float32)], ids=MOVER_IDS)
def test_nifti_decode(hip, disk_type, dtype):
    """Fortran-ordered payloads back to back: the decoded ``(B, C, I, J, K)`` tensor is the transposed view, bit for bit."""
    big.needs_gib(3 * GIB[dtype])
    shape = big.shape_for(dtype)
    on_disk = big.distinct((*shape[:2], *shape[:1:-1]), dtype, "cuda")  # (B, C, K, J, I): each file's array in C order of (k, j, i)
    out = hip.nifti_decode(on_disk.reshape(-1).view(torch.uint8), disk_type=disk_type, shape=shape[2:], channels=shape[1], batch=shape[0])
    assert out.shape == shape and out.dtype == dtype and big.crossings(shape, dtype)
    _each_slice(out, lambda a, b: on_disk[a:b].permute(0, 1, 4, 3, 2).contiguous(), 1, "nifti_decode")


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_label_remap(hip, dtype, inplace):
    big.needs_gib(3 * GIB[dtype])
    data = _input(dtype)
    mapping = {3: 200, 200: 3, 17: 0, 131: 132, 44: 45, (250 if dtype == torch.uint8 else 960): 1}  # (every key is a value of the dtype)
    default = None if inplace else 9.0
    source = data.clone() if inplace else data
    out = hip.label_remap(source, mapping, default=default, inplace=inplace)
    assert (out.data_ptr() == source.data_ptr()) == inplace
    _each_slice(out, lambda a, b: label_cases.remap(data[a:b], mapping, default), 1, "label_remap")


@pytest.mark.parametrize("dtype, batch, classes", [(torch.uint8, 9, 8), (torch.float32, 17, 4)], ids=MOVER_IDS)
def test_label_one_hot(hip, dtype, batch, classes):
    """9 uint8 label maps of 2^26 voxels to 8 classes: 4.9e9 float32, 18 GiB — the OUTPUT passes 2^32 elements.  17 float32 label
    maps (the INPUT passes 2^32 bytes) to 4 classes: 4.6e9 float32."""
    big.needs_gib(26)
    shape = (batch, 1, *big.VOLUME)
    data = big.distinct(shape, dtype, "cuda") % classes
    assert len(big.crossings(shape, dtype)) == (0 if dtype == torch.uint8 else 2)
    out = hip.label_one_hot(data, classes)
    assert len(big.crossings(out.shape, out.dtype)) == 4
    _each_slice(out, lambda a, b: label_cases.one_hot(data[a:b], classes), 1, "label_one_hot")


def _blocks(shape, dtype):
    """Piecewise-constant labels (8 x 8 x 12 blocks, the pattern shifted per slice): contours are thin, as on real label maps."""
    bc, i, j, k = big._terms(shape, "cuda")
    return ((bc % 7).to(dtype) + (i // 8 % 3).to(dtype) + (j // 8 % 5).to(dtype) * 3 + (k // 12 % 4).to(dtype) * 15).contiguous()


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_label_contour(hip, dtype):
    shape = big.shape_for(torch.uint8)  # the float32 OUTPUT passes 2^32 elements either way
    big.needs_gib(4.2 * dtype.itemsize + 17 + 3)
    data = _blocks(shape, dtype)
    out = hip.label_contour(data)
    assert out.dtype == torch.float32 and 0.02 < float(out[0].mean()) < 0.6
    _each_slice(out, lambda a, b: label_cases.contour(data[a:b]), 1, "label_contour")


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_mask_where(hip, dtype):
    big.needs_gib(GIB[dtype] + 2 * 17 if dtype == torch.uint8 else 3 * GIB[dtype])
    data = _input(dtype)
    mask = big.distinct((1, data.shape[1], *data.shape[2:]), torch.uint8, "cuda")[0] % 3  # (C, I, J, K): zero on a third
    out = hip.mask_where(data, mask, -5.0)
    _each_slice(out, lambda a, b: torch.where(mask[None] != 0, data[a:b].float(), torch.tensor(-5.0, device="cuda")), 1, "mask_where")


@pytest.mark.parametrize("dtype", MOVER_DTYPES, ids=MOVER_IDS)
def test_clamp(hip, dtype):
    big.needs_gib(GIB[dtype] + 2 * 17 if dtype == torch.uint8 else 3 * GIB[dtype])
    data = _input(dtype)
    out = hip.clamp(data, 30.5, 201.0)
    _each_slice(out, lambda a, b: data[a:b].clamp(30.5, 201.0), 1, "clamp")


def test_kspace_segment_mix(hip):
    """Float32 only.  The band-pass table multiplies along I, so the whole-tensor leg is the same call on batch slices; the
    crossing slices are held to the float64 product of the library's own (host-built) table with the segments."""
    big.needs_gib(4 * GIB[torch.float32])
    shape = big.shape_for(torch.float32)
    still = big.distinct(shape, torch.float32, "cuda")
    moved = torch.flip(still, [3])
    bounds = (0, 150, shape[2])
    active = torch.ones(shape[0], dtype=torch.uint8, device="cuda")
    out = hip.kspace_segment_mix([still, moved], bounds, torch.float32, active=active)
    for begin in range(shape[0]):
        part = hip.kspace_segment_mix([still[begin : begin + 1], moved[begin : begin + 1]], bounds, torch.float32, active=active[:1])
        assert big.same(out[begin : begin + 1], part), f"element {begin}: {big.first_difference(out[begin : begin + 1], part)}"
    # the FFT route in float64 at the bar of test_kspace_segment_mix_matches_the_fft_route, 1e-5 of the magnitude (the planes
    # are planes of the FIRST spatial axis, so the transform along that axis alone is the whole of it)
    for bc in big.crossing_slices(shape, torch.float32):
        spectrum = torch.fft.fft(still[bc, 0].double(), dim=0)
        spectrum[bounds[1] : bounds[2]] = torch.fft.fft(moved[bc, 0].double(), dim=0)[bounds[1] : bounds[2]]
        expected = torch.fft.ifft(spectrum, dim=0).real
        worst, bar = float((out[bc, 0].double() - expected).abs().max()), 1e-5 * float(expected.abs().max())
        print(f"[large] kspace_segment_mix slice {bc}: max|d| = {worst:.3e}, bar = {bar:.3e}")
        assert worst <= bar, (bc, worst, bar)
        del spectrum, expected


# ==== float arithmetic per voxel ============================================================================================
WIDE = big.shape_for(torch.float32, wide=True)  # (11, 3, 400, 404, 420): past 2^31 elements
WIDE_GIB = math.prod(WIDE) * 4 / 1024**3


def _pieces(shape, dtype):
    """The windows cut at batch-element boundaries: ``(name, batch element, start, stop)`` with flat element indices."""
    per_element = math.prod(shape[1:])
    found = []
    for name, start, stop in big.windows(shape, dtype):
        while start < stop:
            b = start // per_element
            end = min(stop, (b + 1) * per_element)
            found.append((name, b, start, end))
            start = end
    return found


def _piece(tensor: torch.Tensor, start: int, stop: int) -> torch.Tensor:
    """A window of a device tensor as a ``(1, 1, 1, 1, n)`` CPU tensor: what an engine takes as one batch element."""
    return tensor.reshape(-1)[start:stop].cpu().reshape(1, 1, 1, 1, -1)


def _against_slices(out, call, data, *per_element, what):
    """Leg (a) of the float family: the big call's result against the same entry point on batch slices below 2^31 bytes."""
    step = big.batch_step(data, 4)
    assert data[:step].numel() * 4 < big.SLICE_LIMIT
    _each_slice(out, lambda a, b: call(data[a:b], *(None if p is None else p[a:b] for p in per_element)), step, what)


def test_gamma_pow(hip):
    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0  # [-3, 37): both signs
    gamma = torch.linspace(0.6, 1.6, WIDE[0])
    out = hip.gamma_pow(data, gamma)
    _against_slices(out, lambda x, g: hip.gamma_pow(x, g), data, gamma, what="gamma_pow")
    for name, b, start, stop in _pieces(WIDE, torch.float32):
        x = _piece(data, start, stop).double()
        reference = x.sign() * x.abs().pow(float(gamma[b].double()))  # (the float32 exponent the C ABI carries)
        d = (_piece(out, start, stop).double() - reference).abs()
        bar = pointwise.GAMMA_RTOL[torch.float32] * reference.abs() + pointwise.GAMMA_FLOOR[torch.float32]
        print(f"[large] gamma_pow {name}: max d / bar = {float((d / bar).max()):.3g}")
        assert bool((d <= bar).all()), (name, float((d / bar).max()))


def test_bias_field_apply(hip):
    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0
    coarse = (0.5 * torch.randn(*WIDE[:2], 5, 6, 7, generator=torch.Generator().manual_seed(1))).cuda()
    skip = torch.tensor([b == 4 for b in range(WIDE[0])], dtype=torch.uint8)
    out = hip.bias_field_apply(data, coarse, skip=skip.cuda())
    assert torch.equal(out[4], data[4])
    _against_slices(out, lambda x, c, s: hip.bias_field_apply(x, c, skip=s.cuda()), data, coarse, skip, what="bias_field_apply")
    for bc in big.crossing_slices(WIDE, torch.float32):
        b, c = divmod(bc, WIDE[1])
        if skip[b]:
            continue
        reference = pointwise.bias_reference(data[b : b + 1, c : c + 1], coarse[b : b + 1, c : c + 1], False)
        relative = float(((out[b : b + 1, c : c + 1].double() - reference).abs() / reference.abs().clamp_min(1e-30)).max())
        bar = pointwise.bias_bar(coarse[b : b + 1, c : c + 1], torch.float32)
        print(f"[large] bias_field_apply slice {bc}: relative {relative:.3g} (bar {bar:.3g})")
        assert relative <= bar, (bc, relative, bar)
        del reference


def test_add_noise_explicit_draws(hip, oracle):
    big.needs_gib(4 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0
    draws = big.distinct(WIDE, torch.float32, "cuda") / 480.0 - 1.0  # "draws" that are a function of the position, in [-1, 1]
    mean, std = torch.linspace(-0.2, 0.3, WIDE[0]), torch.linspace(0.1, 0.9, WIDE[0])
    keep = torch.tensor([b != 2 for b in range(WIDE[0])], dtype=torch.uint8)
    out = hip.add_noise(data, mean, std, base1=draws, keep=keep.cuda())
    step = big.batch_step(data, 4)
    _each_slice(out, lambda a, b: hip.add_noise(data[a:b], mean[a:b], std[a:b], base1=draws[a:b], keep=keep[a:b].cuda()), step, "add_noise, explicit draws")
    for name, b, start, stop in _pieces(WIDE, torch.float32):  # bit for bit against the oracle (test_gpu_ops_parity.py holds them equal)
        expected = oracle.add_noise(_piece(data, start, stop), mean[b : b + 1], std[b : b + 1], base1=_piece(draws, start, stop), keep=keep[b : b + 1])
        assert torch.equal(_piece(out, start, stop), expected), name


def _no_block_repeats_the_one_2_32_bytes_before(out: torch.Tensor) -> None:
    """A 32-bit byte offset (or a 30-bit element index) in a Philox-keyed kernel repeats the stream: on the device, no
    4096-element block may equal the block that lies 2^32 bytes before it."""
    flat = out.reshape(-1)
    period = 2**32 // flat.element_size()
    tail = flat[period:]
    blocks = tail.numel() // big.WINDOW
    assert blocks > 0
    same = (tail[: blocks * big.WINDOW].view(blocks, big.WINDOW) == flat[: blocks * big.WINDOW].view(blocks, big.WINDOW)).all(dim=1)
    assert not bool(same.any()), f"{int(same.sum())} of {blocks} blocks repeat the block 2^32 bytes before them"


def test_philox_normal(hip):
    big.needs_gib(2 * WIDE_GIB)
    seed, stream = 0x9E3779B97F4A7C15, 1
    out = hip.philox_normal(WIDE, seed, stream, "cuda")
    for name, start, stop in big.windows(WIDE, torch.float32):
        z = big.philox_window(seed, stream, start, stop)
        d = (out.reshape(-1)[start:stop].cpu().double() - z).abs()
        print(f"[large] philox_normal {name}: max|d| = {float(d.max()):.3g}")
        assert bool((d <= pointwise.philox_bar(z)).all()), name
    _no_block_repeats_the_one_2_32_bytes_before(out)


def test_add_noise_philox(hip):
    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0
    seed = 0x1234_5678_9ABC_DEF0
    mean, std = torch.linspace(-0.2, 0.3, WIDE[0]), torch.linspace(0.1, 0.9, WIDE[0])
    out = hip.add_noise(data, mean, std, philox_seed=seed)
    for name, b, start, stop in _pieces(WIDE, torch.float32):  # the draws are keyed by the index in the WHOLE tensor, stream 0
        z = big.philox_window(seed, 0, start // 4 * 4, stop)[start % 4 :]
        reference = _piece(data, start, stop).reshape(-1).double() + (float(mean[b]) + float(std[b]) * z)
        d = (_piece(out, start, stop).reshape(-1).double() - reference).abs()
        bar = float(std[b]) * pointwise.philox_bar(z) + pointwise.EPS * reference.abs()
        print(f"[large] add_noise philox {name}: max d / bar = {float((d / bar).max()):.3g}")
        assert bool((d <= bar).all()), name
    _no_block_repeats_the_one_2_32_bytes_before(out - data)


def test_intensity_map(hip):
    """Bit for bit the reference's own expressions (``intensity_stats_cases``), which the kernel rounds operation by operation."""
    import intensity_stats_cases as stats

    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0
    low = [0.1 * b - 0.5 for b in range(WIDE[0])]
    high = [1.0 + 0.3 * b for b in range(WIDE[0])]
    out_min, out_max = torch.tensor(low), torch.tensor(high)
    out = hip.intensity_map(data, "rescale_clip", in_min=-1.5, in_max=30.25, in_range=31.75, out_min=out_min.cuda(), out_range=(out_max - out_min).cuda())
    _against_slices(out, lambda x, m, r: hip.intensity_map(x, "rescale_clip", in_min=-1.5, in_max=30.25, in_range=31.75, out_min=m.cuda(), out_range=r.cuda()),
                    data, out_min, out_max - out_min, what="intensity_map rescale_clip")
    for name, b, start, stop in _pieces(WIDE, torch.float32):
        expected = stats.normalize(_piece(data, start, stop), -1.5, 30.25, [low[b]], [high[b]])
        assert torch.equal(_piece(out, start, stop), expected), name
    del out
    out = hip.intensity_map(data, "sub_div", in_min=7.25, in_range=3.5)
    _against_slices(out, lambda x: hip.intensity_map(x, "sub_div", in_min=7.25, in_range=3.5), data, what="intensity_map sub_div")
    for name, b, start, stop in _pieces(WIDE, torch.float32):
        assert torch.equal(_piece(out, start, stop), stats.standardize(_piece(data, start, stop), 7.25, 3.5)), name


def test_intensity_map_of_bytes(hip):
    """uint8 in, float32 out: the input passes 2^32 elements, the output 2^34 bytes."""
    import intensity_stats_cases as stats

    shape = big.shape_for(torch.uint8)
    big.needs_gib(4.2 + 16.5 + 8)
    data = big.distinct(shape, torch.uint8, "cuda")
    out = hip.intensity_map(data, "mul_add", in_min=-2.0, in_range=0.375)
    _against_slices(out, lambda x: hip.intensity_map(x, "mul_add", in_min=-2.0, in_range=0.375), data, what="intensity_map mul_add")
    for name, b, start, stop in _pieces(shape, torch.float32):
        assert torch.equal(_piece(out, start, stop), stats.standardize_inverse(_piece(data, start, stop), -2.0, 0.375)), name


def test_histogram_standardize(hip):
    shape = big.shape_for(torch.float32)
    big.needs_gib(3 * GIB[torch.float32] + 2)
    data = big.distinct(shape, torch.float32, "cuda")
    quantiles = swap_histogram_cases.DEFAULT_QUANTILES
    landmarks = swap_histogram_cases.landmarks_for(quantiles)
    out = hip.histogram_standardize(data, landmarks.cuda(), quantiles)
    _against_slices(out, lambda x: hip.histogram_standardize(x, landmarks.cuda(), quantiles), data, what="histogram_standardize")
    for _, _, (bc, _, _, _) in big.crossings(shape, torch.float32):  # the element of each crossing against the numpy restatement
        expected = swap_histogram_cases.standardize_element(data[bc].cpu(), landmarks, quantiles)
        assert swap_histogram_cases.same(out[bc].cpu(), expected), bc


def test_channel_project(hip):
    """(11, 3) channels to two components: input past 2^31 elements, output past 2^32 bytes."""
    import pca_cases

    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") - 3.0
    generator = torch.Generator().manual_seed(5)
    center = torch.randn(WIDE[0], 3, generator=generator).cuda()
    weights = (0.1 * torch.randn(WIDE[0], 2, 3, generator=generator)).cuda()
    offset = torch.rand(WIDE[0], 2, generator=generator).cuda()
    out = hip.channel_project(data, center, weights, offset, clip=True)
    assert len(big.crossings(out.shape, out.dtype)) == 2
    _against_slices(out, lambda x, c, w, o: hip.channel_project(x, c, w, o, clip=True), data, center, weights, offset, what="channel_project")
    voxels = math.prod(WIDE[2:])
    for name, start, stop in big.windows(out.shape, out.dtype):  # (2^-24 (C + 4) (sum |W| |x - c| + |o|): pca_cases.rounding_bound)
        b, rest = divmod(start, 2 * voxels)
        component, first = divmod(rest, voxels)
        count = min(stop - start, voxels - first)  # (the part of the window inside this component's volume)
        x = data[b].reshape(3, voxels)[:, first : first + count].double().cpu().numpy()
        centred = x - center[b].double().cpu().numpy()[:, None]
        w, o = weights[b, component].double().cpu().numpy(), float(offset[b, component])
        exact = {"weights": w[None], "centred": centred, "offset": np.array([o]), "out": (w @ centred + o)[None]}
        got = out.reshape(-1)[start : start + count].double().cpu().numpy()
        assert bool((abs(got - exact["out"][0].clip(0.0, 1.0)) <= pca_cases.rounding_bound(exact)[0]).all()), name


def test_interpolate3d_linear(hip, oracle):
    """Trilinear, align_corners: leg (a) against batch slices; the crossing slices against the CPU oracle bit for bit (both
    restate ATen's arithmetic: test_gpu_ops_parity.py holds them equal)."""
    shape = big.shape_for(torch.float32)
    big.needs_gib(3.3 * GIB[torch.float32] + 2)
    data = big.affine_field(shape, "cuda")
    out_shape = (407, 397, 424)
    out = hip.interpolate3d(data, out_shape, "linear")
    assert len(big.crossings(out.shape, out.dtype)) == 2
    _against_slices(out, lambda x: hip.interpolate3d(x, out_shape, "linear"), data, what="interpolate3d linear")
    for bc in big.crossing_slices(out.shape, out.dtype):
        expected = oracle.interpolate3d(data[bc : bc + 1].cpu(), out_shape, "linear")
        assert torch.equal(out[bc : bc + 1].cpu(), expected), f"slice {bc}: {big.first_difference(out[bc : bc + 1].cpu(), expected)}"


def test_bspline_prefilter(hip, oracle):
    """17 float32 volumes: one recursive filter per line and axis, every volume on its own — against batch slices, and the
    volume of the 2^32-byte crossing against the CPU oracle, bit for bit (test_gpu_bspline.py holds the two equal)."""
    shape = big.shape_for(torch.float32)
    big.needs_gib(3 * GIB[torch.float32])
    data = big.distinct(shape, torch.float32, "cuda") / 24.0 - 10.0
    out = hip.bspline_prefilter(data, 3)
    _each_slice(out, lambda a, b: hip.bspline_prefilter(data[a:b], 3), big.batch_step(data, 4), "bspline_prefilter")
    for _, _, (bc, _, _, _) in big.crossings(shape, torch.float32)[-1:]:  # volume 15, with the 2^32-byte crossing (the oracle takes seconds per volume)
        expected = oracle.bspline_prefilter(data[bc : bc + 1].cpu(), 3)
        assert torch.equal(out[bc : bc + 1].cpu(), expected), f"volume {bc}: {big.first_difference(out[bc : bc + 1].cpu(), expected)}"


def test_axis_gather_lerp_blend(hip):
    """The two-point blend: ``lower * (1 - w) + upper * w`` with every operation rounded, so torch's float32 is the same bits."""
    shape = big.shape_for(torch.float32)
    big.needs_gib(3 * GIB[torch.float32])
    data = big.distinct(shape, torch.float32, "cuda")
    batch, length = shape[0], shape[3]
    lower = (torch.arange(length)[None] * 5 + torch.arange(batch)[:, None] * 3) % length
    upper = (lower + 1).clamp_max(length - 1)
    weight = ((torch.arange(length)[None] * 37 + torch.arange(batch)[:, None]) % 101).float() / 101.0
    out = hip.axis_gather_lerp(data, 1, lower, upper, weight)
    lo, up, w = lower.cuda(), upper.cuda(), weight.cuda()

    def expected(a, b):
        blend = w[a].reshape(1, 1, 1, -1, 1)
        return data[a:b].index_select(3, lo[a]) * (1.0 - blend) + data[a:b].index_select(3, up[a]) * blend

    _each_slice(out, expected, 1, "axis_gather_lerp blend")


# ==== stencil ===============================================================================================================
def _stencil_case(dtype):
    """float32: 17 volumes of 516 x 520 x 252 (past 2^32 bytes, the marching I pass and the fused J + K pass); float64: 9 of them
    (past 2^32 bytes as well: the generic line and K kernels).  Asymmetric per-element taps that sum to one."""
    from stencil_geometry_cases import TAP_STRIDE

    shape = ((17 if dtype == torch.float32 else 9), 1, *big.STENCIL_VOLUME)
    assert len(big.crossings(shape, dtype)) == 2
    data = (big.distinct(shape, torch.float32, "cuda") / 8.0 - 50.0).to(dtype)
    generator = torch.Generator().manual_seed(11)

    def taps_for(radius):
        taps = torch.zeros((shape[0], 3, TAP_STRIDE), dtype=torch.float32)
        for axis, r in enumerate(radius):
            w = torch.rand((shape[0], 2 * r + 1), generator=generator, dtype=torch.float64) + 0.05
            taps[:, axis, : 2 * r + 1] = (w / w.sum(dim=1, keepdim=True)).to(torch.float32)
        return taps

    return shape, data, taps_for


@pytest.mark.parametrize("radius", [1, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_separable_conv3d(hip, oracle, dtype, radius):
    from stencil_geometry_cases import reported_passes

    big.needs_gib(30)
    shape, data, taps_for = _stencil_case(dtype)
    radius = [radius] * 3
    passes, _ = reported_passes(hip._fn, shape, radius, dtype=dtype, has_skip=True)
    assert [p.family for p in passes] == (["march", "march"] if dtype == torch.float32 else ["line", "march", "k"])
    taps = taps_for(radius)
    skip = torch.tensor([b == 2 for b in range(shape[0])], dtype=torch.uint8)  # (no volume with a crossing)
    out = hip.separable_conv3d(data, taps.cuda(), radius, skip=skip.cuda())
    assert torch.equal(out[2], data[2])
    step = big.batch_step(data, 8)  # (the scratch of a call is two float32 volumes per data volume)
    _each_slice(out, lambda a, b: hip.separable_conv3d(data[a:b], taps[a:b].cuda(), radius, skip=skip[a:b].cuda()), step, "separable_conv3d")
    for _, _, (bc, _, _, _) in big.crossings(shape, dtype):  # bit for bit against the CPU oracle (test_gpu_stencil_geometry.py holds them equal)
        expected = oracle.separable_conv3d(data[bc : bc + 1].cpu(), taps[bc : bc + 1], radius, skip=skip[bc : bc + 1])
        assert torch.equal(out[bc : bc + 1].cpu(), expected), f"volume {bc}: {big.first_difference(out[bc : bc + 1].cpu(), expected)}"


def test_separable_conv3d_long_rows(hip, oracle):
    """17 float32 volumes of 400 x 404 x 420: rows beyond 256 voxels leave the fused J + K pass for a K pass of its own (the
    vectorised ``k_v4`` kernel) behind two marching passes."""
    from stencil_geometry_cases import TAP_STRIDE, reported_passes

    big.needs_gib(24)
    shape = big.shape_for(torch.float32)
    found = big.crossings(shape, torch.float32)
    radius = [2, 2, 2]
    passes, _ = reported_passes(hip._fn, shape, radius)
    assert [p.family for p in passes] == ["march", "march", "k_v4"]
    data = big.distinct(shape, torch.float32, "cuda") / 8.0 - 50.0
    w = torch.rand((shape[0], 3, 5), generator=torch.Generator().manual_seed(13), dtype=torch.float64) + 0.05
    taps = torch.zeros((shape[0], 3, TAP_STRIDE))
    taps[:, :, :5] = (w / w.sum(dim=2, keepdim=True)).float()
    out = hip.separable_conv3d(data, taps.cuda(), radius)
    _each_slice(out, lambda a, b: hip.separable_conv3d(data[a:b], taps[a:b].cuda(), radius), 3, "separable_conv3d, long rows")
    for _, _, (bc, _, _, _) in found:
        expected = oracle.separable_conv3d(data[bc : bc + 1].cpu(), taps[bc : bc + 1], radius)
        assert torch.equal(out[bc : bc + 1].cpu(), expected), f"volume {bc}: {big.first_difference(out[bc : bc + 1].cpu(), expected)}"


def test_separable_conv3d_past_2_31_elements(hip, oracle):
    """33 float32 volumes, 2.23e9 elements: with the call's two scratch volumes per data volume 36 GiB, inside the cap."""
    from stencil_geometry_cases import TAP_STRIDE

    big.needs_gib(42)
    shape = (33, 1, *big.STENCIL_VOLUME)
    found = big.crossings(shape, torch.float32)
    assert [name for name, _, _ in found] == ["2^31 bytes", "2^32 bytes", "2^31 elements"]
    data = big.distinct(shape, torch.float32, "cuda") / 8.0 - 50.0
    radius = [1, 1, 1]
    w = torch.rand((shape[0], 3, 3), generator=torch.Generator().manual_seed(12), dtype=torch.float64) + 0.05
    taps = torch.zeros((shape[0], 3, TAP_STRIDE))
    taps[:, :, :3] = (w / w.sum(dim=2, keepdim=True)).float()
    out = hip.separable_conv3d(data, taps.cuda(), radius)
    _each_slice(out, lambda a, b: hip.separable_conv3d(data[a:b], taps[a:b].cuda(), radius), 3, "separable_conv3d, 33 volumes")
    for _, _, (bc, _, _, _) in found:
        expected = oracle.separable_conv3d(data[bc : bc + 1].cpu(), taps[bc : bc + 1], radius)
        assert torch.equal(out[bc : bc + 1].cpu(), expected), f"volume {bc}: {big.first_difference(out[bc : bc + 1].cpu(), expected)}"


@pytest.mark.parametrize("noise, reach", [("draws", 3), ("philox", 3), ("draws", 8)], ids=["draws", "philox", "draws-ring"])
def test_blur_fused(hip, oracle, noise, reach):
    """Bias, the marching I pass, the fused J + K pass and the noise in the stencil's launches, exact mode: bit for bit the chain
    ``bias_field_apply -> separable_conv3d -> add_noise`` (test_gpu_stencil_geometry.py).  Explicit draws: against batch slices of
    the fused call, and the crossing volumes against the chain through the CPU oracle.  Philox draws are keyed by the index in the
    whole tensor: against the chain of the big calls, whose members have their own tests in this file."""
    import torchio_amd as tio
    from stencil_geometry_cases import reported_passes

    big.needs_gib(40)
    shape, data, taps_for = _stencil_case(torch.float32)
    radius = [reach] * 3
    passes, stages = reported_passes(hip._fn, shape, radius, bias=True, noise=2 if noise == "draws" else 1)
    # the I pass (marching; at radius 8 with a bias stage the LDS-ring kernel) and the fused J + K pass
    assert [(p.family, p.radius_k) for p in passes] == [("march" if reach == 3 else "ring", 0), ("march", reach)]
    assert [(s["pre_bias"], s["post_noise"]) for s in stages] == [(1, 0), (0, 2 if noise == "draws" else 1)]
    taps = taps_for(radius)
    coarse = ((torch.rand((*shape[:2], 7, 3, 2), generator=torch.Generator().manual_seed(3)) - 0.5) * 0.6)
    mean, std = torch.linspace(-3.0, 3.0, shape[0]), torch.linspace(0.5, 20.0, shape[0])
    draws = big.distinct(shape, torch.float32, "cuda") / 480.0 - 1.0 if noise == "draws" else None
    seed = 0x1234_5678_9ABC_DEF0
    previous = tio.get_stencil_precision()
    tio.set_stencil_precision("exact")
    try:
        fused = lambda x, t, c, m, s, d: hip.blur_fused(x, t.cuda(), radius, bias_coarse=c.cuda(), noise=(m, s, d if noise == "draws" else seed))  # noqa: E731
        out = fused(data, taps, coarse, mean, std, draws)
        assert out is not None
        if noise == "draws":
            step = big.batch_step(data, 8)
            _each_slice(out, lambda a, b: fused(data[a:b], taps[a:b], coarse[a:b], mean[a:b], std[a:b], draws[a:b]), step, "blur_fused, explicit draws")
            for _, _, (bc, _, _, _) in big.crossings(shape, torch.float32):
                one = slice(bc, bc + 1)
                # (the bias step of one volume on the device: its expf is the device's; the stencil and the noise through the oracle)
                blurred = oracle.separable_conv3d(hip.bias_field_apply(data[one], coarse[one].cuda()).cpu(), taps[one], radius)
                expected = oracle.add_noise(blurred, mean[one], std[one], base1=draws[one].cpu())
                assert torch.equal(out[one].cpu(), expected), f"volume {bc}: {big.first_difference(out[one].cpu(), expected)}"
        else:
            blurred = hip.separable_conv3d(hip.bias_field_apply(data, coarse.cuda()), taps.cuda(), radius)
            chain = hip.add_noise(blurred, mean, std, philox_seed=seed)
            del blurred
            assert big.same(out, chain), big.first_difference(out, chain)
            del chain
            # and, independent of the library's big calls: the crossing volumes blurred by the CPU oracle plus the numpy Philox draw of
            # each voxel's index in the WHOLE tensor, at the noise bar of intensity_pointwise_cases.py
            per_volume = math.prod(shape[2:])
            for name, b, start, stop in _pieces(shape, torch.float32):
                if name in ("first", "last"):
                    continue
                one = slice(b, b + 1)
                blurred = oracle.separable_conv3d(hip.bias_field_apply(data[one], coarse[one].cuda()).cpu(), taps[one], radius).reshape(-1)
                z = big.philox_window(seed, 0, start // 4 * 4, stop)[start % 4 :]
                reference = blurred[start - b * per_volume : stop - b * per_volume].double() + (float(mean[b]) + float(std[b]) * z)
                d = (out.reshape(-1)[start:stop].cpu().double() - reference).abs()
                assert bool((d <= float(std[b]) * pointwise.philox_bar(z) + pointwise.EPS * reference.abs()).all()), name
    finally:
        tio.set_stencil_precision(previous)


def test_separable_conv3d_adjoint(hip, oracle):
    big.needs_gib(24)
    shape, grad, taps_for = _stencil_case(torch.float32)
    radius = [2, 1, 3]
    taps = taps_for(radius)
    skip = torch.tensor([b == 5 for b in range(shape[0])], dtype=torch.uint8)
    out = hip.separable_conv3d_adjoint(grad, taps.cuda(), radius, skip=skip.cuda())
    step = big.batch_step(grad, 8)
    _each_slice(out, lambda a, b: hip.separable_conv3d_adjoint(grad[a:b], taps[a:b].cuda(), radius, skip=skip[a:b].cuda()), step, "separable_conv3d_adjoint")
    for _, _, (bc, _, _, _) in big.crossings(shape, torch.float32):  # the bar of test_stencil_adjoint.py between the two engines
        expected = oracle.separable_conv3d_adjoint(grad[bc : bc + 1].cpu(), taps[bc : bc + 1], radius)
        worst, bar = float((out[bc : bc + 1].cpu() - expected).abs().max()), 2e-6 * float(expected.abs().max()) * (2 * max(radius) + 1)
        print(f"[large] separable_conv3d_adjoint volume {bc}: max|d| = {worst:.3g} (bar {bar:.3g})")
        assert worst <= bar, (bc, worst, bar)


# ==== reductions ============================================================================================================
BYTE_VOLUME = (1, 1, 1640, 1620, 1620)  # 4 304 016 000 voxels in ONE channel: 9 048 704 beyond 2^32
FLOAT_VOLUME = (1, 1, 1300, 1290, 1284)  # 2 153 268 000: 5 784 352 beyond 2^31
TAIL = 5_000_000  # the last voxels of each: behind the last threshold


def _planted(shape, dtype):
    """One value (100) everywhere but in the last TAIL voxels, which hold 20 .. 219 by position; the minimum 3, the maximum 250
    and the label 7 occur once each, in the tail.  More than 2^32 (float32: 2^31) voxels hold 100: a 32-bit count of them wraps."""
    numel = math.prod(shape)
    assert numel - TAIL > (2**32 if dtype.itemsize == 1 else 2**31)
    data = torch.full(shape, 100, dtype=dtype, device="cuda")
    flat = data.view(-1)
    position = torch.arange(TAIL, device="cuda")
    flat[numel - TAIL :] = (20 + (position * 7 % 200)).to(dtype)
    flat[numel - 5], flat[numel - 9], flat[numel - 11] = 3, 250, 7
    return data


def _histogram(data):
    """int64 counts of the values 0 .. 255, chunk by chunk."""
    flat, counts = data.view(-1), torch.zeros(256, dtype=torch.int64, device=data.device)
    for begin in range(0, flat.numel(), 2**29):
        counts += torch.bincount(flat[begin : begin + 2**29].long(), minlength=256)
    return counts.cpu()


def _kth(counts, k):
    """The k-th smallest value (0-based) of a histogram."""
    return int(torch.searchsorted(torch.cumsum(counts, 0), torch.tensor(k), right=True))


@pytest.mark.parametrize("shape, dtype", [(BYTE_VOLUME, torch.uint8), (FLOAT_VOLUME, torch.float32)], ids=MOVER_IDS)
def test_statistics_of_one_huge_channel(hip, shape, dtype):
    """``channel_min``, ``intensity_moments``, ``intensity_quantiles``, ``intensity_multi_quantiles`` and ``unique_labels`` on one
    channel of more than 2^32 (float32: 2^31) voxels, against int64 / float64 torch reductions taken chunk by chunk."""
    import intensity_stats_cases as stats

    big.needs_gib(3 * math.prod(shape) * dtype.itemsize / 1024**3 + 6)
    data = _planted(shape, dtype)
    numel = data.numel()
    assert float(hip.channel_min(data)) == 3.0
    counts = _histogram(data)  # (exact: the values are small integers in both dtypes)
    values = torch.arange(256, dtype=torch.float64)
    assert int(counts.sum()) == numel and int(counts[100]) > (2**32 if dtype.itemsize == 1 else 2**31)
    exact_mean = float((counts.double() * values).sum() / numel)  # (sums of integers below 2^53: exact)
    exact_std = math.sqrt(float((counts.double() * (values - exact_mean) ** 2).sum() / (numel - 1)))
    count, mean, std = hip.intensity_moments(data)
    print(f"[large] moments {dtype}: mean off by {stats.ulps_off(mean, exact_mean):.3f} ulp, std by {stats.ulps_off(std, exact_std):.3f} ulp")
    assert count == numel and stats.ulps_off(mean, exact_mean) <= 1.0 and stats.ulps_off(std, exact_std) <= 1.0
    # quantiles: the order statistics from the histogram, the reference's lerp on 0-dim float32 tensors (_statistics.py:36-43)
    fractions = [0.0, 0.25, 0.5, 1.0 - 2.0e-4, 1.0 - 1.0e-9, 1.0]
    expected = []
    for q in fractions:
        index = q * (numel - 1)
        lower = math.floor(index)
        low, high = (torch.tensor(float(_kth(counts, min(k, numel - 1)))) for k in (lower, lower + 1))
        expected.append(float(low if index == lower else low.lerp(high, index - lower)))
    assert expected[0] == 3.0 and expected[-1] == 250.0 and expected[2] == 100.0 and expected[3] != 100.0
    assert hip.intensity_quantiles(data, fractions) == expected
    # percentiles (np.percentile's linear rule, in float64, from the same order statistics)
    percentiles, inside = hip.intensity_multi_quantiles(data, fractions)
    assert inside.tolist() == [numel]
    for q, got in zip(fractions, percentiles[0].tolist()):
        index = q * (numel - 1)
        lower = math.floor(index)
        low, high, t = float(_kth(counts, lower)), float(_kth(counts, min(lower + 1, numel - 1))), index - lower
        assert got == (high - (high - low) * (1 - t) if t >= 0.5 else low + (high - low) * t), q
    if dtype == torch.uint8:
        assert hip.unique_labels(data).tolist() == [float(v) for v in range(256) if counts[v] > 0]
        assert counts[7] == 1 and counts[250] == 1


def test_channel_min_of_many_channels(hip):
    """65 uint8 channels of 2^26 voxels: the channels' offsets pass 2^32; every channel's minimum is planted at its end."""
    shape = (1, 65, *big.VOLUME)
    big.needs_gib(12)
    data = big.distinct(shape, torch.uint8, "cuda") % 200 + 40
    lows = torch.arange(65, dtype=torch.uint8, device="cuda") % 37
    data[0, :, -1, -1, -3] = lows
    assert torch.equal(hip.channel_min(data), lows.float())


def test_channel_scatter(hip):
    """33 float32 channels of 2^26 voxels (past 2^31 elements) against EXACT sums: the data are integers, so a float64 sum of a
    channel's values or of two channels' products is an integer below 2^53 — exact — and the centring is done in rational
    arithmetic.  Every mean, and the scatter of every pair among the channels round the thresholds."""
    from fractions import Fraction

    channels, voxels = 33, math.prod(big.VOLUME)
    shape = (1, channels, *big.VOLUME)
    big.needs_gib(14)
    factor = (torch.arange(channels, device="cuda") % 3 + 1).reshape(1, -1, 1, 1, 1).float()
    data = big.distinct(shape, torch.float32, "cuda") * factor  # integers up to 2880; the channels differ in scale and offset
    mean, scatter = hip.channel_scatter(data)
    flat = data.reshape(channels, voxels)
    sums = [int(flat[c].double().sum()) for c in range(channels)]  # (integers whose sum stays below 2^53: exact in any order)
    got_mean, got = mean[0].tolist(), scatter[0].tolist()
    checked = [0, 7, 8, 15, 16, 31, 32]  # the channels round the thresholds, the first and the last; every pair of them
    products = {(i, j): int((flat[i].double() * flat[j].double()).sum()) for i in checked for j in checked if i <= j}
    exact = {pair: Fraction(value) - Fraction(sums[pair[0]] * sums[pair[1]], voxels) for pair, value in products.items()}
    diagonal = {i: math.sqrt(float(exact[i, i])) for i in checked}
    for c in range(channels):  # the bars of test_gpu_pca.py
        deviation = diagonal[c] / math.sqrt(voxels - 1) if c in diagonal else 0.0
        assert abs(got_mean[c] - sums[c] / voxels) <= 1e-12 * max(abs(sums[c] / voxels), deviation), c
    for (i, j), value in exact.items():
        assert abs(got[i][j] - float(value)) <= 1e-9 * diagonal[i] * diagonal[j] and got[i][j] == got[j][i], (i, j)


def test_complex_abs_max(hip):
    """Two rows of 2^29 + 1000 complex64 values (8.6 GB): the second row starts past 2^32 bytes and holds its maximum at its end."""
    rows, n = 2, 2**29 + 1000
    big.needs_gib(10)
    spectrum = torch.zeros((rows, n, 2), dtype=torch.float32, device="cuda")
    position = torch.arange(n, device="cuda")
    spectrum[0, :, 0], spectrum[1, :, 1] = (position % 1000).float(), (position % 777).float()
    spectrum[1, n - 3] = torch.tensor([3000.0, 4000.0])  # |.| = 5000 exactly
    spectrum[0, 2**28 + 5] = torch.tensor([-1200.0, 500.0])  # 1300, past 2^31 bytes
    assert hip.complex_abs_max(torch.view_as_complex(spectrum)).tolist() == [1300.0, 5000.0]


def test_centre_draw(hip):
    """A uint8 weight map of more than 2^32 voxels with all of its weight behind voxel 2^32: every centre lies there, and is
    the one the float64 cumulative sum of the (integer) weights gives for the draw's own uniform."""
    import patch_feed_cases

    shape = BYTE_VOLUME[2:]
    numel = math.prod(shape)
    big.needs_gib(6)
    source = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    position = torch.arange(TAIL, device="cuda")
    source.view(-1)[numel - TAIL :] = (position * 7 % 5).to(torch.uint8)
    draw = hip.centre_draw(source, (1, 1, 1), 256, seed=17, return_uniforms=True)
    centres = draw.centres.cpu().numpy()
    assert centres.min() >= 2**32 and centres.max() < numel
    tail = source.view(-1)[numel - TAIL :].cpu().numpy().astype(np.float64)
    indices, _, total = patch_feed_cases.draw_reference(tail, draw.uniforms.cpu().numpy())
    assert np.array_equal(centres, indices + (numel - TAIL))
    record = draw.record.cpu()
    assert float(record[:2].view(torch.float64)) == total
    assert np.array_equal(draw.corners.cpu().numpy(), patch_feed_cases.corners_reference(centres, shape, (1, 1, 1)))


def test_gamma_grad(hip):
    """``sum gy y log|x|`` per element over 2^31 + voxels: the float64 sums taken slice by slice, ``param_grad_reference``'s bound."""
    import param_grad_reference as reference

    big.needs_gib(3 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda") + 0.5  # positive: [0.5, 40)
    gy = big.distinct(WIDE, torch.float32, "cuda") / 480.0 - 1.0
    gamma = torch.linspace(0.6, 1.6, WIDE[0])
    got = hip.gamma_grad(data, gy, gamma)
    refs, scales = [], []
    for b in range(WIDE[0]):
        x, g = data[b].double(), gy[b].double()
        term = g * x.pow(float(gamma[b].double())) * x.log()
        refs.append(float(term.sum()))
        scales.append(float(term.abs().sum()))
    reference.check("large gamma_grad", got, torch.tensor(refs, dtype=torch.float64), torch.tensor(scales, dtype=torch.float64), reference.C_GAMMA, reference.TAU)


# ==== the resampler: many small volumes ===========================================================================================
RES_VOLUME = (132, 136, 140)  # 2 513 280 voxels, 9^3 bricks; 428 float32 volumes are 4 302 735 360 bytes, past 2^32
RES_BATCH = 428
RES_STEP = 107  # batch elements per slice: 1.08 GB of float32


def _resample_geometry(batch, elastic=True):
    """Per-element mappings near the identity (a few degrees of rotation and shear, shifts of a few voxels); a 5^3 control grid
    whose cells span two bricks, switched off for every other element."""
    from case_inputs import _control_points, _mapping

    cp_skip = torch.tensor([b % 2 for b in range(batch)], dtype=torch.uint8)
    return dict(out_shape=RES_VOLUME, mapping=_mapping(batch, 7, scale=0.03, shift=2.0), in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True,
                control_points=_control_points(batch, (5, 5, 5), 8, amplitude=3.0) if elastic else None, cp_skip=cp_skip if elastic else None)


def _on(device, geometry, begin=None, end=None):
    moved = dict(geometry)
    for key in ("mapping", "control_points", "cp_skip"):
        if moved[key] is not None:
            moved[key] = moved[key][begin:end].to(device)
    return moved


def _crossing_elements(tensor):
    per_element = tensor[0].numel()
    return sorted({0, tensor.shape[0] - 1, *(element // per_element for _, element in big.thresholds(tensor.numel(), tensor.element_size()))})


#: name -> (precision, switches, control points, the float group starts from a plan, a fill rule)
RESAMPLE_ROADS = {
    "exact-lean": ("exact", {}, True, True, True),
    "tight-lean": ("tight", {}, True, True, True),
    "fast-planned": ("fast", {}, True, True, True),
    "exact-brick": ("exact", {"TIO_EXACT_LEAN": "0"}, True, False, True),
    "exact-planned-brick": ("exact", {"TIO_EXACT_LEAN": "0"}, False, True, True),
    "fast-brick": ("fast", {"TIO_FAST_KERNEL": "brick"}, True, False, True),
    "gather": ("exact", {"TIO_RESAMPLE_PATH": "gather"}, True, False, True),
    "gather-zero-padding": ("exact", {"TIO_RESAMPLE_PATH": "gather"}, True, False, False),  # (no mask: the interior voxels' own sampling code)
}


@pytest.mark.parametrize("road", sorted(RESAMPLE_ROADS))
def test_resample3d_trilinear_roads(hip, oracle, monkeypatch, road):
    from test_gpu_resample_planned import REL_TOL, _rel, starts_from_a_plan

    precision, switches, elastic, planned, with_fill = RESAMPLE_ROADS[road]
    for key, value in switches.items():
        monkeypatch.setenv(key, value)
    big.needs_gib(12)
    data = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.float32, "cuda") / 240.0 - 1.0  # [-1, 3]: the range REL_TOL is stated for
    assert data.numel() * 4 > 2**32
    geometry = _resample_geometry(RES_BATCH, elastic)
    launch = dict(interps=["linear"], fills=[torch.tensor([-1.0], device="cuda") if with_fill else None], precision=precision)
    whole = _on("cuda", geometry)
    assert starts_from_a_plan(hip, [data], **whole, precision=precision) == planned
    (out,) = hip.resample3d([data], **whole, **launch)
    _each_slice(out, lambda a, b: hip.resample3d([data[a:b]], **_on("cuda", geometry, a, b), **launch)[0], RES_STEP, f"resample3d {road}")
    for b in _crossing_elements(out):
        (expected,) = oracle.resample3d([data[b : b + 1].cpu()], **_on("cpu", geometry, b, b + 1), interps=["linear"], fills=[torch.tensor([-1.0]) if with_fill else None],
                                       precision="exact")
        got = out[b : b + 1].cpu()
        if precision == "exact":
            assert torch.equal(got, expected), f"element {b}: {big.first_difference(got, expected)}"
        else:  # the bar of test_gpu_resample_planned.py
            assert int(((got == -1.0) != (expected == -1.0)).sum()) == 0 and float(_rel(expected, got).max()) <= REL_TOL, (b, float(_rel(expected, got).max()))


def test_resample3d_label_channel_rides_with_the_floats(hip, oracle):
    """A float32 image and an int16 label map in one call: the label channel rides along the exact-coordinate launch."""
    big.needs_gib(20)
    data = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.float32, "cuda") / 8.0
    labels = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.int16, "cuda")
    geometry = _resample_geometry(RES_BATCH)
    launch = dict(interps=["linear", "nearest"], fills=[None, None], precision="exact")
    outs = hip.resample3d([data, labels], **_on("cuda", geometry), **launch)
    for begin in range(0, RES_BATCH, RES_STEP):
        parts = hip.resample3d([data[begin : begin + RES_STEP], labels[begin : begin + RES_STEP]], **_on("cuda", geometry, begin, begin + RES_STEP), **launch)
        for out, part in zip(outs, parts):
            assert big.same(out[begin : begin + RES_STEP], part), (begin, big.first_difference(out[begin : begin + RES_STEP], part))
    for b in _crossing_elements(outs[0]):
        expected = oracle.resample3d([data[b : b + 1].cpu(), labels[b : b + 1].cpu()], **_on("cpu", geometry, b, b + 1), **launch)
        for out, theirs in zip(outs, expected):
            assert torch.equal(out[b : b + 1].cpu(), theirs), b


@pytest.mark.parametrize("kernel", ["narrow", "general"])
def test_resample3d_nearest_alone(hip, oracle, kernel):
    """856 int16 label maps (past 2^32 bytes) through the nearest kernels: without a fill rule the exact-coordinate kernel with its
    24-bit offsets and buffer loads, with one the general kernel (resample.hip: launch_nearest)."""
    batch = 2 * RES_BATCH
    big.needs_gib(12)
    labels = big.distinct((batch, 1, *RES_VOLUME), torch.int16, "cuda")
    assert labels.numel() * 2 > 2**32
    geometry = _resample_geometry(batch)
    fill = None if kernel == "narrow" else torch.tensor([-7.0])
    launch = dict(interps=["nearest"], precision="exact")
    (out,) = hip.resample3d([labels], **_on("cuda", geometry), fills=[None if fill is None else fill.cuda()], **launch)
    step = 2 * RES_STEP
    _each_slice(out, lambda a, b: hip.resample3d([labels[a:b]], **_on("cuda", geometry, a, b), fills=[None if fill is None else fill.cuda()], **launch)[0],
                step, f"resample3d nearest ({kernel})")
    for b in _crossing_elements(out):
        (expected,) = oracle.resample3d([labels[b : b + 1].cpu()], **_on("cpu", geometry, b, b + 1), fills=[fill], **launch)
        assert torch.equal(out[b : b + 1].cpu(), expected), b


def _explicit_adjoint(engine, grad, geometry, fill):
    import adjoint_reference

    geo = adjoint_reference.geometry(in_shape=RES_VOLUME, **geometry)
    return adjoint_reference.adjoint(engine, grad, geo, fill)


def test_resample3d_adjoint(hip, oracle):
    """The ``linear_adjoint`` launch (float atomics on the gather road) on 428 gradient volumes: the whole accumulator against batch
    slices and the crossing elements against the CPU oracle, each voxel within ``adjoint_reference.order_tolerance`` — two float32
    sums of the same products in another order."""
    import adjoint_reference

    big.needs_gib(30)
    grad = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.float32, "cuda") / 240.0 - 1.0
    geometry = _resample_geometry(RES_BATCH)
    fill = torch.tensor([-1.0], device="cuda")
    out = _explicit_adjoint(hip, grad, _on("cuda", geometry), fill)
    assert out.numel() * 4 > 2**32
    step = 54
    for begin in range(0, RES_BATCH, step):
        end = min(begin + step, RES_BATCH)
        part_geometry = _on("cuda", geometry, begin, end)
        part = _explicit_adjoint(hip, grad[begin:end], part_geometry, fill)
        tolerance = adjoint_reference.order_tolerance(adjoint_reference.geometry(in_shape=RES_VOLUME, **part_geometry), grad[begin:end])
        adjoint_reference.assert_within(out[begin:end], part, tolerance, f"adjoint, elements {begin}:{end}")
        del part, tolerance
    for b in _crossing_elements(out):
        one = _on("cpu", geometry, b, b + 1)
        expected = _explicit_adjoint(oracle, grad[b : b + 1].cpu(), one, fill.cpu())
        tolerance = adjoint_reference.order_tolerance(adjoint_reference.geometry(in_shape=RES_VOLUME, **one), grad[b : b + 1].cpu())
        adjoint_reference.assert_within(out[b : b + 1].cpu(), expected, tolerance, f"adjoint against the oracle, element {b}")


def _same_to_an_ulp(first, second) -> bool:
    """test_gpu_geometry_grad.py's rule for two evaluations of the same float64 sums: equal up to the last float32 rounding."""
    first, second = first.detach().cpu().double(), second.detach().cpu().double()
    return bool(((first - second).abs() <= torch.maximum(first.abs(), second.abs()) * 2.0**-23).all())


def test_resample3d_geometry_grad(hip):
    """428 elements, per-element mappings and control points: every element's gradient from the one big call against the same
    element's from batch slices (float64 sums rounded once: equal to an ulp), and element 427 — the last one, in which the
    2^32-byte crossing lies — within ``geometry_grad_reference``'s rounding bound and kink allowance of float64 autograd."""
    import geometry_grad_reference as reference

    big.needs_gib(16)
    data = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.float32, "cuda") / 240.0 - 1.0
    grads = big.distinct((RES_BATCH, 1, *RES_VOLUME), torch.float32, "cuda", first_slice=5) / 480.0 - 1.0
    geometry = _resample_geometry(RES_BATCH)
    whole = _on("cuda", geometry)
    d_mapping, d_control = hip.resample3d_geometry_grad([data], [grads], fills=[None], **whole)
    assert d_mapping.shape == (RES_BATCH, 3, 4) and d_control.shape == (RES_BATCH, 5, 5, 5, 3)
    assert bool((d_control[1::2] == 0).all()) and bool((d_control[0::2] != 0).any())  # every other element has its field switched off
    for begin in range(0, RES_BATCH, RES_STEP):
        end = begin + RES_STEP
        part_mapping, part_control = hip.resample3d_geometry_grad([data[begin:end]], [grads[begin:end]], fills=[None], **_on("cuda", geometry, begin, end))
        assert _same_to_an_ulp(d_mapping[begin:end], part_mapping) and _same_to_an_ulp(d_control[begin:end], part_control), begin
    elements = _crossing_elements(data)
    assert elements == [0, 213, RES_BATCH - 1]  # 2^31 bytes fall into element 213, 2^32 bytes into element 427, the last one
    for b in elements[-1:]:  # element 427, which holds the 2^32-byte crossing (the float64 restatement takes seconds per element on the host)
        one = _on("cpu", geometry, b, b + 1)
        geo = reference.geometry(in_shape=RES_VOLUME, **one)
        images, gradients = [data[b : b + 1].cpu()], [grads[b : b + 1].cpu()]
        case = {"name": f"element {b}", "analytic": reference.analytic(geo, images, gradients, [None]),
                "reference": reference.autograd_reference(geo, images, gradients, [None])}
        reference.check(case, d_mapping[b : b + 1], d_control[b : b + 1])


# ==== the entry points that draw or reduce per element ==========================================================================
def test_noise_grad(hip):
    """``d_mean = sum gy`` and ``d_std = sum gy z`` per element over 2^31 + voxels, explicit draws: float64 torch sums per element,
    ``param_grad_reference``'s bound (c = 0 and 1, no transcendental)."""
    import param_grad_reference as reference

    big.needs_gib(4 * WIDE_GIB)
    data = big.affine_field(WIDE, "cuda")
    gy = big.distinct(WIDE, torch.float32, "cuda") / 480.0 - 1.0
    draws = big.distinct(WIDE, torch.float32, "cuda", first_slice=3) / 480.0 - 1.0
    mean, std = torch.linspace(-0.2, 0.3, WIDE[0]), torch.linspace(0.1, 0.9, WIDE[0])
    d_mean, d_std = hip.noise_grad(data, gy, mean, std, base1=draws)
    refs = [[float(gy[b].double().sum()) for b in range(WIDE[0])], [float((gy[b].double() * draws[b].double()).sum()) for b in range(WIDE[0])]]
    scales = [[float(gy[b].double().abs().sum()) for b in range(WIDE[0])], [float((gy[b].double() * draws[b].double()).abs().sum()) for b in range(WIDE[0])]]
    as64 = lambda values: torch.tensor(values, dtype=torch.float64)  # noqa: E731
    reference.check("large noise_grad d_mean", d_mean, as64(refs[0]), as64(scales[0]), 0, 0.0)
    reference.check("large noise_grad d_std", d_std, as64(refs[1]), as64(scales[1]), 1, 0.0)


def test_bias_field_grad(hip):
    """The gradient with respect to a 5 x 6 x 7 coarse grid per volume, 33 volumes (2.24e9 voxels), in float64 on the device, one
    batch element at a time: the align-corners upsampling is three small matrices (``geometry_grad_reference.lerp_matrix``), so
    the field is ``exp`` of three contractions and the gradient the transposed contractions of ``gy x field`` — matrix products,
    where autograd through ``F.interpolate`` would add 2e8 voxels into 210 nodes with atomics.  ``param_grad_reference``'s
    ``A_p`` (the same with absolute values) and its count of roundings."""
    import geometry_grad_reference
    import param_grad_reference as reference

    big.needs_gib(3 * WIDE_GIB + 8)
    data = big.affine_field(WIDE, "cuda") - 3.0
    gy = big.distinct(WIDE, torch.float32, "cuda") / 480.0 - 1.0
    nodes = (5, 6, 7)
    coarse = (0.5 * torch.randn(*WIDE[:2], *nodes, generator=torch.Generator().manual_seed(2))).cuda()
    got = hip.bias_field_grad(data, gy, coarse)
    wi, wj, wk = (geometry_grad_reference.lerp_matrix(n, extent)[0].cuda() for n, extent in zip(nodes, WIDE[2:]))  # (extent, nodes) float64
    refs, scales = torch.zeros(coarse.shape, dtype=torch.float64), torch.zeros(coarse.shape, dtype=torch.float64)
    up = lambda grid: torch.einsum("ia,ajk->ijk", wi, torch.einsum("jb,abk->ajk", wj, torch.einsum("abc,kc->abk", grid, wk)))  # noqa: E731
    down = lambda volume: torch.einsum("ia,ibc->abc", wi, torch.einsum("ijc,jb->ibc", torch.einsum("ijk,kc->ijc", volume, wk), wj))  # noqa: E731
    for b in range(WIDE[0]):
        for c in range(WIDE[1]):
            field = torch.exp(up(coarse[b, c].double()))
            term = gy[b, c].double() * data[b, c].double() * field
            refs[b, c] = down(term).cpu()
            scales[b, c] = down(term.abs()).cpu()
            del field, term
    reference.check("large bias_field_grad", got, refs, scales, reference.c_bias(WIDE[2:], nodes), reference.TAU)


def test_separable_conv3d_taps_grad(hip):
    """Per-element tap gradients on the stencil's 17 volumes (past 2^32 bytes), radius 1 on every axis: float64 autograd through
    the three replicate-padded correlations on the device, one volume at a time, ``param_grad_reference``'s bound."""
    import param_grad_reference as reference

    big.needs_gib(30)
    shape, data, taps_for = _stencil_case(torch.float32)
    radius = [1, 1, 1]
    taps = taps_for(radius)
    gy = big.distinct(shape, torch.float32, "cuda", first_slice=2) / 480.0 - 1.0
    got = hip.separable_conv3d_taps_grad(data, gy, taps.cuda(), radius)
    assert got.shape == taps.shape

    def loss(x, g, weights):  # (param_grad_reference.taps_loss with its index on the device)
        for axis in range(3):
            extent = x.shape[2 + axis]
            positions = torch.arange(extent, device=x.device)
            out = torch.zeros_like(x)
            for t in range(3):
                out = out + weights[:, axis, t].reshape(-1, 1, 1, 1, 1) * x.index_select(2 + axis, (positions + t - 1).clamp(0, extent - 1))
            x = out
        return (g * x).sum()

    refs, scales = [], []
    for b in range(shape[0]):
        leaf = taps[b : b + 1].double().cuda().requires_grad_(True)
        magnitude = taps[b : b + 1].double().abs().cuda().requires_grad_(True)
        with torch.enable_grad():
            (ref,) = torch.autograd.grad(loss(data[b : b + 1].double(), gy[b : b + 1].double(), leaf), leaf)
            (a,) = torch.autograd.grad(loss(data[b : b + 1].double().abs(), gy[b : b + 1].double().abs(), magnitude), magnitude)
        refs.append(ref.cpu())
        scales.append(a.cpu())
    reference.check("large taps_grad", got, torch.cat(refs), torch.cat(scales), reference.c_taps(radius), 0.0)


def test_labels_to_image(hip):
    """Fused mode (Philox keyed by the index in the whole tensor) on 33 label volumes: the windows against the numpy Philox with the
    key's mean and deviation, no block repeating the one 2^32 bytes before; one-label mode against batch slices and torch."""
    shape = (WIDE[0] * WIDE[1], 1, *big.VOLUME)
    big.needs_gib(4 * WIDE_GIB)
    labels = (big.distinct(shape, torch.uint8, "cuda") % 5).contiguous()
    keys = [0, 1, 2, 4]  # (3 is no key: those voxels become 0)
    generator = torch.Generator().manual_seed(6)
    means = torch.rand(shape[0], 4, generator=generator) * 2 + 1
    stds = torch.rand(shape[0], 4, generator=generator) * 0.5 + 0.1
    seed = 0x0123_4567_89AB_CDEF
    out = hip.labels_to_image(labels, keys, means, stds, seed=seed)
    per_element = math.prod(big.VOLUME)
    for name, b, start, stop in _pieces(shape, torch.float32):
        z = big.philox_window(seed, 0, start // 4 * 4, stop)[start % 4 :]
        label = labels.reshape(-1)[start:stop].cpu().long()
        slot = torch.tensor([keys.index(v) if v in keys else 0 for v in label.tolist()])
        is_key = torch.tensor([v in keys for v in label.tolist()])
        reference = torch.where(is_key, means[b, slot].double() + stds[b, slot].double() * z, torch.zeros_like(z))
        bar = torch.where(is_key, stds[b, slot].double() * pointwise.philox_bar(z) + pointwise.EPS * reference.abs(), torch.zeros_like(z))
        d = (out.reshape(-1)[start:stop].cpu().double() - reference).abs()
        assert bool((d <= bar).all()), (name, float((d - bar).max()))
    assert per_element * shape[0] * 4 > 2**33
    _no_block_repeats_the_one_2_32_bytes_before(out)
    del out
    base = big.distinct(shape, torch.float32, "cuda", first_slice=1) / 480.0 - 1.0
    out = hip.labels_to_image(labels, keys, means, stds, base=base, base_key=2)
    _each_slice(out, lambda a, b: hip.labels_to_image(labels[a:b], keys, means[a:b], stds[a:b], base=base[a:b], base_key=2), 7, "labels_to_image, one label")
    for name, b, start, stop in _pieces(shape, torch.float32):
        label = labels.reshape(-1)[start:stop].cpu()
        expected = torch.where(label == 2, base.reshape(-1)[start:stop].cpu() * stds[b, 2] + means[b, 2], torch.zeros(stop - start))
        assert torch.equal(out.reshape(-1)[start:stop].cpu(), expected), name


def test_ghost_lines_and_add_spikes(hip):
    """17 float32 volumes (past 2^32 bytes), per-element axes, strengths and frequencies: both calls against batch slices bit for
    bit, and the crossing volumes against float64 — the 1-D FFT along the ghost axis with the listed planes scaled, the plane
    waves of the spikes written out — at the bar of ``kspace_artefact_cases.check``, 1e-5 of the magnitude."""
    import kspace_artefact_cases as artefacts

    shape = big.shape_for(torch.float32)
    big.needs_gib(3 * GIB[torch.float32] + 4)
    data = big.distinct(shape, torch.float32, "cuda") / 240.0
    batch = shape[0]
    axes = [b % 3 for b in range(batch)]
    strengths = [0.2 + 0.04 * b for b in range(batch)]
    frequencies = [[(3 + b) % 50 + 1, 2 * b + 7, 0] for b in range(batch)]
    out = hip.ghost_lines(data, axes, strengths, frequencies)
    for b in range(batch):
        part = hip.ghost_lines(data[b : b + 1], axes[b], strengths[b], frequencies[b])
        assert big.same(out[b : b + 1], part), f"ghost_lines, element {b}: {big.first_difference(out[b : b + 1], part)}"
    for bc in big.crossing_slices(shape, torch.float32):
        spectrum = torch.fft.fft(data[bc, 0].double(), dim=axes[bc])
        scale = torch.ones(shape[2 + axes[bc]], dtype=torch.float64, device="cuda")
        for f in frequencies[bc]:
            scale[f] -= float(np.float32(strengths[bc]))
        view = [1, 1, 1]
        view[axes[bc]] = -1
        expected = torch.fft.ifft(spectrum * scale.reshape(view), dim=axes[bc]).real
        worst, bar = float((out[bc, 0].double() - expected).abs().max()), artefacts.FLOAT_BAR * float(expected.abs().max())
        print(f"[large] ghost_lines volume {bc}: max|d| = {worst:.3g} (bar {bar:.3g})")
        assert worst <= bar, (bc, worst, bar)
        del spectrum, expected
    del out
    peaks = (torch.arange(batch, device="cuda").float() + 1.0) * 1.0e6
    triples = [[(b % 7, (2 * b) % 11, (3 * b) % 13), (1, 0, 2)] for b in range(batch)]
    intensities = [0.5 + 0.1 * b for b in range(batch)]
    out = hip.add_spikes(data, triples, intensities, peaks)
    for b in range(batch):
        part = hip.add_spikes(data[b : b + 1], triples[b], intensities[b], peaks[b : b + 1])
        assert big.same(out[b : b + 1], part), f"add_spikes, element {b}: {big.first_difference(out[b : b + 1], part)}"
    i, j, k = (torch.arange(n, device="cuda", dtype=torch.float64) for n in shape[2:])
    for bc in big.crossing_slices(shape, torch.float32):
        waves = torch.zeros(shape[2:], dtype=torch.float64, device="cuda")
        for fi, fj, fk in triples[bc]:
            phase = 2 * math.pi * ((fi * i / shape[2])[:, None, None] + (fj * j / shape[3])[None, :, None] + (fk * k / shape[4])[None, None, :])
            waves += torch.cos(phase)
        expected = data[bc, 0].double() + float(peaks[bc]) * float(np.float32(intensities[bc])) / math.prod(shape[2:]) * waves
        worst, bar = float((out[bc, 0].double() - expected).abs().max()), artefacts.FLOAT_BAR * float(expected.abs().max())
        print(f"[large] add_spikes volume {bc}: max|d| = {worst:.3g} (bar {bar:.3g})")
        assert worst <= bar, (bc, worst, bar)
        del waves, expected
