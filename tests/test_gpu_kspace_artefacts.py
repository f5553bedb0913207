"""GPU: ``tio_kspace_ghost_lines``, ``tio_complex_abs_max``, ``tio_kspace_add_spikes`` and the two classes against the float64
FFT-route restatements of ``kspace_artefact_cases.py`` (which the host tests hold against the reference's own outputs) and
the golden file.

Bars (``cases.check``): float dtypes ``|d| <= 1e-5 * max|expected|`` — the bar of the same kind of float32 sums in
``test_kspace_segment_mix_matches_the_fft_route``; the reference itself sits at 3e-7 of it on these cases — plus half an ulp
of the storage type for float16 / bfloat16; integer dtypes ``|d| <= 1`` on at most a share ``2e-5 * max|expected|`` of the
voxels.  Inactive elements are bit-identical to the input.

Shapes: the issue's six, each with every axis; and axis lengths past each LDS layout of the ghost kernel (``LDS_LIMITS``).
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import kspace_artefact_cases as cases
import torchio_amd as tio
from torchio_amd import ops
from torchio_amd.transforms import ghosting

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kspace_artefacts_golden.pt")
#: axis lengths just past what each layout of ghost_lines_kernel holds in 156 KiB of LDS (csrc/kspace_artefacts.hip):
#: 549 — input and accumulator tiles of 32 lines (more than 8 frequencies); 1067 — one tile of 32 lines; 3397 — an
#: accumulator tile of 8 lines, the input read from memory; beyond, one line per tile (up to 9344)
LDS_LIMITS = (549, 1067, 3397)
LONG_SHAPES = [(1, 1, *np.roll((limit + 3, 2, 3), shift).tolist()) for limit in LDS_LIMITS for shift in range(3)]
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


def _frequency_lists(size: int) -> dict[str, list[int]]:
    """|Z| of 1, about 4 (the default's planes), 12 where the axis has them (two chunks of the kernel), and ``size``."""
    lists = {"one": [size // 3], "default": ghosting.ghost_frequencies(size, 4, 0.0), "all": list(range(size))}
    if size >= 12:
        lists["twelve"] = ghosting.ghost_frequencies(size, 12, 0.0)[:12]
    return lists


# -- Ghosting: the engine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", cases.AXES)
@pytest.mark.parametrize("shape", cases.SHAPES + LONG_SHAPES, ids=ids)
def test_ghost_lines_match_the_fft_route(hip, shape, axis):
    data = cases.signed_image(tuple(shape), 5)
    on_device = data.cuda()
    before = on_device.clone()
    size = shape[2 + axis]
    for label, frequencies in _frequency_lists(size).items():
        out = hip.ghost_lines(on_device, axis, 0.7, frequencies)
        assert out.dtype == data.dtype and out.shape == data.shape and torch.equal(on_device, before)
        expected = cases.ghost_fft(data, [axis] * shape[0], [cases.mask_from_frequencies(size, frequencies, 0.7)] * shape[0])
        cases.check(out, expected, f"ghost {ids(shape)} axis {axis} |Z| {label}")


def test_ghost_lines_per_element_axes_and_inactive_elements(hip):
    shape = (4, 2, 12, 9, 7)
    data = cases.signed_image(shape, 6)
    axes, strengths = [2, 0, 1, 1], [0.9, 0.5, 0.3, 0.6]
    lists = [[1, 3], [0, 5, 11], list(range(9)), []]
    active = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
    out = hip.ghost_lines(data.cuda(), axes, strengths, lists, active.cuda())
    masks = [cases.mask_from_frequencies(shape[2 + a], f, s) for a, f, s in zip(axes, lists, strengths, strict=True)]
    masks[1] = masks[3] = None
    cases.check(out, cases.ghost_fft(data, axes, masks), "ghost mixed axes")
    assert torch.equal(out[1].cpu(), data[1]) and torch.equal(out[3].cpu(), data[3])  # inactive / empty list: the input's bits
    again = hip.ghost_lines(data.cuda(), axes, strengths, lists, active.bool().cuda())
    assert torch.equal(again, out)
    everything = hip.ghost_lines(data.cuda(), axes, strengths, lists)  # no flags: all active
    masks[1] = cases.mask_from_frequencies(12, lists[1], 0.5)
    cases.check(everything, cases.ghost_fft(data, axes, masks), "ghost mixed axes, all active")


@pytest.mark.parametrize("axis", cases.AXES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16, torch.int16, torch.uint8], ids=str)
def test_ghost_lines_dtypes(hip, dtype, axis):
    shape = (2, 1, *cases.INTEGER_SHAPE)
    data = cases.typed_positive(shape, dtype, 7)
    size = shape[2 + axis]
    frequencies = ghosting.ghost_frequencies(size, 4, 0.0)
    out = hip.ghost_lines(data.cuda(), axis, [0.05, 0.05], frequencies, torch.tensor([True, False]).cuda())
    assert out.dtype == dtype
    expected = cases.ghost_fft(data, [axis, axis], [cases.mask_from_frequencies(size, frequencies, 0.05), None])
    cases.check(out[:1], expected[:1], f"ghost {dtype} axis {axis}")
    assert torch.equal(out[1].cpu(), data[1])  # float64 keeps the bits float32 would drop


def test_ghost_lines_empty_batch_and_too_long_an_axis(hip):
    empty = hip.ghost_lines(torch.empty(0, 2, 3, 4, 5, device="cuda"), 0, 0.5, [1])
    assert empty.shape == (0, 2, 3, 4, 5)
    with pytest.raises(ops.EngineError, match="status -5.*an axis of 9400 voxels does not fit"):
        hip.ghost_lines(torch.zeros(1, 1, 9400, 1, 1, device="cuda"), 0, 0.5, [1])


def test_ghost_lines_full_size(hip):
    """One 256^3 float32 volume: per axis a block of 8 x 8 lines against a float64 FFT along that axis; zero strength
    returns the input exactly."""
    data = torch.randn(1, 1, 256, 256, 256, device="cuda", generator=torch.Generator("cuda").manual_seed(8)) * 40 + 100
    frequencies = ghosting.ghost_frequencies(256, 4, 0.0)
    assert frequencies == [128, 192, 0, 64]
    for axis in cases.AXES:
        out = hip.ghost_lines(data, axis, 0.6, frequencies)
        window = [slice(100, 108), slice(37, 45), slice(201, 209)]
        window[axis] = slice(None)
        lines = np.moveaxis(data[0, 0][tuple(window)].cpu().double().numpy(), axis, -1)
        spectrum = np.fft.fft(lines, axis=-1)
        spectrum[..., frequencies] *= 1.0 - 0.6
        expected = np.moveaxis(np.fft.ifft(spectrum, axis=-1).real, -1, axis)
        cases.check(out[0, 0][tuple(window)], expected, f"ghost 256^3 axis {axis}")
        assert torch.equal(hip.ghost_lines(data, axis, 0.0, frequencies), data)


# -- Spike: the engine ---------------------------------------------------------------------------------------------------
def _random_indices(shape, count: int, seed: int):
    generator = torch.Generator().manual_seed(seed)
    return [tuple(int(torch.randint(s, (1,), generator=generator)) for s in shape) for _ in range(count)]


def _check_spikes(hip, data, index_lists, intensities, active=None, what=""):
    shape = tuple(data.shape[2:])
    on_device = data.cuda()
    before = on_device.clone()
    peaks = hip.spectrum_peak(on_device)
    quiet = [i if active is None or active[b] else 0.0 for b, i in enumerate(intensities)]
    expected, true_peaks = cases.spike_fft(data, index_lists, quiet)
    assert peaks.dtype == torch.float32 and peaks.shape == (data.shape[0] * data.shape[1],)
    assert np.abs(peaks.cpu().double().numpy() - true_peaks.reshape(-1)).max() <= 1e-5 * true_peaks.max()
    flags = None if active is None else torch.tensor(active, dtype=torch.uint8).cuda()
    out = hip.add_spikes(on_device, [cases.unshifted(indices, shape) for indices in index_lists], intensities, peaks, flags)
    assert out.dtype == data.dtype and torch.equal(on_device, before)
    cases.check(out, expected, what)
    return out


@pytest.mark.parametrize("kind", ["signed", "positive"])
@pytest.mark.parametrize("shape", cases.SHAPES, ids=ids)
def test_add_spikes_match_the_fft_route(hip, shape, kind):
    data = cases.signed_image(tuple(shape), 9) if kind == "signed" else cases.positive_image(tuple(shape), 9)
    batch, spatial = shape[0], shape[2:]
    for count in (1, 6):
        for sign in (1.0, -1.0):
            lists = [_random_indices(spatial, count, 10 * b + count) for b in range(batch)]
            if count == 6:
                lists = [entries[:5] + entries[:1] for entries in lists]  # a duplicate counts twice
            intensities = [sign * (1.5 - 0.4 * b) for b in range(batch)]
            _check_spikes(hip, data, lists, intensities, what=f"spike {ids(shape)} {kind} {count} x {sign}")
    shared = _random_indices(spatial, 2, 3)  # one list, one intensity for the whole batch
    out = hip.add_spikes(data.cuda(), cases.unshifted(shared, spatial), 0.8, hip.spectrum_peak(data.cuda()))
    cases.check(out, cases.spike_fft(data, [shared] * batch, [0.8] * batch)[0], f"spike {ids(shape)} {kind} shared")


def test_add_spikes_inactive_elements_are_the_input(hip):
    shape = (4, 2, 12, 9, 7)
    data = cases.signed_image(shape, 11)
    lists = [_random_indices(shape[2:], 3, 1), _random_indices(shape[2:], 2, 2), [], _random_indices(shape[2:], 1, 4)]
    out = _check_spikes(hip, data, lists, [1.2, 0.9, 2.0, 0.0], active=[1, 0, 1, 1], what="spike mixed")
    for b in (1, 2, 3):  # flagged off, no spike, zero intensity
        assert torch.equal(out[b].cpu(), data[b])
    assert not torch.equal(out[0].cpu(), data[0])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16, torch.int16, torch.uint8], ids=str)
def test_add_spikes_dtypes(hip, dtype):
    shape = (2, 1, *cases.INTEGER_SHAPE)
    data = cases.typed_positive(shape, dtype, 12)
    lists = [_random_indices(shape[2:], 2, 5), _random_indices(shape[2:], 2, 6)]
    out = _check_spikes(hip, data, lists, [0.05, -0.05], active=[1, 0], what=f"spike {dtype}")
    assert out.dtype == dtype and torch.equal(out[1].cpu(), data[1])
    _check_spikes(hip, data[:1], lists[:1], [-0.05], what=f"spike {dtype} negative")


def test_add_spikes_empty_batch(hip):
    data = torch.empty(0, 2, 3, 4, 5, device="cuda")
    peaks = hip.spectrum_peak(data)
    assert peaks.shape == (0,) and hip.add_spikes(data, [(0, 0, 0)], 1.0, peaks).shape == (0, 2, 3, 4, 5)


def test_add_spikes_full_size(hip):
    """One 256^3 float32 volume, non-negative: the peak is the sum of the voxels (1e-5 relative), a sub-block against the
    closed form."""
    data = torch.rand(1, 1, 256, 256, 256, device="cuda", generator=torch.Generator("cuda").manual_seed(13)) * 180 + 20
    peaks = hip.spectrum_peak(data)
    total = float(data.double().sum())
    assert abs(float(peaks[0]) - total) <= 1e-5 * total
    triples = [(3, 250, 17), (128, 0, 1)]
    out = hip.add_spikes(data, triples, 0.4, peaks)
    window = (slice(96, 112), slice(0, 9), slice(243, 256))
    grids = np.meshgrid(*(np.arange(256)[w] for w in window), indexing="ij")
    waves = sum(np.cos(2 * np.pi * sum(f * g / 256 for f, g in zip(triple, grids, strict=True))) for triple in triples)
    expected = data[0, 0][window].cpu().double().numpy() + total * 0.4 / 256**3 * waves
    cases.check(out[0, 0][window], expected, "spike 256^3")


# -- the peak on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_complex_abs_max(hip, n):
    """Against ``torch.abs(z).amax``: 2 float32 ulp, ``sqrt(re^2 + im^2)`` against ``hypot``.  Odd ``n``: every other row starts
    in the middle of a 16-byte line."""
    generator = torch.Generator().manual_seed(n)
    z = torch.complex(torch.randn(5, n, generator=generator), torch.randn(5, n, generator=generator)) * 1000.0
    z[3] *= 1e-3
    got = hip.complex_abs_max(z.cuda()).cpu()
    expected = torch.abs(z).amax(1)
    assert got.dtype == torch.float32 and got.shape == (5,)
    ulps = (got.double() - expected.double()).abs().numpy() / np.spacing(expected.numpy()).astype(np.float64)
    print(f"n = {n}: worst {ulps.max():.2f} ulp")
    assert ulps.max() <= 2
    assert hip.complex_abs_max(torch.zeros(3, 0, dtype=torch.complex64, device="cuda")).tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="complex_abs_max: expected a complex64"):
        hip.complex_abs_max(z.cuda().to(torch.complex128))


# -- the classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CASES)
def test_transforms_reproduce_the_reference(golden, name):
    """The whole call on a device batch: the reference's recorded parameters, history and warnings; the output within the
    bars of the float64 restatement AND of the reference's own output."""
    out, params, history_name, built, messages = cases.run_case(tio, name, "cuda")
    entry = golden[name]
    assert (params, history_name, built, messages) == (entry["params"], entry["name"], entry["built"], entry["warnings"])
    assert out.device.type == "cuda" and out.dtype == entry["out"].dtype
    cases.check(out, cases.expected_for(name, params), f"{name} against the restatement")
    cases.check(out, entry["out"].double().numpy(), f"{name} against the reference")
    if "_keep" in params:
        image = cases.case_input(name)
        for b, keep in enumerate(params["_keep"]):
            assert keep or torch.equal(out[b].cpu(), image[b])


def test_transforms_on_host_subjects_and_in_a_compose(golden):
    """A host-resident subject is staged on the device and comes back; both classes compose with the others."""
    image = cases.case_input("spike_shared")[0]
    torch.manual_seed(3)
    out = tio.Compose([tio.Ghosting(intensity=0.5, axes=(1,)), tio.Spike(intensity=1.0)])(tio.Subject(t1=tio.ScalarImage(image.clone())))
    assert out["t1"].data.device.type == "cpu" and [record.name for record in out.applied_transforms][-2:] == ["Ghosting", "Spike"]
    ghost, spikes = out.applied_transforms[-2].params, out.applied_transforms[-1].params
    after_ghost = cases.ghost_expected_from_params(image[None], ghost)
    expected = cases.spike_expected_from_params(torch.from_numpy(after_ghost).float(), spikes)
    cases.check(out["t1"].data[None], expected, "Compose[Ghosting, Spike]")
