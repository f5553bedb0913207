"""Time Ghosting and Spike on the engine against the reference's operation sequences on ATen, on the same GPU.

    python scripts/bench_kspace_artefacts.py [--reps 10] [--size 256] [--json out.json]

Input: 8 x 1 x size^3 float32.  Rows:
``Ghosting`` with the defaults (4 ghosts: 4 scaled planes), one set of parameters for the batch along each axis, and one set
per element with mixed axes; one case with ``num_ghosts >= size`` (every plane scaled) — ``Engine.ghost_lines`` against the
reference's sequence restated with torch ops on the device (ghosting.py:218-277 / :149-215: ``fftn``, ``fftshift``, the mask
product, ``ifftshift``, ``ifftn``, ``.real``, and ``where`` on the per-element path);
``Spike`` with one spike, on non-negative and on signed input, shared and per element — ``Engine.spectrum_peak`` +
``Engine.add_spikes`` against spike.py:124-162 / :165-223 (``fftn``, ``fftshift``, ``abs``, ``amax``, the point updates,
``ifftshift``, ``ifftn``, ``.real``); the synthesis pass (``add_spikes`` with the peaks at hand) is also timed alone.
Every row with its time over that of a plain device-to-device copy of the same tensor (``dst.copy_(src)``), and the largest
difference between the two routes over the largest value.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402
from torchio_amd.transforms.ghosting import ghost_frequencies  # noqa: E402
from torchio_amd.transforms.spike import spike_frequencies  # noqa: E402

DIMS = (-3, -2, -1)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(reps):
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - start) * 1e3)
    samples.sort()
    return samples[len(samples) // 2]  # the median


def line_mask(size, ghosts, strength, restore, device):
    mask = torch.ones(size, device=device)
    mask[:: max(size // ghosts, 1)] = 1 - strength
    if restore > 0:
        half = max(int(size * restore / 2), 1)
        mask[size // 2 - half : size // 2 + half] = 1
    return mask


def aten_ghost_shared(data, ghosts, axis, strength, restore):
    spectrum = torch.fft.fftshift(torch.fft.fftn(data.float(), dim=DIMS), dim=DIMS)
    view = [1] * 5
    view[axis + 2] = -1
    corrupted = spectrum * line_mask(data.shape[axis + 2], ghosts, strength, restore, data.device).view(view)
    return torch.fft.ifftn(torch.fft.ifftshift(corrupted, dim=DIMS), dim=DIMS).real.to(data.dtype)


def aten_ghost_per_element(data, ghosts, axes, strengths, restore):
    spectrum = torch.fft.fftshift(torch.fft.fftn(data.float(), dim=DIMS), dim=DIMS)
    mask = torch.ones(data.shape[0], 1, *data.shape[2:], device=data.device)
    for b, (n, axis, strength) in enumerate(zip(ghosts, axes, strengths, strict=True)):
        view = [1] * 4
        view[axis + 1] = -1
        mask[b] = line_mask(data.shape[axis + 2], n, strength, restore, data.device).view(view)
    result = torch.fft.ifftn(torch.fft.ifftshift(spectrum * mask, dim=DIMS), dim=DIMS).real.to(data.dtype)
    active = torch.ones(data.shape[0], dtype=torch.bool, device=data.device).view(-1, 1, 1, 1, 1)
    return torch.where(active, result, data)


def aten_spikes(data, positions, intensities):
    """One list of positions per element (the shared path passes the same list for each: the same launches per point)."""
    shape = data.shape[2:]
    spectrum = torch.fft.fftshift(torch.fft.fftn(data.float(), dim=DIMS), dim=DIMS)
    peak = spectrum.abs().amax(dim=DIMS, keepdim=True)
    for b, (entries, intensity) in enumerate(zip(positions, intensities, strict=True)):
        for position in entries:
            i, j, k = (int(p * s) % s for p, s in zip(position, shape, strict=True))
            spectrum[b, :, i, j, k] += peak[b, :, 0, 0, 0] * intensity
    return torch.fft.ifftn(torch.fft.ifftshift(spectrum, dim=DIMS), dim=DIMS).real.to(data.dtype)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    engine = ops.engine()
    size, batch = args.size, 8
    generator = torch.Generator("cuda").manual_seed(0)
    positive = torch.rand(batch, 1, size, size, size, device="cuda", generator=generator) * 180 + 20
    signed = torch.randn(batch, 1, size, size, size, device="cuda", generator=generator) * 40
    signed += 60 * torch.cos(2 * torch.pi * torch.arange(size, device="cuda") / size).view(-1, 1, 1)  # the peak is not the DC term
    target = torch.empty_like(positive)
    copy_ms = timed(lambda: target.copy_(positive), args.reps)
    del target
    shape = (size, size, size)
    rows = []

    def row(name, ours, theirs):
        ours_ms, theirs_ms = timed(ours, args.reps), (timed(theirs, max(3, args.reps // 3)) if theirs is not None else None)
        entry = {"row": name, "engine_ms": round(ours_ms, 3), "times_the_copy": round(ours_ms / copy_ms, 2)}
        if theirs is not None:
            a, b = ours(), theirs()
            entry.update(aten_ms=round(theirs_ms, 3), speedup=round(theirs_ms / ours_ms, 1),
                         max_difference=float((a - b).abs().max() / b.abs().max()))
            del a, b
        rows.append(entry)
        torch.cuda.empty_cache()

    strength, restore = 0.7, 0.0
    default = ghost_frequencies(size, 4, restore)
    for axis in range(3):
        row(f"Ghosting shared, axis {axis}, |Z| = {len(default)}", lambda axis=axis: engine.ghost_lines(positive, axis, strength, default),
            lambda axis=axis: aten_ghost_shared(positive, 4, axis, strength, restore))
    axes = [b % 3 for b in range(batch)]
    strengths = [0.5 + 0.05 * b for b in range(batch)]
    row("Ghosting per element, mixed axes", lambda: engine.ghost_lines(positive, axes, strengths, [default] * batch),
        lambda: aten_ghost_per_element(positive, [4] * batch, axes, strengths, restore))
    every = ghost_frequencies(size, size + 50, restore)
    for axis in (0, 2):
        row(f"Ghosting shared, axis {axis}, num_ghosts >= S: |Z| = {len(every)}", lambda axis=axis: engine.ghost_lines(positive, axis, strength, every),
            lambda axis=axis: aten_ghost_shared(positive, size + 50, axis, strength, restore))

    torch.manual_seed(1)
    one = torch.rand(1, 3).tolist()
    each = [torch.rand(1, 3).tolist() for _ in range(batch)]
    intensities = [1.0 + 0.1 * b for b in range(batch)]
    for label, data in (("non-negative", positive), ("signed", signed)):
        row(f"Spike shared, {label}", lambda data=data: engine.add_spikes(data, spike_frequencies(one, shape), 1.5, engine.spectrum_peak(data)),
            lambda data=data: aten_spikes(data, [one] * batch, [1.5] * batch))
        row(f"Spike per element, {label}",
            lambda data=data: engine.add_spikes(data, [spike_frequencies(p, shape) for p in each], intensities, engine.spectrum_peak(data)),
            lambda data=data: aten_spikes(data, each, intensities))
    peaks = engine.spectrum_peak(positive)
    row("Spike: the peak alone (rfftn + tio_complex_abs_max)", lambda: engine.spectrum_peak(positive), None)
    row("Spike: the synthesis alone (tio_kspace_add_spikes)", lambda: engine.add_spikes(positive, spike_frequencies(one, shape), 1.5, peaks), None)

    result = {"device": torch.cuda.get_device_name(0), "shape": list(positive.shape), "copy_ms": round(copy_ms, 3), "rows": rows}
    print(f"device-to-device copy of the tensor: {copy_ms:.3f} ms")
    print("| row | engine ms | ATen ms | speed-up | times the copy | max difference |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['row']} | {r['engine_ms']} | {r.get('aten_ms', '')} | {r.get('speedup', '')} | {r['times_the_copy']} | {r.get('max_difference', '')} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
