"""Time Swap and HistogramStandardization on the engine against the reference's operation sequences on ATen, on the same GPU.

    python scripts/bench_swap_histogram.py [--reps 20] [--size 256] [--json out.json]

Input: 8 x 1 x size^3 float32 white noise.  Rows:
``Swap`` with patch 15 and 100 iterations, one list for the batch and one list per element — ``Engine.swap_patches`` against
the reference's loop restated with torch ops on the device (swap.py:195-219: two clones and two slice assignments per swap;
:222-258: two advanced-indexing gathers and two scatters per swap);
``HistogramStandardization`` with the 13 default percentiles — ``Engine.histogram_standardize`` against the reference's lines
(histogram_standardization.py:276-303) per element: a copy to the host, ``np.percentile``, then ``diff`` / ``bucketize`` / gather
on the device.
Each with the bytes the engine's launches move at least (Swap: the copy reads and writes the batch, the gather reads and
writes the box voxels; the standardization reads the batch five times — four selection passes and the map — and writes it once) and that volume's share of the
device-to-device copy rate (``dst.copy_(src)`` of a 1 GiB buffer, read + written).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402
from torchio_amd.transforms.histogram_standardization import _build_quantiles  # noqa: E402
from torchio_amd.transforms.swap import _sample_swap_locations  # noqa: E402


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


def aten_swap_shared(data, locations, patch):
    result = data.clone()
    pi, pj, pk = patch
    for (ai, aj, ak), (bi, bj, bk) in locations:
        first = result[:, :, ai : ai + pi, aj : aj + pj, ak : ak + pk].clone()
        second = result[:, :, bi : bi + pi, bj : bj + pj, bk : bk + pk].clone()
        result[:, :, ai : ai + pi, aj : aj + pj, ak : ak + pk] = second
        result[:, :, bi : bi + pi, bj : bj + pj, bk : bk + pk] = first
    return result


def aten_swap_per_instance(data, locations, patch):
    result = data.clone()
    batch, channels = data.shape[:2]
    device = data.device
    count = max(len(entries) for entries in locations)
    origins = torch.zeros(batch, count, 2, 3, dtype=torch.long)
    for b, entries in enumerate(locations):
        if entries:
            origins[b, : len(entries)] = torch.tensor(entries)
    origins = origins.to(device)
    b_index = torch.arange(batch, device=device).view(-1, 1, 1, 1, 1)
    c_index = torch.arange(channels, device=device).view(1, -1, 1, 1, 1)
    offsets = [torch.arange(p, device=device).view([1, 1] + [-1 if axis == d else 1 for axis in range(3)]) for d, p in enumerate(patch)]
    for s in range(count):
        index = []
        for which in range(2):
            at = [origins[:, s, which, d].view(-1, 1, 1, 1, 1) + offsets[d] for d in range(3)]
            index.append((b_index, c_index, *at))
        first, second = result[index[0]].clone(), result[index[1]].clone()
        result[index[0]] = second
        result[index[1]] = first
    return result


def aten_standardize(data, landmarks, quantiles):
    out = torch.empty_like(data)
    percentiles = [100.0 * q for q in quantiles]
    for b in range(data.shape[0]):
        flat = data[b].float().reshape(-1)
        found = torch.as_tensor(np.percentile(flat.cpu().numpy(), percentiles), dtype=torch.float32, device=data.device)
        widths = torch.diff(found)
        widths = torch.where(widths.abs() < 1e-5, torch.tensor(float("inf"), device=data.device), widths)
        slopes = torch.diff(landmarks) / widths
        intercepts = landmarks[:-1] - slopes * found[:-1]
        bins = torch.bucketize(flat, found[1:-1], right=False)
        out[b] = (slopes[bins] * flat + intercepts[bins]).reshape(data[b].shape)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    engine = ops.engine()
    size, batch, patch, iterations = args.size, 8, (15, 15, 15), 100
    data = torch.randn(batch, 1, size, size, size, device="cuda") * 40 + 20
    gib = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    target = torch.empty_like(gib)
    copy_gbps = 2 * gib.numel() * 4 / (timed(lambda: target.copy_(gib), args.reps) * 1e-3) / 1e9
    del gib, target
    torch.manual_seed(0)
    shared = _sample_swap_locations((size, size, size), patch, iterations)
    per_instance = [_sample_swap_locations((size, size, size), patch, iterations) for _ in range(batch)]
    quantiles = _build_quantiles((0.01, 0.99))
    landmarks = torch.linspace(0, 100, len(quantiles), device="cuda")
    batch_bytes = data.numel() * 4
    box_bytes = 2 * iterations * 15**3 * batch * 4
    rows = []

    def row(name, ours, theirs, moved):
        ours_ms, theirs_ms = timed(ours, args.reps), timed(theirs, max(3, args.reps // 4))
        same = torch.equal(ours(), theirs())
        achieved = moved / (ours_ms * 1e-3) / 1e9
        rows.append({"row": name, "engine_ms": round(ours_ms, 3), "aten_ms": round(theirs_ms, 3), "speedup": round(theirs_ms / ours_ms, 1),
                     "bytes_moved": moved, "GBps": round(achieved, 1), "share_of_copy_rate": round(achieved / copy_gbps, 3), "same_bits": same})

    row("Swap shared", lambda: engine.swap_patches(data, shared, patch), lambda: aten_swap_shared(data, shared, patch), 2 * batch_bytes + 2 * box_bytes)
    row("Swap per-instance", lambda: engine.swap_patches(data, per_instance, patch), lambda: aten_swap_per_instance(data, per_instance, patch),
        2 * batch_bytes + 2 * box_bytes)
    row("HistogramStandardization", lambda: engine.histogram_standardize(data, landmarks, quantiles), lambda: aten_standardize(data, landmarks, quantiles),
        6 * batch_bytes)
    result = {"device": torch.cuda.get_device_name(0), "shape": list(data.shape), "copy_GBps": round(copy_gbps, 1), "rows": rows}
    print("| row | engine ms | ATen ms | speed-up | bytes moved | GB/s | share of copy rate | same bits |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['row']} | {r['engine_ms']} | {r['aten_ms']} | {r['speedup']}x | {r['bytes_moved']} | {r['GBps']} | {r['share_of_copy_rate']} | {r['same_bits']} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
