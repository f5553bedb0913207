"""Time the two PCA kernels and the whole ``tio.PCA`` call against the reference's op sequence on stock ATen, on the same GPU.

    python scripts/bench_pca.py [--rounds 3] [--iters 10] [--json out.json]

Per shape (float32, one element: ``16 x 128^3`` and ``64 x 64^3``) one process measures, ALTERNATING round by round (other
people's work shares the machine; a difference only counts inside one round):
``scatter``    one ``Engine.channel_scatter`` (``tio_channel_scatter``: the accumulating launch and the small finishing one);
``project``    one ``Engine.channel_project`` to three components with the clamp (``tio_channel_project``);
``clone``      ``clone`` of the input: the device-to-device copy rate of this box in this session (reads and writes every byte);
``tio.PCA``    the whole transform on a device batch, host clock around it, device synchronised before and after;
``ATen``       pca.py:83-140 op for op on device tensors (``torch.pca_lowrank`` included), the same clock.
Kernel samples are the device time per call of ``iters`` calls enqueued back to back (events); a row holds the median over the
rounds and the spread.  Further scatter-only rows walk the channel count from the memory-bound to the matrix-bound side:
per voxel the pass reads ``4 C`` bytes and does ``T (T + 1) / 2 x 512`` float64 FLOP, ``T = ceil(C / 16)``.
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

import torchio_amd as tio  # noqa: E402
from torchio_amd import ops  # noqa: E402


def device_timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def host_timed(fn):
    torch.cuda.synchronize()
    begin = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) * 1e3


def reference_sequence(tensor, num_components=3, values_range=(-2.3, 2.3)):
    """``PCA._pca_single`` with its defaults (whiten, normalize, clip) on a ``(C, I, J, K)`` device tensor."""
    c, si, sj, sk = tensor.shape
    flat = tensor.float().reshape(c, -1).t()  # the view einops makes of "c i j k -> (i j k) c"
    mean = flat.mean(dim=0, keepdim=True)
    centered = flat - mean
    _u, s, v = torch.pca_lowrank(centered, q=num_components)
    projected = centered @ v
    n = flat.shape[0]
    std = (s / ((n - 1) ** 0.5 if n > 1 else 1.0)).clamp(min=1e-8)
    projected = projected / std.unsqueeze(0)
    first_std = projected[:, 0].std().clamp(min=1e-8)
    projected = projected / first_std
    lo, hi = values_range
    projected = ((projected - lo) / (hi - lo)).clamp(0, 1)
    return torch.stack([projected.t().reshape(num_components, si, sj, sk)])


def summary(samples):
    ordered = sorted(samples)
    return {"median_ms": round(ordered[len(ordered) // 2], 4), "min_ms": round(ordered[0], 4), "max_ms": round(ordered[-1], 4)}


def element(channels, size, seed):
    generator = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(channels, channels, device="cuda", generator=generator) / channels**0.5
    data = torch.randn(channels, size**3, device="cuda", generator=generator)
    return (mix @ data + torch.randn(channels, 1, device="cuda", generator=generator)).reshape(1, channels, size, size, size)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca.py measures on the GPU; there is none")
    engine = ops.engine()
    rows = []
    for channels, size in ((16, 128), (64, 64)):
        data = element(channels, size, channels)
        batch = tio.SubjectsBatch.from_subjects([tio.Subject(emb=tio.ScalarImage(data[0]))])
        transform = tio.PCA(num_components=3)
        center = torch.zeros(1, channels, device="cuda")
        weights = torch.randn(1, 3, channels, device="cuda")
        offset = torch.full((1, 3), 0.5, device="cuda")
        kernels = {
            "scatter": lambda: engine.channel_scatter(data),  # noqa: B023
            "project": lambda: engine.channel_project(data, center, weights, offset, clip=True),  # noqa: B023
            "clone": lambda: data.clone(),  # noqa: B023
        }
        calls = {
            "tio_pca": lambda: transform(batch).images["emb"].data,  # noqa: B023
            "aten": lambda: reference_sequence(data[0]),  # noqa: B023
        }
        ours, theirs = calls["tio_pca"]().double(), calls["aten"]().double()
        deviation = torch.minimum((ours - theirs).abs(), (ours - (1 - theirs)).abs()).amax(dim=(0, 2, 3, 4))  # up to the sign of each axis
        for fn in (*kernels.values(), *calls.values()):
            fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in (*kernels, *calls)}
        for _ in range(args.rounds):
            for name, fn in kernels.items():
                samples[name].append(device_timed(fn, args.iters))
            for name, fn in calls.items():
                samples[name].append(host_timed(fn))
        row = {"shape": [channels, size, size, size], "input_mb": round(data.numel() * 4 / 1e6, 1)}
        row.update({name: summary(values) for name, values in samples.items()})
        in_bytes, out_bytes = data.numel() * 4, 3 * size**3 * 4
        row["scatter_gb_per_s"] = round(in_bytes / row["scatter"]["median_ms"] / 1e6, 1)
        row["project_gb_per_s"] = round((in_bytes + out_bytes) / row["project"]["median_ms"] / 1e6, 1)
        row["clone_gb_per_s"] = round(2 * in_bytes / row["clone"]["median_ms"] / 1e6, 1)
        row["aten_over_tio_pca"] = round(row["aten"]["median_ms"] / row["tio_pca"]["median_ms"], 2)
        row["tio_pca_vs_aten_max_abs_per_component"] = [float(f"{v:.3e}") for v in deviation.tolist()]
        rows.append(row)
        del data, batch
        torch.cuda.empty_cache()
    rates = []
    for channels, size in ((16, 128), (32, 128), (48, 128), (64, 64), (128, 64), (256, 64), (1024, 32)):
        data = element(channels, size, channels)
        engine.channel_scatter(data)
        torch.cuda.synchronize()
        ms = summary([device_timed(lambda: engine.channel_scatter(data), args.iters) for _ in range(args.rounds)])  # noqa: B023
        tiles = (channels + 15) // 16
        flop = tiles * (tiles + 1) // 2 * 512 * size**3
        rates.append({"shape": [channels, size, size, size], **ms, "gb_per_s": round(data.numel() * 4 / ms["median_ms"] / 1e6, 1),
                      "f64_tflop_per_s": round(flop / ms["median_ms"] / 1e9, 2)})
        del data
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "rows": rows, "scatter_rates": rates}
    print("| C x size^3 | scatter ms | GB/s | project ms | GB/s | clone ms | GB/s | tio.PCA ms (min .. max) | ATen ms (min .. max) | ATen / tio.PCA |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['shape'][0]} x {r['shape'][1]}^3 | {r['scatter']['median_ms']} | {r['scatter_gb_per_s']} | {r['project']['median_ms']} | "
              f"{r['project_gb_per_s']} | {r['clone']['median_ms']} | {r['clone_gb_per_s']} | {r['tio_pca']['median_ms']} ({r['tio_pca']['min_ms']} .. "
              f"{r['tio_pca']['max_ms']}) | {r['aten']['median_ms']} ({r['aten']['min_ms']} .. {r['aten']['max_ms']}) | {r['aten_over_tio_pca']} |")
    print("| C x size^3 | scatter ms (min .. max) | GB/s | float64 TFLOP/s |")
    print("|---|---|---|---|")
    for r in rates:
        print(f"| {r['shape'][0]} x {r['shape'][1]}^3 | {r['median_ms']} ({r['min_ms']} .. {r['max_ms']}) | {r['gb_per_s']} | {r['f64_tflop_per_s']} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
