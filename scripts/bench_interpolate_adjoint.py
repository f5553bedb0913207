"""Time the data-gradient passes of Resize, Anisotropy, the non-constant Pad modes, Ghosting and Motion next to their forwards.

    python scripts/bench_interpolate_adjoint.py [--size 256] [--batch 8] [--rounds 5] [--iters 5] [--json profiles/interpolate_adjoint_bench.json]

Whole engine calls (``ops.Engine`` methods: allocation of the result, uploads and - for the per-instance Anisotropy adjoint - the
inversion of the tables included) on ``batch x 1 x size^3`` float32, device time from events around ``iters`` calls enqueued back
to back; the rounds alternate the rows and each row reports the median and the spread.  ``copy`` is a plain device-to-device copy
of one such volume batch, taken in the same rounds: the yardstick of a pass that reads and writes every byte once.

    resize_up / resize_down     interpolate3d size/2 -> size and size -> size/2 (trilinear), and the adjoint of each
    anisotropy                  axis_gather_lerp with per-element tables (factors 1.5 .. 3.3, every axis) and its adjoint
    pad_reflect                 pad3d size -> size + 16 (8 per side, reflect) and its adjoint
    ghosting                    ghost_lines (4 planes per element, per-element axes); its backward is the same call on the gradient
    motion                      kspace_segment_mix of three segments; its backward: the three launches on the gradient (autograd)

Reads nothing outside the repository.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402
from torchio_amd.transforms import anisotropy  # noqa: E402


def device_timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def summary(samples):
    ordered = sorted(samples)
    return {"median_ms": round(ordered[len(ordered) // 2], 4), "min_ms": round(ordered[0], 4), "max_ms": round(ordered[-1], 4)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--batch", type=int, default=8)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--iters", type=int, default=5)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    engine, device = ops.hip_engine(), "cuda"
    size, half, batch = args.size, args.size // 2, args.batch
    generator = torch.Generator(device=device).manual_seed(1)
    full = torch.randn((batch, 1, size, size, size), device=device, generator=generator)
    small = full[:, :, ::2, ::2, ::2].contiguous()
    padded = torch.randn((batch, 1, size + 16, size + 16, size + 16), device=device, generator=generator)
    target = torch.empty_like(full)

    rows = {"copy": lambda: target.copy_(full)}
    rows["resize_up forward"] = lambda: engine.interpolate3d(small, (size,) * 3, "linear")
    rows["resize_up adjoint"] = lambda: engine.interpolate3d_adjoint(full, (half,) * 3, "linear")
    rows["resize_down forward"] = lambda: engine.interpolate3d(full, (half,) * 3, "linear")
    rows["resize_down adjoint"] = lambda: engine.interpolate3d_adjoint(small, (size,) * 3, "linear")

    factors = torch.linspace(1.5, 3.3, batch, dtype=torch.float64)
    down_sizes = torch.round(size / factors).clamp_min(1).to(torch.long)
    tables = [t.to(device) for t in anisotropy._linear_source_indices(size, down_sizes)]
    for axis in range(3):
        rows[f"anisotropy axis {axis} forward"] = lambda axis=axis: engine.axis_gather_lerp(full, axis, *tables)
        rows[f"anisotropy axis {axis} adjoint"] = lambda axis=axis: engine.axis_gather_lerp_adjoint(full, axis, *tables)

    padding = (8,) * 6
    rows["pad_reflect forward"] = lambda: engine.pad3d(full, padding, "reflect")
    rows["pad_reflect adjoint"] = lambda: engine.pad3d_adjoint(padded, (size,) * 3, padding, "reflect")

    ghost_axes = [b % 3 for b in range(batch)]
    ghost_lists = [[(f * size) // 4 for f in range(4)]] * batch
    rows["ghosting forward (= backward)"] = lambda: engine.ghost_lines(full, ghost_axes, 0.7, ghost_lists)

    third = size // 3
    bounds = [0, third, 2 * third, size]
    moved = [full.roll(1, 3), full.roll(2, 4)]
    rows["motion forward"] = lambda: engine.kspace_segment_mix([full, *moved], bounds, torch.float32)
    leaves = [t.clone().requires_grad_(True) for t in (full, *moved)]
    recorded = engine.kspace_segment_mix(leaves, bounds, torch.float32)
    rows["motion backward (every segment a leaf)"] = lambda: torch.autograd.grad(recorded, leaves, target, retain_graph=True)

    samples = {name: [] for name in rows}
    for name, row in rows.items():  # warm-up: first-use allocations, table uploads
        row()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, row in rows.items():
            samples[name].append(device_timed(row, args.iters))
    result = {
        "device": torch.cuda.get_device_name(0), "batch": batch, "size": size, "dtype": "float32", "rounds": args.rounds, "iters": args.iters,
        "bytes_copy": 2 * full.numel() * 4, "rows": {name: summary(values) for name, values in samples.items()},
    }
    copy_ms = result["rows"]["copy"]["median_ms"]
    for name, row in result["rows"].items():
        row["copies"] = round(row["median_ms"] / copy_ms, 2)
        print(f"{name:36s} {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f} .. {row['max_ms']:.3f}]  {row['copies']:6.2f} x copy")
    if args.json:
        with open(args.json, "w", encoding="utf-8") as file:
            json.dump(result, file, indent=1)
            file.write("\n")


if __name__ == "__main__":
    main()
