"""Time LabelsToImage on the engine against the reference's operation sequence on ATen, on the same GPU.

    python scripts/bench_labels_to_image.py [--reps 10] [--size 256] [--json out.json]

Label maps: 8 x 1 x size^3, int16 and uint8, with 4 and with 32 labels, as blocks of 8^3 voxels of one label (a
segmentation) and as one random label per voxel (the worst case for the table lookups).  Rows, per case:
``fused``      ``Engine.labels_to_image(..., seed=...)``: the median of whole calls, each ended by a synchronise, its one
               packed parameter upload included; and the device time per call of 20 calls enqueued back to back;
``one label``  one launch of the parity road (``base=``, ``base_key=``) with the draws at hand — the reference-identical
               mode makes one per label, after a host draw and an upload of the volume that are not timed here;
``ATen``       labels_to_image.py:263-290 restated with torch ops on the device: per label ``randn_like``, ``* std``,
               ``+ mean``, ``==``, ``.float()``, ``*``, ``+=`` (device draws: the reference's CPU generator is not the point);
``draws``      ``Engine.philox_normal`` of the output's shape alone: the arithmetic of the draws with 4 bytes per voxel written;
``copy``       a plain device-to-device copy that moves the same bytes as the fused pass (it reads the label and writes
               a float32 per voxel: 6 bytes for int16, 5 for uint8; the copy reads and writes half of that each).
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


def device_timed(fn, iters=20):
    """Device time per call of ``iters`` calls enqueued back to back (events): the host side of a call hides behind the
    previous call's kernel wherever the kernel is the longer of the two."""
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def aten_generate(labels, means, stds):
    """_generate_from_labels (labels_to_image.py:263-290) on the device."""
    result = torch.zeros(labels.shape[0], 1, *labels.shape[2:], device=labels.device)
    for value, mean in means.items():
        std = stds.get(value, 0.0)
        if mean == 0.0 and std == 0.0:
            continue
        mask = (labels[:, 0:1] == value).float()
        tissue = torch.randn_like(result) * std + mean
        result += tissue * mask
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    engine = ops.engine()
    size, batch = args.size, 8
    voxels = batch * size**3
    generator = torch.Generator("cuda").manual_seed(0)
    rows = []
    draws_ms = device_timed(lambda: engine.philox_normal((batch, 1, size, size, size), 1, 0, "cuda"))
    for dtype in (torch.int16, torch.uint8):
        element = torch.empty((), dtype=dtype).element_size()
        moved = voxels * (element + 4)
        source, target = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy_ms = timed(lambda: target.copy_(source), args.reps)  # noqa: B023
        del source, target
        for n_labels in (4, 32):
            keys = list(range(n_labels))
            means = {k: 0.1 + 0.8 * k / n_labels for k in keys}
            stds = {k: 0.01 + 0.09 * k / n_labels for k in keys}
            coarse = torch.randint(0, n_labels, (batch, 1, size // 8, size // 8, size // 8), device="cuda", generator=generator)
            blocks = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4).to(dtype)
            random = torch.randint(0, n_labels, (batch, 1, size, size, size), device="cuda", generator=generator).to(dtype)
            base = torch.randn(batch, 1, size, size, size, device="cuda", generator=generator)
            out = torch.zeros_like(base)
            aten_ms = timed(lambda: aten_generate(blocks, means, stds), max(3, args.reps // 3))  # noqa: B023
            for pattern, labels in (("blocks of 8^3", blocks), ("random per voxel", random)):
                device_ms = device_timed(lambda: engine.labels_to_image(labels, keys, list(means.values()), list(stds.values()), seed=1))  # noqa: B023
                fused_ms = timed(lambda: engine.labels_to_image(labels, keys, list(means.values()), list(stds.values()), seed=1), args.reps)  # noqa: B023
                one_ms = timed(lambda: engine.labels_to_image(labels, keys, list(means.values()), list(stds.values()), base=base, base_key=1, out=out),  # noqa: B023
                               args.reps)
                rows.append({
                    "dtype": str(dtype).replace("torch.", ""), "labels": n_labels, "pattern": pattern, "bytes_per_voxel": element + 4,
                    "fused_ms": round(fused_ms, 3), "fused_device_ms": round(device_ms, 3), "one_label_ms": round(one_ms, 3), "aten_ms": round(aten_ms, 3), "copy_ms": round(copy_ms, 3),
                    "speedup": round(aten_ms / fused_ms, 1), "times_the_copy": round(device_ms / copy_ms, 2),
                    "fused_gb_per_s": round(moved / device_ms / 1e6, 1),
                })
            del coarse, blocks, random, base, out
            torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "shape": [batch, 1, size, size, size], "philox_normal_device_ms": round(draws_ms, 3), "rows": rows}
    print(f"the draws alone (philox_normal of the output's shape, device time): {draws_ms:.3f} ms")
    print("| labels | dtype | pattern | bytes / voxel | fused call ms | fused device ms | GB/s (device) | copy of the same bytes ms | times the copy (device) | one label ms | ATen ms | speed-up (call) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['labels']} | {r['dtype']} | {r['pattern']} | {r['bytes_per_voxel']} | {r['fused_ms']} | {r['fused_device_ms']} | {r['fused_gb_per_s']} | {r['copy_ms']} | "
              f"{r['times_the_copy']} | {r['one_label_ms']} | {r['aten_ms']} | {r['speedup']} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
