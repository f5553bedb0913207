"""Time one batch of weighted patches through the three roads of the patch feed, on one GPU, in one process.

    python scripts/bench_patch_feed.py [--size 256] [--patch 64] [--patches 16] [--rounds 3] [--iters 20] [--json out.json]

Workload: ``LabelSampler`` (two labels, weights 0.25 / 0.75), ``patches`` patches of ``patch``^3 out of a ``size``^3 subject on
the device that holds one float32 image and one int16 label map.
``iterate``     the road before ``sample_batch``: ``islice(sampler(subject), n)`` + ``SubjectsBatch.from_subjects``
                (the law copied to the host, one ``torch.multinomial`` per patch, views, one ``torch.stack`` per image);
``reference``   ``sample_batch`` with ``set_centre_draw("reference")``: the same host draws, one gather launch per image;
``device``      ``sample_batch`` with ``set_centre_draw("device")``: ``tio_centre_law_sums`` + ``tio_centre_draw`` + the gathers,
                one small copy back.
These rows are wall time per call with the device synchronised before and after; the rounds alternate the roads after one
warm-up call of each, and every row reports median, minimum and maximum so the spread is visible.
The gather alone (``tio_patch_gather`` of the float32 image's ``patches`` patches, corners already on the device) is device
time per call (events around ``iters`` calls) next to ``torch.stack`` of the same views and next to a device-to-device copy of
the same number of bytes; ``gather_share_of_copy`` is copy time over gather time.
"""
from __future__ import annotations

import argparse
import itertools
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


def summary(samples):
    ordered = sorted(samples)
    return {"median_ms": round(ordered[len(ordered) // 2], 4), "min_ms": round(ordered[0], 4), "max_ms": round(ordered[-1], 4), "samples": len(ordered)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--patch", type=int, default=64)
    parser.add_argument("--patches", type=int, default=16)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_feed.py measures on the GPU; there is none")
    device = torch.device("cuda")
    size, n = args.size, args.patches
    patch = (args.patch,) * 3
    generator = torch.Generator(device="cuda").manual_seed(0)
    axis = torch.arange(size, device=device, dtype=torch.float32) - (size - 1) / 2
    radius = (axis[:, None, None] ** 2 + axis[None, :, None] ** 2 + axis[None, None, :] ** 2).sqrt()
    labels = ((radius < 0.4 * size).to(torch.int16) + (radius < 0.2 * size).to(torch.int16))[None]
    subject = tio.Subject(
        t1=tio.ScalarImage(torch.rand((1, size, size, size), device=device, generator=generator)),
        seg=tio.LabelMap(labels),
    )
    sampler = tio.LabelSampler(subject, patch, label_name="seg", label_probabilities={1: 0.25, 2: 0.75})

    def iterate():
        tio.set_centre_draw("reference")
        return tio.SubjectsBatch.from_subjects(list(itertools.islice(sampler(subject), n)))

    def reference():
        tio.set_centre_draw("reference")
        return sampler.sample_batch(subject, n)

    def on_device():
        tio.set_centre_draw("device")
        return sampler.sample_batch(subject, n)

    roads = {"iterate": iterate, "reference": reference, "device": on_device}
    torch.manual_seed(0)
    for road in roads.values():  # warm-up: library load, allocator, pinned staging
        road()
    samples = {name: [] for name in roads}
    for _ in range(args.rounds):
        for name, road in roads.items():
            samples[name].append(host_timed(road))
    rows = {name: summary(values) for name, values in samples.items()}

    # the gather launch alone, against torch.stack of the views and a copy of the same bytes
    engine = ops.engine()
    tio.set_centre_draw("device")
    data = subject.images["t1"].data
    locations = sampler.sample_batch(subject, n).metadata["patch_location"]
    corners = torch.tensor([where.index for where in locations], dtype=torch.int32, device=device)
    windows = [(slice(None), *where.to_slices()) for where in locations]
    gathered = engine.patch_gather(data, corners, patch)
    assert torch.equal(gathered, torch.stack([data[window] for window in windows]))
    twin = torch.empty_like(gathered)
    kernels = {
        "gather": lambda: engine.patch_gather(data, corners, patch),
        "stack": lambda: torch.stack([data[window] for window in windows]),
        "copy": lambda: twin.copy_(gathered),
    }
    for kernel in kernels.values():
        kernel()
    torch.cuda.synchronize()
    kernel_samples = {name: [] for name in kernels}
    for _ in range(max(args.rounds, 5)):
        for name, kernel in kernels.items():
            kernel_samples[name].append(device_timed(kernel, args.iters))
    kernel_rows = {name: summary(values) for name, values in kernel_samples.items()}
    nbytes = gathered.numel() * gathered.element_size()
    spread = max(row["max_ms"] - row["min_ms"] for row in (kernel_rows["gather"], kernel_rows["stack"]))
    result = {
        "device": torch.cuda.get_device_name(0), "size": size, "patch": args.patch, "patches": n, "rounds": args.rounds, "iters": args.iters,
        "wall_ms_per_call": rows,
        "device_over_iterate_speedup": round(rows["iterate"]["median_ms"] / rows["device"]["median_ms"], 1),
        "reference_over_iterate_speedup": round(rows["iterate"]["median_ms"] / rows["reference"]["median_ms"], 3),
        "device_faster_than_iterate": rows["device"]["max_ms"] < rows["iterate"]["min_ms"],
        "gather_device_ms_per_call": kernel_rows,
        "gather_bytes": nbytes,
        "gather_gb_per_s_read_plus_write": round(2 * nbytes / kernel_rows["gather"]["median_ms"] / 1e6, 1),
        "gather_share_of_copy": round(kernel_rows["copy"]["median_ms"] / kernel_rows["gather"]["median_ms"], 3),
        "gather_minus_stack_ms": round(kernel_rows["gather"]["median_ms"] - kernel_rows["stack"]["median_ms"], 4),
        "run_to_run_spread_ms": round(spread, 4),
        "gather_not_slower_than_stack_beyond_spread": kernel_rows["gather"]["median_ms"] <= kernel_rows["stack"]["median_ms"] + spread,
    }
    tio.set_centre_draw("reference")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
