"""Time the gradient with respect to the mapping and the control points: the engine's fused launch against the ATen road.

    python scripts/bench_geometry_grad.py [--rounds 5] [--iters 10] [--json profiles/geometry_grad_bench.json]

Workload: forward + backward with respect to a batched ``(B, 3, 4)`` mapping and a batched ``(B, 7, 7, 7, 3)`` control grid of one
``B x 1 x S^3`` float32 volume, at 8 x 1 x 256^3 and at 2 x 1 x 128^3; the loss is ``<out, g>`` with a fixed ``g``.

(a) road      ``torchio_amd.warp`` + ``backward`` against ``tests/aten_pipeline.resample`` (the materialised grid +
              ``F.grid_sample``) + ``backward`` to the same leaves, on the same GPU, the two alternating over ``rounds`` rounds of
              ``iters`` steps; device time per step (events), median over the rounds, and the peak of device memory above what is
              allocated before the step (inputs, leaves, ``g``).
(b) kernel    ``tio_resample3d_geometry_grad`` alone (with its workspace clear and its finishing kernel) next to one
              ``TIO_LINEAR_ADJOINT`` launch of the same geometry (with the zero fill of its accumulator): it reads the same taps and
              one more volume per channel.
Before anything is timed the two roads' gradients are compared.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aten_pipeline  # noqa: E402
import torchio_amd as tio  # noqa: E402
from torchio_amd import ops  # noqa: E402


def make_inputs(batch, size, seed=0):
    generator = torch.Generator().manual_seed(seed)
    axes = [torch.arange(size, dtype=torch.float32) for _ in range(3)]
    i, j, k = torch.meshgrid(*axes, indexing="ij")
    smooth = torch.sin(0.11 * i) * torch.cos(0.07 * j) + 0.5 * torch.sin(0.05 * k + 0.02 * j)
    volume = (smooth[None, None] + (torch.rand(batch, 1, size, size, size, generator=generator) - 0.5) * 0.3).to("cuda")
    mapping = torch.eye(3, 4)[None].repeat(batch, 1, 1)
    mapping[:, :, :3] += (torch.rand(batch, 3, 3, generator=generator) - 0.5) * 0.08
    mapping[:, :, 3] = (torch.rand(batch, 3, generator=generator) - 0.5) * 6.0
    control = (torch.rand(batch, 7, 7, 7, 3, generator=generator) - 0.5) * 8.0
    grad = torch.randn(batch, 1, size, size, size, generator=generator).to("cuda")
    return volume, mapping.to("cuda"), control.to("cuda"), grad


def engine_step(volume, mapping, control, grad):
    mapping, control = mapping.detach().requires_grad_(True), control.detach().requires_grad_(True)
    (tio.warp(volume, mapping, control) * grad).sum().backward()
    return mapping.grad, control.grad


def aten_step(volume, mapping, control, grad):
    mapping, control = mapping.detach().requires_grad_(True), control.detach().requires_grad_(True)
    (aten_pipeline.resample(volume, mapping, control, None) * grad).sum().backward()
    return mapping.grad, control.grad


def timed(step, iters):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "geometry_grad_bench.json"))
    args = parser.parse_args()
    engine = ops.engine()
    report = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "workloads": []}
    for batch, size in ((2, 128), (8, 256)):
        volume, mapping, control, grad = make_inputs(batch, size)
        ours, theirs = engine_step(volume, mapping, control, grad), aten_step(volume, mapping, control, grad)
        agreement = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, theirs, strict=True)]
        legs = {"engine": lambda: engine_step(volume, mapping, control, grad), "aten": lambda: aten_step(volume, mapping, control, grad)}  # noqa: B023
        shared = dict(out_shape=volume.shape[2:], mapping=mapping, control_points=control, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True)

        def adjoint():
            accumulator = torch.zeros_like(volume)
            engine.resample3d([accumulator], interps=["linear_adjoint"], fills=[None], _adjoint_of=[grad], **shared)  # noqa: B023

        legs["geometry_grad_kernel"] = lambda: engine.resample3d_geometry_grad([volume], [grad], fills=[None], **shared)  # noqa: B023
        legs["adjoint_launch"] = adjoint
        samples = {name: [] for name in legs}
        for leg in legs.values():  # warm-up: allocator, plans, autotuned libraries
            timed(leg, 2)
        for _ in range(args.rounds):
            for name, leg in legs.items():
                samples[name].append(timed(leg, args.iters))
        entry = {"batch": batch, "size": size, "max_relative_difference_engine_vs_aten": {"mapping": agreement[0], "control_points": agreement[1]}}
        for name, runs in samples.items():
            times = [t for t, _ in runs]
            entry[name] = {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times),
                           "peak_mib_above_inputs": max(m for _, m in runs)}
        entry["aten_over_engine_time"] = entry["aten"]["ms_median"] / entry["engine"]["ms_median"]
        entry["geometry_grad_over_adjoint_time"] = entry["geometry_grad_kernel"]["ms_median"] / entry["adjoint_launch"]["ms_median"]
        report["workloads"].append(entry)
        print(json.dumps(entry), flush=True)
        del volume, mapping, control, grad, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as stream:
        json.dump(report, stream, indent=1)
        stream.write("\n")


if __name__ == "__main__":
    main()
