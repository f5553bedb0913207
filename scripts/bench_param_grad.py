"""Time the parameter gradients of the intensity ops: each fused reduction next to a copy of the bytes it must read and next to the
same gradient from the torch composition under autograd.

    python scripts/bench_param_grad.py [--batch 8] [--size 256] [--rounds 3] [--iters 5] [--only NAME] [--no-torch NAME]
                                       [--json profiles/intensity_param_grad_bench.json]

Workload: one ``B x 1 x S^3`` float32 volume and a fixed incoming gradient of its shape (8 x 1 x 256^3 by default).  Per entry point:

  kernel   the engine call alone (workspace clear, reduction, finishing kernel; the tap gradient with its stencil intermediates),
           back-to-back launches between two device events;
  copy     a device-to-device copy of the bytes the kernel must read (``x`` and ``gy``; ``gy`` alone for additive Philox noise);
  torch    forward + backward of the reference's composition to the same parameter leaf on the same GPU
           (``F.interpolate`` -> ``exp`` -> ``*``; ``F.pad(mode="replicate")`` + ``conv3d`` per axis; ``x + (mean + std z)``;
           ``sign(x) |x|^gamma``), which is what a user without these kernels runs.

For each leg: device time per call (median, minimum and maximum over the rounds) and the peak of device memory above what is
allocated before the call.  Before anything is timed the two gradients are compared.  The report is rewritten after every entry
point, so an interrupted run keeps what it measured (``--only NAME`` then measures one entry point and merges it into the report).
``--no-torch NAME`` leaves the torch leg of that entry point out: ``F.pad`` + ``conv3d`` with 1 x 1 x 7 kernels on 8 x 256^3 did
not finish its first call within seven minutes on the MI355X.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402


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


def leaf_grad(forward, leaf, grad):
    leaf = leaf.detach().requires_grad_(True)
    (forward(leaf) * grad).sum().backward()
    return leaf.grad


def torch_blur(x, taps, radius):
    """blur.py:157-252: replicate padding and a one-axis conv3d per axis, order I, J, K."""
    out = x
    for axis, r in enumerate(radius):
        pad = [0, 0, 0, 0, 0, 0]
        pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = r
        shape = [1, 1, 1, 1, 1]
        shape[2 + axis] = 2 * r + 1
        out = F.conv3d(F.pad(out, pad, mode="replicate"), taps[0, axis, : 2 * r + 1].reshape(shape))
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--batch", type=int, default=8)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--iters", type=int, default=5)
    parser.add_argument("--only", default=None)
    parser.add_argument("--no-torch", action="append", default=[])
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "intensity_param_grad_bench.json"))
    args = parser.parse_args()
    engine = ops.engine()
    batch, size = args.batch, args.size
    generator = torch.Generator(device="cuda").manual_seed(0)
    shape = (batch, 1, size, size, size)
    x = torch.rand(shape, generator=generator, device="cuda") + 0.25
    grad = torch.randn(shape, generator=generator, device="cuda")
    two, one = torch.empty((2, *shape), device="cuda"), torch.empty(shape, device="cuda")
    pair = torch.stack([x, grad])
    coarse = (torch.rand(batch, 1, 4, 4, 4, generator=generator, device="cuda") - 0.5) * 0.5
    gamma = torch.rand(batch, generator=generator, device="cuda") * 0.6 + 0.7
    mean, std = torch.rand(batch, generator=generator, device="cuda") * 0.1, torch.rand(batch, generator=generator, device="cuda") * 0.2 + 0.05
    radius = [3, 3, 3]
    offsets = torch.arange(-3, 4, dtype=torch.float32, device="cuda")
    kernel = torch.exp(-0.5 * (offsets / 1.0) ** 2)
    taps = (kernel / kernel.sum()).repeat(1, 3, 1)
    seed = 1234
    draws = engine.philox_normal(shape, seed, 0, "cuda")
    per_element = (-1, 1, 1, 1, 1)

    entries = {
        "bias_field_grad": dict(
            kernel=lambda: engine.bias_field_grad(x, grad, coarse), copy=lambda: two.copy_(pair),
            torch=lambda: leaf_grad(lambda c: x * torch.exp(F.interpolate(c, size=shape[2:], mode="trilinear", align_corners=True)), coarse, grad)),
        "gamma_grad": dict(
            kernel=lambda: engine.gamma_grad(x, grad, gamma), copy=lambda: two.copy_(pair),
            torch=lambda: leaf_grad(lambda e: torch.sign(x) * x.abs() ** e.reshape(per_element), gamma, grad)),
        "noise_grad": dict(
            kernel=lambda: engine.noise_grad(x, grad, mean, std, philox_seed=seed), copy=lambda: one.copy_(grad),
            torch=lambda: leaf_grad(lambda s: x + (mean.reshape(per_element) + s.reshape(per_element) * draws), std, grad)),
        "separable_conv3d_taps_grad": dict(
            kernel=lambda: engine.separable_conv3d_taps_grad(x, grad, taps, radius), copy=lambda: two.copy_(pair),
            torch=lambda: leaf_grad(lambda w: torch_blur(x, w, radius), taps, grad)),
    }
    report = {"device": torch.cuda.get_device_name(0), "batch": batch, "size": size, "dtype": "float32", "rounds": args.rounds, "iters": args.iters,
              "blur_radius": radius, "coarse_shape": [4, 4, 4], "entry_points": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    if args.only is not None and os.path.isfile(args.json):
        with open(args.json) as stream:
            report["entry_points"] = json.load(stream).get("entry_points", {})
    for name, legs in entries.items():
        if args.only not in (None, name):
            continue
        entry = {}
        if name in args.no_torch:
            legs = {leg: step for leg, step in legs.items() if leg != "torch"}
            entry["torch"] = None
        else:
            ours, theirs = legs["kernel"](), legs["torch"]()
            ours = ours[1] if isinstance(ours, tuple) else ours
            entry["max_relative_difference_kernel_vs_torch"] = float((ours.reshape(-1) - theirs.reshape(-1)).abs().max() / theirs.abs().max())
            del ours, theirs
        print(f"{name}: timing {sorted(legs)}", flush=True)
        samples = {leg: [] for leg in legs}
        for leg in legs.values():  # warm-up: allocator, library heuristics
            timed(leg, 1)
        for _ in range(args.rounds):
            for leg_name, leg in legs.items():
                samples[leg_name].append(timed(leg, args.iters if leg_name != "torch" else max(1, args.iters // 2)))
        for leg_name, runs in samples.items():
            times = [t for t, _ in runs]
            entry[leg_name] = {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times),
                               "peak_mib_above_inputs": max(m for _, m in runs)}
        entry["kernel_over_copy_time"] = entry["kernel"]["ms_median"] / entry["copy"]["ms_median"]
        if entry["torch"] is not None:
            entry["torch_over_kernel_time"] = entry["torch"]["ms_median"] / entry["kernel"]["ms_median"]
        report["entry_points"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        with open(args.json, "w") as stream:
            json.dump(report, stream, indent=1)
            stream.write("\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
