"""Time Normalize and Standardize on the engine against the reference's operation sequences on ATen, on the same GPU.

    python scripts/bench_intensity_stats.py [--reps 50] [--json out.json]

Inputs: 1 x 1 x 256^3 and 8 x 1 x 256^3 float32, three kinds each — white noise, a volume that is half exact zeros, a
constant volume (every element in one histogram bin: the contention case of the radix select).  Per input:
``Normalize(percentile_low=0.5, percentile_high=99.5)``, ``Standardize()`` and ``Standardize(masking_method=...)`` (an int16
label map, 60 % inside) as ``make_params`` + ``apply_transform`` of this package, and the same lines of the reference
(normalize.py:352-365, :176-183; standardize.py:63-76, :97; _statistics.py:36-43) with torch ops on the device, read-backs
included.  The statistics launches are also timed alone, with the bytes they read against the device-to-device copy rate
(``dst.copy_(src)`` of a 1 GiB buffer, read + written).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchio_amd as tio  # noqa: E402
from torchio_amd import ops  # noqa: E402


def timed(fn, reps, warmup=3):
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


def aten_quantile(values, q):
    index = q * (values.numel() - 1)
    lower = math.floor(index)
    lower_value = torch.kthvalue(values, lower + 1).values
    if index == lower:
        return lower_value
    return lower_value.lerp(torch.kthvalue(values, lower + 2).values, index - lower)


def aten_normalize(data, pct_low, pct_high, out_min=-1.0, out_max=1.0):
    values = data[0].reshape(-1)
    in_min = float(aten_quantile(values.float(), pct_low / 100.0).item())
    in_max = float(aten_quantile(values.float(), pct_high / 100.0).item())
    in_range = in_max - in_min
    if in_range == 0:
        return data
    out = data.float().clamp(in_min, in_max)
    return (out - in_min) / in_range * (out_max - out_min) + out_min


def aten_standardize(data, mask=None):
    tensor = data[0]
    values = tensor[mask.bool().expand_as(tensor)] if mask is not None else tensor.reshape(-1)
    mean = float(values.float().mean().item())
    std = float(values.float().std().item())
    if std == 0:
        return data
    return (data.float() - mean) / std


def make_batch(data, labels):
    subjects = [tio.Subject(t1=tio.ScalarImage(data[b]), seg=tio.LabelMap(labels[b])) for b in range(data.shape[0])]
    return tio.SubjectsBatch.from_subjects(subjects)


def run_transform(transform, batch, original):
    batch.images["t1"].data = original
    try:
        transform.apply_transform(batch, transform.make_params(batch))
    except RuntimeError as error:  # the constant volume: zero deviation (the statistics were computed, which is what is timed)
        if "Standard deviation is zero" not in str(error):
            raise


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=50)
    parser.add_argument("--json", default=None)
    parser.add_argument("--batches", default="1,8")
    args = parser.parse_args()
    engine = ops.engine()
    device = torch.device("cuda")
    src = torch.empty(1 << 30, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), args.reps)
    copy_rate = 2 * src.numel() / copy_ms / 1e6  # GB/s, read + written
    del src, dst
    results = {"copy_GBps": round(copy_rate, 1), "cases": {}}
    print(f"device-to-device copy: {copy_rate:.0f} GB/s (read + written)")
    import warnings

    warnings.simplefilter("ignore")
    for batch_size in [int(b) for b in args.batches.split(",")]:
        shape = (batch_size, 1, 256, 256, 256)
        generator = torch.Generator().manual_seed(batch_size)
        noise = (torch.randn(shape[1:], generator=generator) * 40 + 20).to(device).expand(shape).contiguous()
        half = noise.clone()
        half[:, :, :128] = 0.0
        labels = (torch.rand(shape[1:], generator=generator) < 0.6).to(torch.int16).to(device).expand(shape).contiguous()
        kinds = {"white noise": noise, "half exact zeros": half, "constant": torch.full(shape, 3.25, device=device)}
        n_first = noise[0].numel()
        for kind, data in kinds.items():
            name = f"{batch_size}x1x256^3 {kind}"
            batch = make_batch(data, labels)
            rows = {}

            def row(op, ours_ms, theirs_ms=None, streamed_bytes=None):
                rows[op] = {"engine_ms": round(ours_ms, 3)}
                text = f"{name:28s} {op:26s} engine {ours_ms:8.3f} ms"
                if theirs_ms is not None:
                    rows[op].update(reference_ms=round(theirs_ms, 3), speedup=round(theirs_ms / ours_ms, 1))
                    text += f"   ATen {theirs_ms:9.3f} ms   x{theirs_ms / ours_ms:6.1f}"
                if streamed_bytes is not None:
                    share = streamed_bytes / ours_ms / 1e6 / (copy_rate / 2)  # against the one-way rate: these launches only read
                    rows[op]["share_of_one_way_copy_rate"] = round(share, 3)
                    text += f"   {100 * share:5.1f} % of the one-way copy rate"
                print(text, flush=True)

            normalize = tio.Normalize(percentile_low=0.5, percentile_high=99.5, per_instance=False)
            standardize = tio.Standardize()
            masked = tio.Standardize(masking_method="seg")
            if kind == "white noise":
                ours = normalize.apply_transform(batch, normalize.make_params(batch)).images["t1"].data
                # (not bit for bit: the engine reproduces torch's CPU arithmetic — IEEE division, the CPU lerp —, ATen's device
                # kernels divide by a scalar through its reciprocal)
                assert torch.allclose(ours, aten_normalize(data, 0.5, 99.5), rtol=1e-5, atol=1e-5), "Normalize differs from the ATen sequence"
            row("Normalize(0.5, 99.5)", timed(lambda: run_transform(normalize, batch, data), args.reps), timed(lambda: aten_normalize(data, 0.5, 99.5), args.reps))
            row("Standardize()", timed(lambda: run_transform(standardize, batch, data), args.reps), timed(lambda: aten_standardize(data), args.reps))
            row("Standardize(mask)", timed(lambda: run_transform(masked, batch, data), args.reps), timed(lambda: aten_standardize(data, labels[0]), args.reps))
            row("quantiles alone (3 reads)", timed(lambda: engine.intensity_quantiles(data, [0.005, 0.995]), args.reps), None, 3 * 4 * n_first)
            row("moments alone (1 read)", timed(lambda: engine.intensity_moments(data), args.reps), None, 4 * n_first)
            row("moments, masked", timed(lambda: engine.intensity_moments(data, labels[0]), args.reps), None, 6 * n_first)
            row("map alone (read + write)", timed(lambda: engine.intensity_map(data, "sub_div", in_min=20.0, in_range=40.0), args.reps), None, 4 * data.numel())
            results["cases"][name] = rows
            del batch
        del noise, half, labels, kinds
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as handle:
            json.dump(results, handle, indent=1)


if __name__ == "__main__":
    main()
