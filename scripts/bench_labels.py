"""Time the label-map kernels against the reference's operation sequences on ATen, on the same GPU.

    python scripts/bench_labels.py [--reps 10] [--json out.json]

Two inputs: 8 x 1 x 256^3 and 1 x 1 x 512^3 int16 label maps (four values, box-filtered noise cut at its quantiles: blobs
of many sizes).  Per op: the engine call, the reference's sequence (transforms/label/*.py) with torch ops on the device
and, for the three streaming kernels (remap, one-hot, contour), the share of the device-to-device copy rate
(``dst.copy_(src)`` of a 1 GiB buffer) their read + written bytes reach.  ``KeepLargestComponent``'s reference leaves the
device (SimpleITK per label and element); it is timed against ``scipy.ndimage.label`` on the host, copies included.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402


def label_field(shape, seed, device):
    noise = torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(device)
    for _ in range(2):
        noise = F.avg_pool3d(noise, 3, stride=1, padding=1)
    cuts = torch.quantile(noise.reshape(-1)[::97][:1000000], torch.tensor([0.4, 0.6, 0.8], device=device))
    return (noise[..., None] > cuts).sum(-1).to(torch.int16)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) / reps * 1e3


def aten_remap(data, mapping, default=None):
    out = data.clone() if default is None else torch.full_like(data, default)
    for old, new in mapping.items():
        out[data == old] = new
    return out


def aten_one_hot(data, num_classes):
    return F.one_hot(data.long()[:, 0], num_classes=num_classes).permute(0, 4, 1, 2, 3).float()


def aten_contour(data):
    padded = F.pad(data.float(), [1] * 6, mode="constant", value=-1)
    return (-F.max_pool3d(-padded, kernel_size=3, stride=1, padding=0) != data.float()).float()


def host_keep_largest(data, labels, background=0):
    import numpy as np
    from scipy import ndimage

    host = data.cpu().numpy()
    out = host.copy()
    for b in range(host.shape[0]):
        for value in labels:
            numbered, count = ndimage.label(host[b, 0] == value, structure=np.ones((3, 3, 3)))
            if count:
                sizes = np.bincount(numbered.reshape(-1))[1:]
                out[b, 0][(numbered > 0) & (numbered != 1 + int(sizes.argmax()))] = background
    return torch.from_numpy(out).to(data.device)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--json", default=None)
    parser.add_argument("--no-host", action="store_true", help="skip the scipy timing (minutes at these sizes)")
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
    mapping = {1: 2, 2: 1, 3: 7}
    for name, shape in (("8x1x256^3", (8, 1, 256, 256, 256)), ("1x1x512^3", (1, 1, 512, 512, 512))):
        data = label_field(shape, 0, device)
        n = data.numel()
        rows = {}

        def row(op, ours_ms, theirs_ms, streamed_bytes=None):
            rows[op] = {"engine_ms": round(ours_ms, 3), "reference_ms": round(theirs_ms, 3), "speedup": round(theirs_ms / ours_ms, 1)}
            text = f"{name:10s} {op:22s} engine {ours_ms:9.3f} ms   reference {theirs_ms:10.3f} ms   x{theirs_ms / ours_ms:7.1f}"
            if streamed_bytes is not None:
                share = streamed_bytes / ours_ms / 1e6 / copy_rate
                rows[op]["share_of_copy_rate"] = round(share, 3)
                text += f"   {100 * share:5.1f} % of the copy rate"
            print(text, flush=True)

        assert torch.equal(engine.label_remap(data, mapping), aten_remap(data, mapping))
        row("remap (3 pairs)", timed(lambda: engine.label_remap(data, mapping), args.reps), timed(lambda: aten_remap(data, mapping), args.reps), 4 * n)
        row("sequential (4 pairs)", timed(lambda: engine.label_remap(data, {0: 0, 1: 1, 2: 2, 3: 3}, default=0), args.reps),
            timed(lambda: aten_remap(data, {0: 0, 1: 1, 2: 2, 3: 3}, default=0), args.reps), 4 * n)
        assert torch.equal(engine.label_one_hot(data, 4), aten_one_hot(data, 4))
        row("one-hot (4 classes)", timed(lambda: engine.label_one_hot(data, 4), args.reps), timed(lambda: aten_one_hot(data, 4), args.reps), 18 * n)
        assert torch.equal(engine.label_contour(data), aten_contour(data))
        row("contour", timed(lambda: engine.label_contour(data), args.reps), timed(lambda: aten_contour(data), args.reps), 6 * n)
        ours = timed(lambda: engine.keep_largest_component(data, [1, 2, 3]), args.reps)
        if args.no_host:
            rows["keep largest (3 labels)"] = {"engine_ms": round(ours, 3)}
            print(f"{name:10s} keep largest (3 labels) engine {ours:9.3f} ms", flush=True)
        else:
            start = time.perf_counter()
            expected = host_keep_largest(data, [1, 2, 3])
            theirs = (time.perf_counter() - start) * 1e3
            equal = torch.equal(engine.keep_largest_component(data, [1, 2, 3]), expected)
            row("keep largest (3 labels)", ours, theirs)
            rows["keep largest (3 labels)"]["equals_scipy"] = equal  # (False only if two largest components tie)
            print(f"{name:10s} keep largest equals the scipy result: {equal}", flush=True)
        results["cases"][name] = rows
        del data
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as handle:
            json.dump(results, handle, indent=1)


if __name__ == "__main__":
    main()
