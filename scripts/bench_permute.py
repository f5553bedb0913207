"""Time ``Engine.permute3d`` against the ATen sequence the reference runs and against a plain copy, on the same GPU.

    python scripts/bench_permute.py [--rounds 5] [--iters 20] [--size 256] [--json out.json]

Volumes: 8 x 1 x size^3, float32, int16 and uint8 (4-, 2- and 1-byte elements).  All six permutations, each without flips
and with all three.  Per case the same process times three things, ALTERNATING round by round (other people's work shares the machine; a difference only
counts inside one round):
``permute3d``  one ``tio_permute3d`` launch;
``ATen``       reorient.py:63-91 on the device: ``torch.flip`` per flipped axis, ``permute``, ``contiguous``;
``clone``      ``clone`` of the same bytes: the ceiling of a pass that reads and writes every byte once.
Each sample is the device time per call of ``iters`` calls enqueued back to back (events); a row holds the median over
the rounds.  Before a case is timed its two results are compared bit for bit.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchio_amd import ops  # noqa: E402


def device_timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def aten_sequence(data, perm, flips):
    for axis in flips:
        data = torch.flip(data, [2 + axis])
    return data.permute(0, 1, 2 + perm[0], 2 + perm[1], 2 + perm[2]).contiguous()


def median(samples):
    return sorted(samples)[len(samples) // 2]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_permute.py measures on the GPU; there is none")
    engine = ops.engine()
    size, batch = args.size, 8
    rows = []
    for dtype in (torch.float32, torch.int16, torch.uint8):
        data = torch.arange(batch * size**3, device="cuda").remainder_(251 if dtype == torch.uint8 else 30011).to(dtype).reshape(batch, 1, size, size, size)
        moved = 2 * data.numel() * data.element_size()  # read once, written once
        for perm, flips in itertools.product(itertools.permutations(range(3)), ((), (0, 1, 2))):
            calls = {
                "permute3d": lambda: engine.permute3d(data, perm, flips),  # noqa: B023
                "aten": lambda: aten_sequence(data, perm, flips),  # noqa: B023
                "clone": lambda: data.clone(),  # noqa: B023
            }
            if not torch.equal(calls["permute3d"](), calls["aten"]()):
                raise SystemExit(f"permute3d differs from the ATen sequence: {dtype}, perm {perm}, flips {flips}")
            for fn in calls.values():  # every shape and kernel of the timed window has run once
                fn()
            torch.cuda.synchronize()
            samples = {name: [] for name in calls}
            for _ in range(args.rounds):
                for name, fn in calls.items():
                    samples[name].append(device_timed(fn, args.iters))
            ms = {name: median(values) for name, values in samples.items()}
            rows.append({
                "dtype": str(dtype).replace("torch.", ""), "perm": list(perm), "flips": list(flips),
                "route": "rows" if perm[2] == 2 else "tile",
                "permute3d_ms": round(ms["permute3d"], 3), "aten_ms": round(ms["aten"], 3), "clone_ms": round(ms["clone"], 3),
                "permute3d_gb_per_s": round(moved / ms["permute3d"] / 1e6, 1), "clone_gb_per_s": round(moved / ms["clone"] / 1e6, 1),
                "aten_over_permute3d": round(ms["aten"] / ms["permute3d"], 2), "permute3d_over_clone": round(ms["permute3d"] / ms["clone"], 2),
                "permute3d_spread_ms": [round(min(samples["permute3d"]), 3), round(max(samples["permute3d"]), 3)],
            })
        del data
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "shape": [batch, 1, size, size, size], "rounds": args.rounds, "iters": args.iters, "rows": rows}
    print("| dtype | perm | flips | route | permute3d ms (min .. max) | GB/s | ATen ms | ATen / permute3d | clone ms | permute3d / clone |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        low, high = r["permute3d_spread_ms"]
        print(f"| {r['dtype']} | {tuple(r['perm'])} | {'all' if r['flips'] else 'none'} | {r['route']} | {r['permute3d_ms']} ({low} .. {high}) | "
              f"{r['permute3d_gb_per_s']} | {r['aten_ms']} | {r['aten_over_permute3d']} | {r['clone_ms']} | {r['permute3d_over_clone']} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
