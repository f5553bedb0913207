"""Time loading NIfTI files onto the GPU: ``tio_nifti_decode`` alone, the whole road from files to a stacked batch, and the
three-pass composition the kernel replaces.

    python scripts/bench_nifti_load.py [--size 256] [--batch 8] [--rounds 5] [--iters 20] [--json profiles/nifti_load_bench.json]

Files: ``batch`` volumes of ``size``^3, int16 (unscaled and with a slope / intercept) and float32, as ``.nii``, and the int16
ones as ``.nii.gz`` too, written to a temporary directory with ``struct`` / ``tobytes(order="F")`` (not with the library's
writer).  The voxels are smooth structure plus noise (12 bits used), so that gzip has something to do but not everything.

(a) kernel   device time (events) per ``tio_nifti_decode`` launch over ``iters`` launches back to back on bytes that are already
             on the device; effective GB/s = (disk bytes + output bytes) / time; next to it a device-to-device copy
             (``hipMemcpyAsync`` under ``Tensor.copy_``) that READS AND WRITES the same total (a buffer of half that many bytes),
             timed in the same rounds, alternating.
(b) road     wall time, ending in a device synchronise, of ``SubjectsBatch.from_subjects(subjects, device="cuda")`` on fresh
             ``Subject``s against a plain numpy decode written out below (``frombuffer``, ``reshape(order="F")``,
             ``ascontiguousarray``, ``astype``, ``from_numpy``, ``stack``, ``.to("cuda")``), alternating, warm page cache;
             for ``.nii.gz`` also the inflate alone.
(c) 3-pass   the scaled int16 case as ``tio_permute3d`` + ``.to(float32)`` + one scale pass: device time and peak device memory
             next to the single launch's.
Before anything is timed the results of the roads are compared.
"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchio_amd as tio  # noqa: E402
from torchio_amd import ops  # noqa: E402

SLOPE, INTER = 0.25, -1024.0
CODES = {"int16": (4, "<i2"), "float32": (16, "<f4")}


def build_file(path, array, code, slope=0.0, inter=0.0):
    header = bytearray(348)
    struct.pack_into("<i", header, 0, 348)
    struct.pack_into("<8h", header, 40, 3, *array.shape, 1, 1, 1, 1)
    struct.pack_into("<hh", header, 70, code, 8 * array.dtype.itemsize)
    struct.pack_into("<8f", header, 76, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into("<3f", header, 108, 352.0, slope, inter)
    struct.pack_into("<hh", header, 252, 0, 1)
    struct.pack_into("<12f", header, 280, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    header[344:348] = b"n+1\0"
    content = bytes(header) + b"\0\0\0\0" + array.tobytes(order="F")
    opener = gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")
    with opener as stream:
        stream.write(content)


def make_volume(size, seed):
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0, 3000, size, dtype=np.float32)
    volume = ramp[:, None, None] * 0.5 + ramp[None, :, None] * 0.3 + ramp[None, None, :] * 0.2
    return (volume + rng.normal(0, 40, size=volume.shape).astype(np.float32)).clip(0, 4095)


def numpy_road(paths, kind, scaled, size):
    """The usual host decode, written out: what a reader without this kernel does."""
    tensors = []
    for path in paths:
        if path.endswith(".gz"):
            with gzip.open(path, "rb") as stream:
                raw = stream.read()
        else:
            with open(path, "rb") as stream:
                raw = stream.read()
        array = np.frombuffer(raw, dtype=CODES[kind][1], offset=352).reshape((size, size, size), order="F")
        array = np.ascontiguousarray(array)
        if scaled:
            array = array.astype(np.float64) * SLOPE + INTER
        tensors.append(torch.from_numpy(array.astype(np.float32) if scaled or kind == "float32" else array))
    out = torch.stack(tensors).unsqueeze(1).to("cuda")
    torch.cuda.synchronize()
    return out


def engine_road(paths, dtype):
    subjects = [tio.Subject(image=tio.ScalarImage.from_file(path, dtype=dtype)) for path in paths]
    out = tio.SubjectsBatch.from_subjects(subjects, device="cuda").image.data
    torch.cuda.synchronize()
    return out


def wall(fn):
    start = time.perf_counter()
    fn()
    return (time.perf_counter() - start) * 1e3


def device_timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def median(samples):
    return sorted(samples)[len(samples) // 2]


def summary(samples):
    return {"median_ms": round(median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--batch", type=int, default=8)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    size, batch = args.size, args.batch
    result = {"size": size, "batch": batch, "rounds": args.rounds, "iters": args.iters, "kernel": [], "road": [], "three_pass": {}}
    with tempfile.TemporaryDirectory() as directory:
        files = {}
        for case, kind, scaled, suffix in (("int16", "int16", False, ".nii"), ("int16 scaled", "int16", True, ".nii"),
                                          ("float32", "float32", False, ".nii"), ("int16 gz", "int16", False, ".nii.gz")):
            paths = []
            for index in range(batch):
                path = os.path.join(directory, f"{case.replace(' ', '_')}_{index}{suffix}")
                build_file(path, make_volume(size, index).astype(CODES[kind][1]), CODES[kind][0], *((SLOPE, INTER) if scaled else ()))
                paths.append(path)
            files[case] = (paths, kind, scaled)
        if not torch.cuda.is_available():
            raise SystemExit("bench_nifti_load.py measures on the GPU; there is none (the files were built)")
        engine = ops.engine()
        voxels = batch * size**3

        # (a) the kernel alone
        for case, code, element, scaled, out_dtype in (("int16 -> int16", 4, 2, False, None), ("int16 scaled -> float32", 4, 2, True, torch.float32),
                                                       ("int16 scaled -> float64", 4, 2, True, None), ("float32 -> float32", 16, 4, False, None),
                                                       ("int16 big-endian -> float32", 4, 2, False, torch.float32)):
            raw = torch.randint(0, 256, (voxels * element,), dtype=torch.uint8, device="cuda")
            call = lambda: engine.nifti_decode(raw, disk_type=code, shape=(size,) * 3, batch=batch, swap_bytes="big-endian" in case,  # noqa: E731, B023
                                               slope=SLOPE if scaled else None, inter=INTER, out_dtype=out_dtype)  # noqa: B023
            out = call()
            moved = raw.numel() + out.numel() * out.element_size()
            source = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            target = torch.empty_like(source)
            copy = lambda: target.copy_(source)  # noqa: E731, B023
            del out
            for fn in (call, copy):
                device_timed(fn, 3)
            samples = {"decode": [], "copy": []}
            for _ in range(args.rounds):
                samples["decode"].append(device_timed(call, args.iters))
                samples["copy"].append(device_timed(copy, args.iters))
            decode_ms, copy_ms = median(samples["decode"]), median(samples["copy"])
            result["kernel"].append({
                "case": case, "bytes_moved": moved, "decode": summary(samples["decode"]), "copy": summary(samples["copy"]),
                "decode_gb_per_s": round(moved / decode_ms / 1e6, 1), "copy_gb_per_s": round(moved / copy_ms / 1e6, 1),
                "decode_over_copy": round(decode_ms / copy_ms, 2),
            })
            del raw, source, target

        # (b) the whole road
        for case, (paths, kind, scaled) in files.items():
            dtype = torch.float32 if scaled else None
            ours, theirs = engine_road(paths, dtype), numpy_road(paths, kind, scaled, size)  # (also the warm-up: page cache, pinned pool)
            if ours.dtype != theirs.dtype or not torch.equal(ours, theirs):
                raise SystemExit(f"{case}: the engine's road and the numpy road differ")
            del ours, theirs
            samples = {"engine": [], "numpy": []}
            for _ in range(args.rounds):
                samples["engine"].append(wall(lambda: engine_road(paths, dtype)))  # noqa: B023
                samples["numpy"].append(wall(lambda: numpy_road(paths, kind, scaled, size)))  # noqa: B023
            row = {"case": case, "engine": summary(samples["engine"]), "numpy": summary(samples["numpy"]),
                   "numpy_over_engine": round(median(samples["numpy"]) / median(samples["engine"]), 2)}
            if case.endswith("gz"):
                inflate = [wall(lambda: [gzip.open(path, "rb").read() for path in paths]) for _ in range(args.rounds)]  # noqa: B023
                row["inflate_alone"] = summary(inflate)
                row["inflate_share_of_engine_road"] = round(median(inflate) / median(samples["engine"]), 2)
            result["road"].append(row)

        # (c) the three-pass composition, scaled int16 -> float32
        raw = torch.randint(0, 256, (voxels * 2,), dtype=torch.uint8, device="cuda")
        inter = torch.tensor(INTER, device="cuda")

        def three_pass():
            disk = raw.view(torch.int16).view(batch, 1, size, size, size)  # (B, C, K, J, I) as it lies on disk
            return torch.add(inter, engine.permute3d(disk, (2, 1, 0)).to(torch.float32), alpha=SLOPE)

        def one_launch():
            return engine.nifti_decode(raw, disk_type=4, shape=(size,) * 3, batch=batch, slope=SLOPE, inter=INTER, out_dtype=torch.float32)

        close = torch.allclose(three_pass(), one_launch(), rtol=1e-6, atol=1e-3)  # (float32 arithmetic against float64 + one rounding)
        if not close:
            raise SystemExit("the three-pass composition and the single launch disagree")
        peaks, samples = {}, {"three_pass": [], "one_launch": []}
        for name, fn in (("three_pass", three_pass), ("one_launch", one_launch)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        for _ in range(args.rounds):
            samples["three_pass"].append(device_timed(three_pass, args.iters))
            samples["one_launch"].append(device_timed(one_launch, args.iters))
        result["three_pass"] = {
            "case": "int16 scaled -> float32", "three_pass": summary(samples["three_pass"]), "one_launch": summary(samples["one_launch"]),
            "three_pass_over_one_launch": round(median(samples["three_pass"]) / median(samples["one_launch"]), 2),
            "peak_bytes_above_the_input": peaks, "output_bytes": voxels * 4,
        }
    result["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(result, indent=1))
    if args.json:
        with open(args.json, "w") as stream:
            json.dump(result, stream, indent=1)
            stream.write("\n")


if __name__ == "__main__":
    main()
