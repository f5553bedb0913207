"""Headline benchmark: volumes/s for Compose[Affine, ElasticDeformation, BiasField, Blur, Noise] on 256^3 float32.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line.  ``--full`` adds everything else the line
can carry (the roofline's per-launch timing, the other noise / resampling modes, multi-stream, the other configurations,
the stock-ATen and CPU baselines, the measured HBM ceiling).  ``--dump-outputs DIR`` writes what the last timed step
returned as ``DIR/<name>.npy`` (see ``dump_outputs``).

One "step" = one pass of the Compose over one device-resident SubjectsBatch of
`--batch` (default 8) synthetic 1x256^3 float32 volumes per GPU with per-instance
parameters (the reference's default for batches).  Inputs are resident in HBM
before the timed region; outputs stay on the device.  Weak scaling: the per-GPU
batch is fixed, ranks never exchange data; the only collective is the all-gather
of three counters per rank at the end.  Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torchio_amd as tio  # noqa: E402
from torchio_amd import distributed as tdist  # noqa: E402
from torchio_amd import ops  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def stencil_mode(resample_precision: str) -> str:
    """The Blur's taps of a resampling mode: the reference's rounding sequence in "exact", fused multiply-adds otherwise."""
    return "exact" if resample_precision == "exact" else "fast"


def build_transform() -> tio.Compose:
    """The metric's pipeline with the explicit ranges of SURVEY.md §8(d) / BASELINE.md §3."""
    return tio.Compose(
        [
            tio.Affine(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5)),
            tio.ElasticDeformation(),
            tio.BiasField(),
            tio.Blur(std=(0.5, 2)),
            tio.Noise(),
        ]
    )


def make_batch(size: int, batch: int, seed: int, device) -> tio.SubjectsBatch:
    generator = torch.Generator(device=device).manual_seed(seed)
    data = torch.rand(batch, 1, size, size, size, generator=generator, device=device)
    affines = [tio.AffineMatrix() for _ in range(batch)]
    return tio.SubjectsBatch({"t1": tio.ImagesBatch(data, affines, image_class=tio.ScalarImage)})


class KernelTimer:
    """HIP-event timing of one C-ABI entry point on the stream it is launched on.

    The engine launches on torch's current stream, so torch.cuda.Event brackets
    exactly the kernel(s) of that call.  Events are only resolved after the timed
    region (no sync inside it).
    """

    def __init__(self, engine, name: str):
        self.engine, self.name, self.pairs, self.active = engine, name, [], False
        self._original = engine._call

        def timed_call(fn_name, ref, *args):
            if self.active and fn_name == self.name:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                self._original(fn_name, ref, *args)
                end.record()
                self.pairs.append((start, end))
            else:
                self._original(fn_name, ref, *args)

        engine._call = timed_call

    def mean_ms(self) -> float | None:
        if not self.pairs:
            return None
        return sum(s.elapsed_time(e) for s, e in self.pairs) / len(self.pairs)


def cpu_reference_ops_baseline(size: int, seed: int) -> dict:
    """The reference's CPU path: the op sequence its transforms dispatch to ATen (``grid_sample`` twice per resampling,
    ``interpolate``, ``conv3d`` on a replicate pad, ``randn``: tests/aten_pipeline.py restates it op for op — the
    reference itself cannot travel to the GPU box) on torch-CPU tensors, on this box's host cores: all of them and ONE
    thread (SURVEY.md §8(d) protocol).  Bounded sample: one 1x256^3 volume per run — a warm-up + two timed
    runs on all cores, one timed run on one thread (~40 s of wall clock)."""
    import aten_pipeline  # noqa: PLC0415

    cores = os.cpu_count() or 1
    previous = torch.get_num_threads()
    data = torch.rand(1, 1, size, size, size, generator=torch.Generator().manual_seed(seed))
    rng = torch.Generator()

    def run() -> float:
        start = time.perf_counter()
        aten_pipeline.compose_step(data, rng.manual_seed(7))
        return time.perf_counter() - start

    legs = {}
    try:
        # all cores (the protocol's leg), a moderate count (256 hardware threads oversubscribe these memory-bound ATen kernels:
        # measured on the MI355X box's host 10.4 s per volume on 256 threads against 5.3 s on ONE) and one thread
        for threads in sorted({cores, min(cores, 32), 1}, reverse=True):
            torch.set_num_threads(threads)
            if threads == cores:
                run()  # warm-up (page-in, thread pool, oneDNN primitive selection)
            times = sorted(run() for _ in range(2 if threads == cores else 1))
            legs[threads] = times
    finally:
        torch.set_num_threads(previous)
    best_threads = min(legs, key=lambda t: legs[t][0])
    best = legs[best_threads][0]
    return {
        "value": 1.0 / best, "unit": "volumes/s", "cores": best_threads, "kind": "port",
        # (what it is: DESIGN.md §5 — the reference's own op sequence on torch-CPU ATen; `value` = the fastest leg)
        "sample": f"1 x 1x{size}^3 f32 per run, reference op sequence on torch-CPU ATen (tests/aten_pipeline.py); s/volume by threads: "
                  + ", ".join(f"{t}: {legs[t][0]:.2f}" for t in sorted(legs, reverse=True)),
        "host_cpus": cores,
        "seconds_per_volume": {str(t): legs[t][0] for t in sorted(legs, reverse=True)},
    }


def recorded_reference_timing() -> dict | None:
    """The REAL reference (TorchIO 2.0.0a2, stub-imported, unmodified) timed by scripts/time_reference_cpu.py in the BUILD
    CONTAINER — /root/reference does not exist on this box, so this leg is a recording (profiles/r05_reference_cpu_timing.json),
    carried next to the legs measured live here.  `kind: "reference"`, on that container's cores (8), not this box's."""
    path = os.path.join(ROOT, "profiles", "r05_reference_cpu_timing.json")
    try:
        with open(path) as handle:
            report = json.load(handle)
    except (OSError, ValueError):
        return None
    legs = report.get("legs", {})
    best = min(legs.values(), key=lambda leg: leg["transform(subject)_s"]["min"]) if legs else None
    if best is None:
        return None
    return {
        "value": 1.0 / best["transform(subject)_s"]["min"], "unit": "volumes/s", "cores": best["threads"], "kind": "reference",
        "recorded": True, "where": f"build container, {report.get('host_cpus')} CPUs (not this box)",
        "sample": "1 x 1x256^3 f32 through the unmodified reference, transform(subject), min of 3",
        "seconds_per_volume": {str(threads): leg["transform(subject)_s"]["min"] for threads, leg in legs.items()},
        "source": "profiles/r05_reference_cpu_timing.json",
    }


def hbm_measured_ceiling(device, n_bytes: int = 512 * 2**20, reps: int = 10) -> dict:
    """What this box's HBM delivers to plain streaming kernels on the bench's own stream ("the vendor
    figure and also a measured hipMemcpyDtoD / stream-triad ceiling"): a device-to-device copy (read + write) and a
    triad c = a + s b (two reads + one write) over buffers of the bench batch's size, HIP events around `reps` launches."""
    n = n_bytes // 4
    a, b, c = (torch.rand(n, device=device) for _ in range(3))

    def timed(fn, moved: int) -> float:
        for _ in range(3):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return moved * reps / (start.elapsed_time(end) * 1e-3) / 1e9

    copy = timed(lambda: c.copy_(a), 2 * n_bytes)
    triad = timed(lambda: torch.add(a, b, alpha=1.5, out=c), 3 * n_bytes)
    return {"d2d_copy_GBps": copy, "triad_GBps": triad}  # (torch's copy / add kernels on the bench stream; bytes read + written)


def cpu_baseline(size: int, n_volumes: int, seed: int, budget_s: float = 12.0) -> dict:
    """The CPU oracle ("port") timed on this host's cores on a bounded sample of the same workload."""
    from oracle.oracle import num_threads, oracle_engine  # noqa: PLC0415
    from parity_harness import use_engine  # noqa: PLC0415

    transform = build_transform()
    batch = make_batch(size, n_volumes, seed, "cpu")
    torch.manual_seed(seed)
    done, elapsed = 0, 0.0
    with use_engine(oracle_engine()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        transform(make_batch(size, 1, seed, "cpu"))  # warm-up (page-in, OpenMP pool)
        while elapsed < budget_s and done < 64 * n_volumes:  # bounded sample: ~budget_s of CPU work
            start = time.perf_counter()
            transform(batch)
            elapsed += time.perf_counter() - start
            done += n_volumes
    return {
        "value": done / elapsed, "unit": "volumes/s", "cores": num_threads(), "kind": "port",
        "sample": f"{done} x 1x{size}^3 f32, same Compose through oracle/libtio_oracle.so (C, OpenMP)", "seconds": elapsed,
    }


def aten_baseline(size: int, batch: int, device, steps: int = 3) -> dict:
    """Stock ATen ops on the same GPU: the reference's op sequence restated in tests/aten_pipeline.py."""
    import aten_pipeline  # noqa: PLC0415

    rng = torch.Generator()
    data = torch.rand(batch, 1, size, size, size, device=device)
    # Steady state: the same parameter draw every step, so MIOpen's per-shape selection of the
    # grouped conv3d (which otherwise costs seconds whenever a new blur radius shows up) is
    # paid in the warm-up and not timed.
    aten_pipeline.compose_step(data, rng.manual_seed(7))
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(steps):
        aten_pipeline.compose_step(data, rng.manual_seed(7))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    return {
        "value": steps * batch / elapsed, "unit": "volumes/s", "kind": "stock ATen ops on the same MI355X (tests/aten_pipeline.py)",
        "sample": f"{steps} x {batch} x 1x{size}^3 f32", "peak_memory_GiB": torch.cuda.max_memory_allocated() / 2**30,
    }


DUMP_BUDGET_BYTES = 32 * 2**20  # the image's voxels written by --dump-outputs at most, all ranks together (a seeded sample above it)
DUMP_SAMPLE_SEED = 20261016


def dump_outputs(out, directory: str, suffix: str = "", budget_bytes: int = DUMP_BUDGET_BYTES) -> dict:
    """What the timed path handed back in its last step, as ``.npy`` files: ``t1.npy`` (float32) holds the image's voxels —
    the whole ``(B, 1, D, H, W)`` tensor when it fits *budget_bytes*, otherwise the same fixed, seeded sample of
    voxel positions (sorted flat indices) of every volume, ``(B, n)`` — and ``t1_affine.npy`` (float64) the ``(B, 4, 4)``
    affines.  The inputs are seeded, so two builds run with the same arguments can be compared file by file."""
    import numpy as np  # noqa: PLC0415

    os.makedirs(directory, exist_ok=True)
    image = out["t1"]
    data = image.data.detach()
    arrays = {}
    if data.numel() * 4 <= budget_bytes:
        arrays["t1"] = data.float().cpu().numpy()
    else:
        flat = data.reshape(data.shape[0], -1)
        per_volume = min(flat.shape[1], budget_bytes // 4 // flat.shape[0])
        index = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(flat.shape[1], per_volume, replace=False))
        arrays["t1"] = flat[:, torch.from_numpy(index).to(flat.device)].float().cpu().numpy()
    arrays["t1_affine"] = torch.stack([affine.data.double().cpu() for affine in image.affines]).numpy()
    written = {}
    for name, array in arrays.items():
        np.save(os.path.join(directory, f"{name}{suffix}.npy"), array)
        written[f"{name}{suffix}"] = list(array.shape)
    return written


def time_mode(transform, batch, steps: int, *, noise_rng: str, precision: str, seed: int, timer=None, launch_bytes: int = 0, draw_policy: str | None = None,
              noise_plan: str | None = None) -> dict:
    """A few steps of the same Compose in another (noise rng, resample precision) mode: volumes/s on this GPU, and the
    mean duration of the tio_resample3d launches in that mode (live HIP events, as for the headline's roofline)."""
    previous = (tio.get_noise_rng(), tio.get_resample_precision(), tio.get_stencil_precision(), tio.get_draw_policy(), tio.get_noise_plan())
    tio.set_noise_rng(noise_rng)
    if noise_plan is not None:
        tio.set_noise_plan(noise_plan)
    if draw_policy is not None:
        tio.set_draw_policy(draw_policy)
    tio.set_resample_precision(precision)
    tio.set_stencil_precision(stencil_mode(precision))
    try:
        torch.manual_seed(seed)
        # (warm: a mode's first steps grow the caching allocator's pools — the reference-noise modes draw on a stream of their
        # own, whose pool starts empty: their first steps are device allocations of 512 MiB each)
        for _ in range(12):
            transform(batch)
        torch.cuda.synchronize()
        if timer is not None:
            timer.pairs, timer.active = [], True
        start = time.perf_counter()
        for _ in range(steps):
            out = transform(batch)
        del out
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - start
    finally:
        if timer is not None:
            timer.active = False
        tio.set_noise_rng(previous[0])
        tio.set_resample_precision(previous[1])
        tio.set_stencil_precision(previous[2])
        tio.set_draw_policy(previous[3])
        tio.set_noise_plan(previous[4])
    n = steps * batch.batch_size
    result = {"volumes_per_s": n / elapsed, "ms_per_step": 1e3 * elapsed / steps, "steps": steps}
    launch_ms = timer.mean_ms() if timer is not None else None
    if launch_ms:
        result["resample_launch_ms"] = launch_ms
        result["resample_frac_of_hbm_peak"] = launch_bytes / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
    return result


def multi_stream(transform, batch, steps: int, n_streams: int) -> dict:
    """The headline step issued from this ONE host thread on *n_streams* alternating HIP streams (step n on stream n mod S):
    consecutive steps are independent, so their kernels may overlap on the device — no single kernel saturates a unit of the
    chip.  Reported next to `value`, never as `value`: under overlap a kernel's duration is no longer its own, and the
    roofline of the line is measured on the single stream."""
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    outs = [None] * n_streams
    for step in range(6 * n_streams):  # warm the allocator's per-stream pools
        with torch.cuda.stream(streams[step % n_streams]):
            outs[step % n_streams] = transform(batch)
    torch.cuda.synchronize()
    start = time.perf_counter()
    for step in range(steps):
        with torch.cuda.stream(streams[step % n_streams]):
            outs[step % n_streams] = transform(batch)
    host = time.perf_counter() - start
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    del outs
    return {"volumes_per_s": steps * batch.batch_size / elapsed, "ms_per_step": 1e3 * elapsed / steps, "host_enqueue_ms_per_step": 1e3 * host / steps, "steps": steps}


def other_configs(batch, size: int, device, timer) -> dict:
    """The other configurations BASELINE.json names, on this GPU, in both north-star-compliant resampling precisions: the fused
    ``tio.Spatial`` (affine + elastic in ONE resampling — the north-star's named kernel) and ``Compose[Affine, ElasticDeformation]``
    (config 2, both forms) on the bench batch, and config 5, the 512^3 multi-modal subject (2 x float32 + int16 label map,
    nearest for the labels).  Every leg draws the SAME per-instance parameters (the generator is re-seeded in front of the
    warm-up and of the timed steps: VERDICT r5 weak #8 — freshly drawn boxes differ from leg to leg) and times 20 steps."""
    from parity_harness import nested_spheres  # noqa: PLC0415

    affine = dict(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5))
    fused = tio.Spatial(**affine, max_displacement=7.5)
    two_resamples = tio.Compose([tio.Affine(**affine), tio.ElasticDeformation()])  # config 2's second form ("report both")
    volume = size**3 * 4
    out: dict = {}
    previous = tio.get_resample_precision()

    def timed(transform, data, steps):
        result = None
        torch.manual_seed(4242)
        for _ in range(10):  # (new shapes: the caching allocator needs a few steps to settle on its blocks)
            result = transform(data)
        torch.cuda.synchronize()
        torch.manual_seed(4243)
        timer.pairs, timer.active = [], True
        start = time.perf_counter()
        for _ in range(steps):
            result = transform(data)
        torch.cuda.synchronize()
        elapsed = (time.perf_counter() - start) / steps
        timer.active = False
        del result
        return elapsed, timer.mean_ms()

    try:
        for precision in ("tight", "exact"):
            tio.set_resample_precision(precision)
            seconds, launch_ms = timed(fused, batch, 20)
            nbytes = 2 * volume * batch.batch_size
            out[f"fused_spatial,{precision}"] = {
                "volumes_per_s": batch.batch_size / seconds, "ms_per_step": 1e3 * seconds, "launch_ms": launch_ms,
                "launch_frac": nbytes / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if launch_ms else None,
            }
            seconds, launch_ms = timed(two_resamples, batch, 20)
            out[f"compose_affine_elastic,{precision}"] = {
                "volumes_per_s": batch.batch_size / seconds, "ms_per_step": 1e3 * seconds, "launch_ms": launch_ms,
                "launch_frac": nbytes / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if launch_ms else None,
            }
        big = 2 * size
        g = torch.Generator(device=device).manual_seed(5)
        subject = tio.SubjectsBatch({
            "t1": tio.ImagesBatch(torch.rand(1, 1, big, big, big, generator=g, device=device), [tio.AffineMatrix()], image_class=tio.ScalarImage),
            "t2": tio.ImagesBatch(torch.rand(1, 1, big, big, big, generator=g, device=device) + 1, [tio.AffineMatrix()], image_class=tio.ScalarImage),
            "seg": tio.ImagesBatch(nested_spheres(big).unsqueeze(0).to(device), [tio.AffineMatrix()], image_class=tio.LabelMap),
        })
        nbytes = 2 * (2 * 4 + 2) * big**3
        for precision in ("tight", "exact"):
            tio.set_resample_precision(precision)
            seconds, launch_ms = timed(fused, subject, 20)
            out[f"config5_{big}^3_2xf32+i16,{precision}"] = {
                "subjects_per_s": 1 / seconds, "ms_per_step": 1e3 * seconds, "launch_ms": launch_ms,
                "step_frac": nbytes / seconds / 1e9 / HBM_PEAK_GBS,
            }
    finally:
        tio.set_resample_precision(previous)
    return out


def load_pmc(key: str) -> float | None:
    """A per-launch figure of the dominant kernel from the committed PMC summary (profiles/resample_traffic.json), if any:
    ``hbm_bytes_per_launch_<precision>`` (FETCH_SIZE / WRITE_SIZE passes) or ``valu_insts_per_launch_<precision>`` (SQ_INSTS_VALU)."""
    path = os.path.join(ROOT, "profiles", "resample_traffic.json")
    try:
        with open(path) as handle:
            return float(json.load(handle)[key])
    except (OSError, KeyError, ValueError):
        return None


def compact(value, digits: int = 4):
    """Floats to *digits* significant digits, recursively: the line must survive the driver's 8 KB tail."""
    if isinstance(value, float):
        return float(f"{value:.{digits}g}")
    if isinstance(value, dict):
        return {key: compact(item, digits) for key, item in value.items()}
    if isinstance(value, (list, tuple)):
        return [compact(item, digits) for item in value]
    return value


# wave64 vector instructions a SIMD issues per clock at best (SIMD-32: two cycles each — MI355X_MICROARCH.md), SIMDs, clock
VALU_CYCLES_PER_INST, N_SIMDS, CLOCK_HZ = 2.0, 256 * 4, 2.4e9
# ... and what tests/native/valu_rates.cpp measured on this chip with three to four resident waves per SIMD (cycles per wave64 instruction per
# SIMD at the nominal clock, profiles/r01_valu_rates_w1-8.log): float32 add / mul / fma, and everything else (floor, conversions, integer
# multiplies, min / max, compares, selects, moves, DPP)
VALU_CYCLES_FAST_CLASS, VALU_CYCLES_OTHER = 2.9, 4.6


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=50)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--batch", type=int, default=8, help="volumes per GPU per step")
    parser.add_argument("--noise-rng", choices=["reference", "philox"], default="philox")
    parser.add_argument("--resample-precision", choices=["exact", "tight"], default="tight",
                        help="tight (default here, like --noise-rng philox: the throughput mode) = the reference's coordinates, taps and fill "
                             "decisions bit for bit, fused interpolation: inside the north-star bar PER VOXEL; exact = the library default, the "
                             "reference's float32 operation sequence bit for bit.  With --full the other modes are timed as well (mode_matrix) "
                             "unless --no-mode-matrix")
    parser.add_argument("--prewarm", type=int, default=100, help="untimed process pre-warm calls before the W warm-up steps")
    parser.add_argument("--settle-seconds", type=float, default=8.0, help="upper bound of the untimed settling phase after the pre-warm")
    parser.add_argument("--no-cpu-baseline", action="store_true")
    parser.add_argument("--cpu-volumes", type=int, default=8)
    parser.add_argument("--no-aten-baseline", action="store_true", help="--full: skip the stock-ATen restatement of the pipeline (the honest 'before')")
    parser.add_argument("--no-other-configs", action="store_true", help="--full: skip the fused tio.Spatial and config-5 (512^3 subject) legs (rank 0, N=1 only)")
    parser.add_argument("--no-mode-matrix", action="store_true", help="--full: skip the extra noise-rng / resample-precision legs (rank 0, N=1 only)")
    parser.add_argument("--full", action="store_true",
                        help="besides the headline: the roofline (HIP events around every resample launch of the timed steps), and with "
                             "N=1 the mode matrix, multi-stream, the other configurations, the stock-ATen and CPU baselines and the "
                             "measured HBM ceiling (each of those can still be left out with its --no-* switch)")
    parser.add_argument("--dump-outputs", metavar="DIR", default=None,
                        help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32 / float64)")
    args = parser.parse_args()

    info = tdist.init_process_group()
    pinned_cpus = tdist.pin_host_threads(info)  # N ranks on one host: each on its share of its GPU's NUMA node (no-op for N = 1)
    assert info.world_size == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={info.world_size}"
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    device = torch.device("cuda", info.local_rank)
    torch.cuda.set_device(device)
    warnings.simplefilter("ignore")

    tio.set_noise_rng(args.noise_rng)
    tio.set_resample_precision(args.resample_precision)
    tio.set_stencil_precision(stencil_mode(args.resample_precision))  # the Blur's taps: fused multiply-adds in the throughput modes
    engine = ops.engine()
    timer = KernelTimer(engine, "resample3d") if args.full else None  # (events inside the timed steps: --full only)
    transform = build_transform()
    batch = make_batch(args.size, args.batch, 1234 + info.rank, device)
    torch.manual_seed(4321 + info.rank)

    # Process pre-warm (untimed set-up, before the W warm-up steps the caller asked for): the first ~100
    # calls of a fresh process are ~30 % slower on the host side (pinned staging allocator, dispatcher and
    # Python caches still growing).  Same batch and shapes as the timed steps, so a profiler's per-kernel
    # averages over the whole process stay comparable with the live numbers below.
    # (every untimed loop below keeps its latest output alive exactly like the timed loop does — `out = transform(batch)` —
    # so that the caching allocator has reached the timed loop's steady state, one more 0.5 GB block than a loop that drops
    # its result at once, before the clock starts: a first `hipMalloc` inside the timed region synchronises the device and
    # showed up as 1.8 ms of "host" time per step instead of 1.2)
    out = None
    for _ in range(args.prewarm):
        out = transform(batch)
    torch.cuda.synchronize()
    # ... and a fresh BOX can stay slow on the host side for seconds (its image is still paging in: the same step has been
    # seen to take 1.85 ms of host time instead of 1.22, which makes the step host bound): keep stepping, untimed, until
    # the host time of a block of steps stops improving (two blocks within 3 % of the best so far) or the budget is spent.
    settle_log, best, calm = [], float("inf"), 0
    settle_deadline = time.perf_counter() + args.settle_seconds
    while calm < 2 and time.perf_counter() < settle_deadline:
        t0 = time.perf_counter()
        for _ in range(20):
            out = transform(batch)
        host_ms = 1e3 * (time.perf_counter() - t0) / 20
        torch.cuda.synchronize()
        settle_log.append(round(host_ms, 3))
        calm = calm + 1 if 0.97 * best <= host_ms <= 1.03 * best else 0  # neither improving any more nor an outlier
        best = min(best, host_ms)
    torch.manual_seed(4321 + info.rank)
    for _ in range(args.warmup):
        out = transform(batch)
    torch.cuda.synchronize()
    tdist.barrier()
    torch.cuda.synchronize()
    if timer is not None:
        timer.active = True
    start = time.perf_counter()
    for _ in range(args.steps):
        out = transform(batch)
    host_enqueue_s = time.perf_counter() - start  # host time to issue all steps (no sync inside the loop)
    torch.cuda.synchronize()
    tdist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    if timer is not None:
        timer.active = False
    if args.dump_outputs:
        # (every rank writes its own files: the budget is shared, so N ranks stay within what one writes)
        dump_outputs(out, args.dump_outputs, f"_rank{info.rank}" if info.world_size > 1 else "", DUMP_BUDGET_BYTES // info.world_size)

    volume_bytes = args.size**3 * 4
    n_volumes = args.steps * args.batch
    counters = tdist.gather_counters(n_volumes, elapsed, n_volumes * 10 * volume_bytes, device=device)
    total = tdist.aggregate_throughput(counters)

    if info.rank == 0:
        kernel_ms = timer.mean_ms() if timer is not None else None
        launch_bytes = 2 * volume_bytes * args.batch  # read input once + write output once, per launch
        achieved = launch_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms else None
        precision = args.resample_precision
        # the vector-issue floor beside the HBM one: SQ_INSTS_VALU of the dominant kernel (committed PMC pass) at the SIMD's best
        # rate — what the launch could not go below whatever the memory system does
        valu_insts = load_pmc(f"valu_insts_per_launch_{precision}")
        valu = None
        if valu_insts:
            floor_ms = 1e3 * valu_insts * VALU_CYCLES_PER_INST / (N_SIMDS * CLOCK_HZ)
            valu = {"insts_per_voxel": valu_insts * 64 / (args.batch * args.size**3), "floor_ms": floor_ms,
                    "frac_of_issue": floor_ms / kernel_ms if kernel_ms else None}
            fast_class = load_pmc(f"valu_fast_class_insts_per_launch_{precision}")  # (SQ_INSTS_VALU_ADD_F32 + MUL_F32 + FMA_F32)
            if fast_class:
                issue_ms = 1e3 * (fast_class * VALU_CYCLES_FAST_CLASS + (valu_insts - fast_class) * VALU_CYCLES_OTHER) / (N_SIMDS * CLOCK_HZ)
                valu.update({"fast_class_share": fast_class / valu_insts, "issue_ms_at_measured_rates": issue_ms,
                             "frac_at_measured_rates": issue_ms / kernel_ms if kernel_ms else None})
        roofline = {
            "kernel": "tio::resample_lean_exact_kernel<EXACT_LERP=%s> + plan_bricks_kernel (tio_resample3d: mean of the Affine and ElasticDeformation launches)"
                      % ("true" if precision == "exact" else "false"),
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": (achieved / HBM_PEAK_GBS) if achieved else None,
            "traffic": load_pmc(f"hbm_bytes_per_launch_{precision}"),
            "launch_ms": kernel_ms, "algorithmic_bytes_per_launch": launch_bytes, "launches_timed": len(timer.pairs) if timer is not None else 0,
            "valu": valu,
        }
        extras: dict = {}
        single = args.gpus == 1 and args.full  # (the legs beyond the headline, rank 0 of one GPU: --full only)
        if single and not args.no_mode_matrix:
            # The headline value is the mode named in config.  The other modes of the same pipeline:
            #   noise "reference" = the reference's own stream, bit for bit (the library's default); "philox" = in-kernel draws;
            #   resample "exact" = bit-identical coordinates AND interpolation (default); "tight" = bit-identical coordinates /
            #   taps / fill decisions, fused interpolation (per-voxel 1e-4).  Every row names the draw policy it ran under.
            out = None
            modes = {}
            library_policy = tio.get_draw_policy()

            def row(rng_mode, prec, steps, policy=None, plan=None):
                result = time_mode(transform, batch, steps, noise_rng=rng_mode, precision=prec, seed=77, timer=timer, launch_bytes=launch_bytes, draw_policy=policy,
                                   noise_plan=plan)
                if rng_mode == "reference":
                    result["draws"] = policy or tio.get_draw_policy()
                    result["plan"] = plan or ("device" if ops.noise_plan_on_device() else "host")
                return result

            for prec in ("tight", "exact"):
                modes[f"philox,{prec}"] = row("philox", prec, 20)
            # The reference's own noise stream: WHERE its draw kernel runs is a box-dependent trade: every
            # policy is timed, and `ops.calibrate_draw_policy` — the library's run-time choice — picks the one behind
            # `value_reference_identical`.  The process-wide policy is restored afterwards.
            for policy in ("gated", "free", "off"):
                modes[f"reference,exact,draws={policy}"] = row("reference", "exact", 30, policy)
            previous_mode = (tio.get_noise_rng(), tio.get_resample_precision(), tio.get_stencil_precision())
            try:
                tio.set_noise_rng("reference"); tio.set_resample_precision("exact"); tio.set_stencil_precision("exact")
                calibration = ops.calibrate_draw_policy(lambda: transform(batch))
            finally:
                tio.set_noise_rng(previous_mode[0]); tio.set_resample_precision(previous_mode[1]); tio.set_stencil_precision(previous_mode[2])
            chosen = tio.get_draw_policy()
            try:
                modes["reference,exact"] = row("reference", "exact", 30, chosen)
                modes["reference,tight"] = row("reference", "tight", 30, chosen)
                # the state chain of the reference's stream on the DEVICE (what `auto` selects when several ranks share a host)
                modes["reference,exact,plan=device"] = row("reference", "exact", 30, chosen, "device")
            finally:
                tio.set_draw_policy(library_policy)
            extras["mode_matrix"] = modes
            extras["draw_policy"] = {"chosen": chosen, "calibration_ms_per_step": calibration}
            # the number that sits beside the reference itself: the LIBRARY DEFAULT — the reference's own noise stream bit for
            # bit + the bit-exact resamplers (the headline `value` is the throughput mode named in `config`)
            extras["value_reference_identical"] = modes["reference,exact"]["volumes_per_s"]
            out = None
            torch.manual_seed(78)
            extras["multi_stream"] = {f"{n}_streams": multi_stream(transform, batch, 40, n) for n in (2, 3)}
        if single and not args.no_other_configs:
            out = None
            extras["other_configs"] = other_configs(batch, args.size, device, timer)
        if single and not args.no_aten_baseline:
            out = None
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            extras["aten_baseline"] = aten_baseline(args.size, min(args.batch, 2), device)
        if single:
            out = None
            torch.cuda.empty_cache()
            extras["hbm_measured_ceiling_GBps"] = hbm_measured_ceiling(device)
            if achieved:
                roofline["frac_of_measured_copy"] = achieved / extras["hbm_measured_ceiling_GBps"]["d2d_copy_GBps"]
        if single and not args.no_cpu_baseline:
            # `cpu_baseline` is the stated baseline of the tier: the reference's CPU op sequence on this box's host cores
            # (all cores, 32 threads, one thread); the C / OpenMP oracle ("port" of the arithmetic, the parity checker) next to it
            extras["cpu_baseline"] = cpu_reference_ops_baseline(args.size, 99)
            extras["cpu_baseline_reference_recorded"] = recorded_reference_timing()
            extras["cpu_baseline_oracle_port"] = cpu_baseline(args.size, args.cpu_volumes, 99, budget_s=8.0)
        # ---- the line: numbers first, in the order a reader needs them; prose lives in DESIGN.md (§2 parity coverage per mode,
        # §5 what every leg is) ------------------------------------------------------------------------------------------------
        line = {
            "metric": "volumes/s (256^3 float32) for Compose[affine+elastic+bias+blur+noise]",
            "value": total["volumes_per_s"],
            "unit": "volumes/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * total["elapsed_s"] / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"Compose[Affine(+-10deg,0.9-1.1,+-5mm),ElasticDeformation(7^3cp,7.5mm),BiasField,Blur(0.5-2mm),Noise] on 1x{args.size}^3 f32, per-instance params",
                "batch_per_gpu": args.batch, "global_batch": args.batch * args.gpus,
                "noise_rng": args.noise_rng, "resample_precision": precision, "stencil_precision": stencil_mode(precision),
                "parallelism": f"batch-split x{args.gpus} (no data-path collective)",
            },
            "value_reference_identical": extras.get("value_reference_identical"),
            "host_enqueue_ms_per_step": 1e3 * host_enqueue_s / args.steps,
        }
        if args.full:
            line["roofline"] = roofline
        other = extras.get("other_configs")
        if other and other.get(f"fused_spatial,{precision}", {}).get("launch_ms"):
            fused_row = other[f"fused_spatial,{precision}"]
            # the kernel north_star names: ONE tio_resample3d launch for affine + elastic (tio.Spatial), same batch
            line["roofline_fused_spatial"] = {
                "bound": "hbm", "achieved": launch_bytes / (fused_row["launch_ms"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": fused_row["launch_frac"], "launch_ms": fused_row["launch_ms"],
            }
        if "cpu_baseline" in extras:
            line["cpu_baseline"] = extras["cpu_baseline"]
            # BASELINE.md holds no published number for this metric, so `vs_baseline` stays null (the bench contract); the ratios
            # to the CPU path measured here are reported under their own names
            line["vs_cpu_reference_ops"] = {
                "headline_over_best_leg": line["value"] / line["cpu_baseline"]["value"],
                "reference_identical_over_best_leg": (extras.get("value_reference_identical") or 0.0) / line["cpu_baseline"]["value"] or None,
            }
        for key in ("mode_matrix", "other_configs", "multi_stream", "draw_policy", "hbm_measured_ceiling_GBps", "aten_baseline",
                    "cpu_baseline_reference_recorded", "cpu_baseline_oracle_port"):
            if key in extras:
                line[key] = extras[key]
        line["pipeline_algorithmic_GBps"] = total["algorithmic_bytes"] / total["elapsed_s"] / 1e9
        line["distributed"] = {
            "backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
            "world_size": info.world_size, "counters_shape": list(counters.shape),
            "per_rank_volumes_per_s": [float(row[0] / row[1]) if row[1] > 0 else None for row in counters.tolist()],
            "host_threads_per_rank": tdist.host_thread_budget(), "noise_plan": "device" if ops.noise_plan_on_device() else "host",
            "rank0_pinned_cpus": len(pinned_cpus) if pinned_cpus else None,
        }
        line["host_settling_ms_per_step"] = settle_log[-4:]  # untimed blocks of 20 steps before the warm-up: the host side of a fresh box
        line["docs"] = "DESIGN.md: §2 parity coverage per mode, §5 what every leg measures"
        print(json.dumps(compact(line), separators=(",", ":")), flush=True)
    del out
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
