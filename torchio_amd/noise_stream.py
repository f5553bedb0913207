"""The reference-identical noise stream: ``torch.randn`` from one seeded CPU generator, restated on all host cores and on the
device (``HostNormalStream``), who runs its mt19937 state chain (``set_noise_plan``), and the pinned buffers its plans and
draws are staged in (``PinnedRing``).  ``ops`` re-exports the public names.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import threading
import warnings

import torch
from torch import Tensor

from . import _abi
from . import _lib
from ._autograd import _AttachBackward
from ._autograd import _wants_grad
from ._lib import EngineError
from .distributed import cached_host_thread_budget
from .streams import _device_index
from .streams import draw_stream
from .streams import on_draw_stream

# Who runs the mt19937 state chain of the reference's noise stream (round 6):
#   "host"    this rank's worker threads, by jump-ahead (0.6 ms per 134 M draws on 32 threads of an idle host, overlapped with the
#             enqueue work of a Compose that draws ahead; 4.8 - 5.7 ms on the 15 threads a rank has when eight share a host);
#   "device"  the device (csrc/mt19937.hip: tio_mt19937_device_snapshots — one workgroup per segment jumps and chains, ~0.1 ms
#             beside whatever else runs); the host writes a 5 KB prefix;
#   "auto"    "device" when several ranks share this host (LOCAL_WORLD_SIZE > 1), else "host".
_NOISE_PLANS = ("auto", "host", "device")


def _noise_plan_from_env() -> str:
    value = os.environ.get("TIO_NOISE_PLAN", "auto")
    if value not in _NOISE_PLANS:
        raise ValueError(f"TIO_NOISE_PLAN must be one of {_NOISE_PLANS}, got {value!r}")
    return value


_NOISE_PLAN = _noise_plan_from_env()


def set_noise_plan(where: str) -> None:
    """Where the state chain of the reference's noise stream is run: ``"host"``, ``"device"`` or ``"auto"`` (see above).  The
    draws are the same bits either way (tests/test_gpu_device_rng.py)."""
    global _NOISE_PLAN
    if where not in _NOISE_PLANS:
        raise ValueError(f"noise plan must be one of {_NOISE_PLANS}, got {where!r}")
    _NOISE_PLAN = where


def get_noise_plan() -> str:
    return _NOISE_PLAN


def noise_plan_on_device() -> bool:
    if _NOISE_PLAN == "auto":
        try:
            return int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > 1
        except ValueError:
            return False
    return _NOISE_PLAN == "device"


def _device_rng_enabled() -> bool:
    """``TIO_DEVICE_RNG=0`` keeps every draw on the host road (read at call time: tests and A/B runs flip it between calls)."""
    return os.environ.get("TIO_DEVICE_RNG", "1") != "0"


def _raw_stream(device: torch.device) -> C.c_void_p:
    """The current HIP stream of *device* as the C ABI takes it."""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(_device_index(device)))


class _PinnedBuffer:
    """One pinned host tensor, the event of its last upload, and whether a native plan job holds it."""

    __slots__ = ("tensor", "event", "lent")

    def __init__(self, tensor: Tensor, event) -> None:
        self.tensor = tensor
        self.event = event
        self.lent = False

    def lend(self) -> None:
        """Busy from now on: no upload event guards the buffer until its holder has called ``release``."""
        self.lent = True

    def release(self) -> None:
        self.lent = False

    def uploaded(self) -> None:
        """Called behind the asynchronous copy that reads the buffer: it is free again once that copy has completed."""
        self.event.record()

    def free(self) -> bool:
        # (`query()` is True for an event that was never recorded — a buffer handed to a native plan job by
        # `prefetch_plan` has no recorded upload yet, so a second request of the same size, before the first plan is collected,
        # used to get the SAME buffer: two Noise children of one Compose then shared a plan.  Such a buffer is `lent` until the
        # job has been ended.)
        return not self.lent and self.event.query()


def _pinned(size: int, dtype) -> Tensor:
    return torch.empty(size, dtype=dtype, pin_memory=True)


class PinnedRing:
    """Pinned host buffers of one dtype (allocating 512 MiB of pinned memory costs ~0.2 s): kept PER THREAD — a buffer is
    written by the host and read by an asynchronous upload, and ``Queue``'s workers draw concurrently (a ring shared between
    threads handed two of them the same buffer: one's raw state words went up as the other's "draws") —, per device (an event
    belongs to the device it is first recorded on) and per size, at most ``length`` per size used in turn, each guarded by
    the event of its last upload."""

    SIZES = 4  # distinct sizes kept per thread and device

    def __init__(self, dtype, length: int, allocate=_pinned, event=torch.cuda.Event) -> None:
        self.dtype, self.length = dtype, length
        self._allocate, self._event = allocate, event
        self._threads = threading.local()

    def _sizes(self, device: int) -> dict[int, list[_PinnedBuffer]]:
        if not hasattr(self._threads, "per_device"):
            self._threads.per_device = {}
        return self._threads.per_device.setdefault(device, {})

    def buffers(self, device: int) -> list[_PinnedBuffer]:
        """Every buffer the calling thread keeps for *device*."""
        return [buffer for ring in self._sizes(device).values() for buffer in ring]

    def take(self, size: int, device: int) -> _PinnedBuffer:
        """A buffer of *size* elements that nobody reads or writes any more, for the calling thread on *device* (an index)."""
        sizes = self._sizes(device)
        ring = sizes.setdefault(size, [])
        if len(sizes) > self.SIZES:  # (a few distinct sizes at most: drop the rest)
            # (never a buffer a native plan job still owns — its upload event is recorded later; a ring keeps such
            # buffers and is dropped at a later call)
            for other in [key for key in sizes if key != size]:
                kept = [buffer for buffer in sizes[other] if buffer.lent]
                if kept:
                    sizes[other] = kept
                else:
                    del sizes[other]
        for buffer in ring:
            if buffer.free():
                return buffer
        if len(ring) < self.length or all(buffer.lent for buffer in ring):
            buffer = _PinnedBuffer(self._allocate(size, self.dtype), self._event())
            ring.append(buffer)
            return buffer
        buffer = next(buffer for buffer in ring if not buffer.lent)
        buffer.event.synchronize()
        return buffer


_PLAN_RING = PinnedRing(torch.int32, 3)
_STAGING_RING = PinnedRing(torch.float32, 2)


@dataclasses.dataclass
class _PlanAhead:
    """A plan started ahead of its launch (``prefetch_plan``): the native job owns the stream's state and *buffer*."""

    count: int
    device: torch.device
    buffer: _PinnedBuffer
    handle: int


class HostNormalStream:
    """``torch.Generator().manual_seed(seed)`` + ``torch.randn(shape, generator=...)`` on all host cores, bit for bit
    (``tio_host_mt19937_*``, csrc/host_rng.cpp), delivered on the device.

    The reference's Noise draws from ONE seeded CPU generator, call after call (noise.py:108-116); torch produces that
    stream on a single thread (0.35 s for 8 x 256^3 values).  Large draws for the device are made ON the device
    (``_randn_on_device``: the host only runs the mt19937 state chain and uploads a snapshot every 128 blocks); the host
    road — the chain on one thread, everything else on the others, into pinned memory, the upload of a chunk overlapping
    the generation of the next one — serves host tensors, small draws and streams that stand inside a group of 16.
    """

    CHUNK = 16 * (1 << 20)  # values per upload (64 MiB; a multiple of 16: only the last chunk can carry torch's tail rule)

    # Whose `torch` allocates the stream's tensors.  They are engine allocations like `Engine`'s own, so `ops` points this at
    # ITS view of torch, looked up call by call (tests/guarded_memory.py swaps that view to carve every allocation from a
    # guard-banded arena); `ops` imports this module, not the other way round.
    _torch = staticmethod(lambda: torch)

    def __init__(self, seed: int) -> None:
        _, functions = _lib.load()
        self._fn = functions
        self._state = (C.c_uint64 * (_abi.HOST_MT_STATE_BYTES // 8))()
        status = functions["host_mt19937_seed"](C.addressof(self._state), int(seed) & (2**64 - 1))
        if status != _abi.OK:
            raise EngineError(f"tio_host_mt19937_seed failed with status {status}")
        threads = os.environ.get("TIO_HOST_RNG_THREADS")
        # (default: this rank's share of the host — LOCAL_WORLD_SIZE ranks per host, the affinity mask —, at most 32)
        self.threads = int(threads) if threads else cached_host_thread_budget()

    _self_check: bool | None = None  # does the restated stream equal THIS torch build's? (checked once per process)

    @classmethod
    def verified(cls) -> bool:
        """The restatement is tied to the arithmetic of torch's CPU ``normal_`` (mt19937 + the 16-lane Box-Muller of
        ``normal_fill_16_AVX2`` with ``avx_mathfun.h``'s polynomials: torch 2.10 on AVX2 hosts).  Another torch build or a host
        without AVX2 may take another path, so the first use draws 4 096 values both ways from one seed — a microsecond-scale
        check — and on ANY difference the stream is switched off for the process: ``takes`` then answers False and the
        callers keep ``torch.randn`` (slow, and by definition the reference's stream)."""
        if cls._self_check is None:
            try:
                _, functions = _lib.load()
                state = (C.c_uint64 * (_abi.HOST_MT_STATE_BYTES // 8))()
                ok = functions["host_mt19937_seed"](C.addressof(state), 20260922) == _abi.OK
                ours = torch.empty(4096 + 48, dtype=torch.float32)
                for start, length in ((0, 4096), (4096, 48)):  # a continuation too: the state must end up where torch's does
                    ok = ok and functions["host_mt19937_randn"](C.addressof(state), C.c_void_p(ours.data_ptr() + 4 * start), length, 1) == _abi.OK
                generator = torch.Generator().manual_seed(20260922)
                theirs = torch.cat([torch.randn(4096, generator=generator), torch.randn(48, generator=generator)])
                cls._self_check = bool(ok and torch.equal(ours.view(torch.int32), theirs.view(torch.int32)))
            except Exception:  # noqa: BLE001 - whatever went wrong, the answer is "not verified"
                cls._self_check = False
            if not cls._self_check:
                warnings.warn(
                    "torchio_amd: the restated CPU normal stream differs from this torch build's torch.randn; reference-identical "
                    "noise falls back to torch.randn on the host (slow)", RuntimeWarning, stacklevel=2)
        return cls._self_check

    @classmethod
    def takes(cls, shape) -> bool:
        """torch uses another algorithm below 16 values (not restated): such draws stay with ``torch.randn`` — and so does
        everything when the stream could not be verified against this torch build (``verified``)."""
        return math.prod(shape) >= 16 and cls.verified()

    DEVICE_DRAW_MIN = 1 << 20  # draws from which the device produces the stream itself (below: the host road's one small upload)

    def randn(self, shape, device) -> Tensor:
        shape = tuple(int(extent) for extent in shape)
        count = math.prod(shape)
        device = torch.device(device)
        on_gpu = device.type == "cuda"
        on_device_road = on_gpu and count >= self.DEVICE_DRAW_MIN and _device_rng_enabled()
        ahead = self._prefetched
        if ahead is not None and not (on_device_road and count == ahead.count and device == ahead.device):
            self._end_plan_ahead()
            raise EngineError("HostNormalStream: a plan was started ahead for a draw that is not the next one")
        if on_device_road:
            out = self._randn_on_device(count, device)
            if out is not None:
                return out.view(shape)
        if on_gpu:  # (the uploads and the event that frees the staging buffer belong to the DATA's device and its current stream)
            with torch.cuda.device(device):
                return self._randn_via_host(count, device).view(shape)
        return self._randn_via_host(count, device).view(shape)

    def _randn_via_host(self, count: int, device) -> Tensor:
        on_gpu = device.type == "cuda"
        staging = _STAGING_RING.take(count, torch.cuda.current_device()) if on_gpu else None
        host = staging.tensor if on_gpu else self._torch().empty(count, dtype=torch.float32)
        out = self._torch().empty(count, dtype=torch.float32, device=device) if on_gpu else host
        for start in range(0, count, self.CHUNK):
            stop = min(start + self.CHUNK, count)
            if count - stop < 16 and stop != count:
                stop = count  # (never leave a last chunk of fewer than 16 values)
            status = self._fn["host_mt19937_randn"](C.addressof(self._state), C.c_void_p(host.data_ptr() + 4 * start), stop - start, self.threads)
            if status != _abi.OK:
                raise EngineError(f"tio_host_mt19937_randn failed with status {status}")
            if on_gpu:
                out[start:stop].copy_(host[start:stop], non_blocking=True)
            if stop == count:
                break
        if on_gpu:
            staging.uploaded()
        return out

    _prefetched: _PlanAhead | None = None

    def prefetch_plan(self, count: int, device) -> None:
        """Start the plan of the NEXT ``count`` draws of this stream on a native thread (``tio_host_mt19937_plan_begin``: the
        state chain runs on this rank's worker threads, no interpreter lock involved) while the caller goes on enqueueing; the
        next ``_device_plan(count, device)`` — whoever asks first: the fused Noise kernel or ``randn`` — collects it.  Called
        by ``Noise._prefetch`` from a ``Compose`` that drew its children's parameters ahead: the seed is known one millisecond
        of host work before the noise kernel is launched."""
        if self._prefetched is not None or count < self.DEVICE_DRAW_MIN or not _device_rng_enabled():
            return
        if noise_plan_on_device() and count % 16 == 0:
            return  # (the device runs the chain: the host's part is a 5 KB prefix, written when the plan is asked for)
        device = torch.device(device)
        words = int(self._fn["host_mt19937_plan_words"](count))
        with torch.cuda.device(device):
            buffer = _PLAN_RING.take(words, torch.cuda.current_device())
        buffer.lend()
        handle = int(self._fn["host_mt19937_plan_begin"](C.addressof(self._state), count, C.c_void_p(buffer.tensor.data_ptr()), words, self.threads))
        if handle != 0:
            self._prefetched = _PlanAhead(count, device, buffer, handle)
        else:
            buffer.release()

    def _end_plan_ahead(self, used: C.c_int64 | None = None):
        """End the native job of a plan started ahead, if there is one (the state is the job's until it has returned), and take
        its buffer back from it: returns the record and the job's status.  With *used* the plan is handed on (the words it
        takes are written there; the caller uploads it and calls ``buffer.uploaded()``), without it the plan is abandoned."""
        ahead, self._prefetched = self._prefetched, None
        if ahead is None:
            return None, _abi.OK
        status = self._fn["host_mt19937_plan_end"](ahead.handle, None if used is None else C.byref(used))
        ahead.buffer.release()
        return ahead, status

    def __del__(self):  # a job that nobody collected still owns the state and the staging buffer: wait for it
        if getattr(self, "_prefetched", None) is not None:
            self._end_plan_ahead()

    def _device_plan(self, count: int, device):
        """The plan of ``count`` draws (``tio_host_mt19937_plan``: the host runs the mt19937 state chain — in parallel, by
        jump-ahead — and keeps a snapshot every 128 blocks), uploaded: 2.5 KB of state per 79 872 draws instead of 4 bytes
        per draw.  ``None`` when the stream stands inside a group of 16 (the host road takes over; the state is untouched)."""
        used = C.c_int64(0)
        ahead, status = self._end_plan_ahead(used)
        if ahead is not None:
            if ahead.count != count or ahead.device != torch.device(device):
                raise EngineError(f"HostNormalStream: a plan of {ahead.count} draws on {ahead.device} was started ahead, {count} on {device} are asked for")
            buffer = ahead.buffer
        else:
            if noise_plan_on_device():
                made = self._device_made_plan(count, device)
                if made is not None:
                    return made
            words = int(self._fn["host_mt19937_plan_words"](count))
            buffer = _PLAN_RING.take(words, torch.cuda.current_device())
            status = self._fn["host_mt19937_plan"](C.addressof(self._state), count, C.c_void_p(buffer.tensor.data_ptr()), words, C.byref(used), self.threads)
        if status == _abi.UNSUPPORTED_CONFIG:
            return None
        if status != _abi.OK:
            raise EngineError(f"tio_host_mt19937_plan failed with status {status}")
        plan_dev = self._torch().empty(used.value, dtype=torch.int32, device=device)
        plan_dev.copy_(buffer.tensor[: used.value], non_blocking=True)
        buffer.uploaded()
        return buffer.tensor, plan_dev

    # segment polynomials on the device: {(device index, segment_blocks): (count, tensor)} — 2.5 KB per segment, made by the host
    # once per segment length (tens of milliseconds: polynomial products) and uploaded once
    _segment_polynomials: dict = {}
    _SEGMENTS = 224  # workgroups of the snapshot kernel to aim for (one per CU; a segment is a power of two of 128-block units)

    def _device_made_plan(self, count: int, device):
        """The plan with its snapshots made ON the device (``set_noise_plan("device")``): the host writes the prefix (header,
        rest of the current block, snapshot 0 — ``tio_host_mt19937_plan_prefix``) and leaves its own state owing the twists;
        ``tio_mt19937_device_snapshots`` jumps to every segment's first state and chains through it.  ``None`` (state
        untouched) where that form does not apply: the caller makes the whole plan on the host."""
        prefix_words, used, total_blocks = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        buffer = _PLAN_RING.take(2048, torch.cuda.current_device())
        plan_host = buffer.tensor
        status = self._fn["host_mt19937_plan_prefix"](C.addressof(self._state), count, C.c_void_p(plan_host.data_ptr()), 2048,
                                                      C.byref(prefix_words), C.byref(used), C.byref(total_blocks))
        if status == _abi.UNSUPPORTED_CONFIG:
            return None
        if status != _abi.OK:
            raise EngineError(f"tio_host_mt19937_plan_prefix failed with status {status}")
        device = torch.device(device)
        index = _device_index(device)
        blocks = total_blocks.value
        segment = 128
        while segment * self._SEGMENTS < blocks:
            segment *= 2
        n_segments = (blocks + segment - 1) // segment
        polys = None
        if n_segments > 1:
            cached = HostNormalStream._segment_polynomials.get((index, segment))
            if cached is None or cached[0] < n_segments - 1:
                need = max(n_segments - 1, self._SEGMENTS)
                host = self._torch().empty(need * 624, dtype=torch.int32)
                status = self._fn["host_mt19937_segment_polynomials"](segment, need, C.c_void_p(host.data_ptr()))
                if status != _abi.OK:
                    raise EngineError(f"tio_host_mt19937_segment_polynomials failed with status {status}")
                cached = (need, host.to(device))
                HostNormalStream._segment_polynomials[(index, segment)] = cached
            polys = cached[1]
        plan_dev = self._torch().empty(used.value, dtype=torch.int32, device=device)
        plan_dev[: prefix_words.value].copy_(plan_host[: prefix_words.value], non_blocking=True)
        buffer.uploaded()
        status = self._fn["mt19937_device_snapshots"](C.c_void_p(plan_dev.data_ptr()), blocks, segment,
                                                      None if polys is None else C.c_void_p(polys.data_ptr()), _raw_stream(device))
        if status != _abi.OK:
            raise EngineError(f"tio_mt19937_device_snapshots failed with status {status}")
        # (the consumers read the HEADER from the host copy — magic, units, tail flag, n — while the kernels read the device's:
        # a private copy, the ring buffer goes back to the ring)
        return plan_host[:16].clone(), plan_dev

    def can_draw_ahead(self, shape, device) -> bool:
        """Can :meth:`randn_ahead` take these draws?  (Nothing is drawn; a stream that stands inside a group of 16 still
        declines later — the caller then draws with :meth:`randn`.)"""
        count = math.prod(shape)
        device = torch.device(device)
        ahead = self._prefetched
        return not (
            draw_stream(device) is None or count < self.DEVICE_DRAW_MIN or not _device_rng_enabled()
            or (ahead is not None and (count != ahead.count or device != ahead.device))
        )

    def randn_ahead(self, shape, device) -> Tensor | None:
        """The next draws of this stream, made on the device's DRAW stream (``draw_stream``) instead of the data's: the kernel
        that turns the plan into normal draws is bound by vector arithmetic (torch's Box-Muller, ~135 instructions per pair)
        and depends on nothing but the plan, so it runs next to the memory-bound kernels of the data stream — the resamplers
        and the stencil's first pass of this step, or, with the host running ahead, of the step before.  The current stream is
        ordered behind the draws (an event: no host wait) and the buffer is handed over to it.  ``None`` (nothing drawn, the
        state untouched) when this road does not apply; the caller then draws with :meth:`randn` / :meth:`add_noise`."""
        if not self.can_draw_ahead(shape, device):
            return None
        shape = tuple(int(extent) for extent in shape)
        count = math.prod(shape)
        device = torch.device(device)
        out = on_draw_stream(device, lambda: self._randn_on_device(count, device))
        return None if out is None else out.view(shape)

    def _randn_on_device(self, count: int, device) -> Tensor | None:
        """The draws made on the device (``tio_mt19937_randn_device``) from the host's plan of the state chain."""
        with torch.cuda.device(device):
            plan = self._device_plan(count, device)
            if plan is None:
                return None
            out = self._torch().empty(count, dtype=torch.float32, device=device)
            status = self._fn["mt19937_randn_device"](
                C.c_void_p(plan[0].data_ptr()), C.c_void_p(plan[1].data_ptr()), C.c_void_p(out.data_ptr()), _raw_stream(device)
            )
        if status != _abi.OK:
            raise EngineError(f"tio_mt19937_randn_device failed with status {status}")
        return out

    def add_noise(self, data: Tensor, mean, std) -> Tensor | None:
        """``data + (mean + std * randn(data.shape))`` in ONE kernel (``tio_mt19937_add_noise_device``): the draws of this stream
        never exist in memory.  *data*: a dense float32 ``(B, ...)`` device tensor; *mean* / *std*: numbers or ``(B,)`` float32
        device tensors.  ``None`` (nothing drawn) when this form does not apply: the caller draws with :meth:`randn`."""
        count = data.numel()
        if (
            not data.is_cuda or data.dtype != torch.float32 or not data.is_contiguous() or count < self.DEVICE_DRAW_MIN
            or data.shape[0] < 1 or not _device_rng_enabled()
        ):
            return None
        per_element = count // data.shape[0]
        if (isinstance(mean, Tensor) or isinstance(std, Tensor)) and per_element < 624:
            return None  # (per-element parameters: the kernel wants elements of at least one state block)
        for vector in (mean, std):  # per-element parameters as the kernel reads them: (B,) float32 next to the data
            if isinstance(vector, Tensor) and (
                vector.device != data.device or vector.dtype != torch.float32 or vector.numel() != data.shape[0]
                or not vector.is_contiguous() or vector.requires_grad
            ):
                return None
        if _wants_grad(data):  # additive: dy/dx = 1 (as Engine.add_noise)
            result = self.add_noise(data.detach(), mean, std)
            return None if result is None else _AttachBackward.apply(data, result, lambda grad: grad)
        device = data.device
        with torch.cuda.device(device):
            plan = self._device_plan(count, device)
            if plan is None:
                return None
            out = self._torch().empty_like(data)
            mean_dev = mean if isinstance(mean, Tensor) else None
            std_dev = std if isinstance(std, Tensor) else None
            status = self._fn["mt19937_add_noise_device"](
                C.c_void_p(plan[0].data_ptr()), C.c_void_p(plan[1].data_ptr()), C.c_void_p(data.data_ptr()), C.c_void_p(out.data_ptr()), per_element,
                0.0 if mean_dev is not None else float(mean), 0.0 if std_dev is not None else float(std),
                C.c_void_p(mean_dev.data_ptr()) if mean_dev is not None else None, C.c_void_p(std_dev.data_ptr()) if std_dev is not None else None,
                _raw_stream(device),
            )
        if status != _abi.OK:
            raise EngineError(f"tio_mt19937_add_noise_device failed with status {status}")
        return out
