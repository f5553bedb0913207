"""Forced delays on GPU streams (a helper module: no tests are collected from it; tests/test_gpu_stream_order.py uses it).

On an idle GPU a side stream's few microseconds of work are always over before the data stream reaches their consumer, so a
missing ``wait_event``, a missing ``record_stream`` or a ring buffer reused one upload too early passes every comparison.
A *hold* keeps one stream busy for a known time; whatever is enqueued behind it runs late, and an ordering that is missing
becomes a wrong result instead of a lucky one.

* ``hold(stream, ms)``: work on *stream* that ends by itself after about *ms*; the returned object says whether it is still
  ``in_force()``.
* ``independent_stream(side, device)``: a stream that really runs beside *side* (the process has a handful of hardware
  queues: two torch streams can share one, and then a hold on one also stalls the other and proves nothing), chosen by the
  *teeth probe* on plain torch ops.
* ``watch(engine, names)``: records, for every watched C call, the stream it was enqueued on and which holds were in force
  at that moment.
"""
from __future__ import annotations

import contextlib
import time

import pytest
import torch

MAX_HOLD_MS = 500.0  # one hold never exceeds this: a request beyond it raises
FLOOR_HOLD_MS = 20.0
PROBE_HOLD_MS = 20.0
MAX_CANDIDATES = 8

# what the test file writes into its report (profiles/stream_order.md): the calibration, the chosen stream pairs
CALIBRATION: dict = {}
PAIRS: list[dict] = []


class Hold:
    """Work enqueued on *stream* that keeps it busy; ``end`` is recorded right behind it."""

    __slots__ = ("stream", "ms", "end", "label")

    def __init__(self, stream, ms: float, end, label: str) -> None:
        self.stream, self.ms, self.end, self.label = stream, ms, end, label

    def in_force(self) -> bool:
        return not self.end.query()


def hold_length(enqueue_ms: float) -> float:
    """Four times what the host took to enqueue the same work in the plain pass, at least ``FLOOR_HOLD_MS``, at most the cap
    (a cap that is too short shows as a launch recorded outside the hold: the in-force assertion of the test then says so)."""
    return min(max(4.0 * enqueue_ms, FLOOR_HOLD_MS), MAX_HOLD_MS)


def _timed(stream, enqueue) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record(stream)
        enqueue()
        end.record(stream)
    end.synchronize()
    return float(start.elapsed_time(end))


def _calibrate(device) -> dict:
    """Once per process and device: what the argument of ``torch.cuda._sleep`` counts on this runtime, from event timings at
    two lengths (the second four times the first).  Where the two are not roughly proportional, holds are made of repeated
    elementwise passes over a large tensor instead, timed the same way."""
    key = torch.device(device).index or 0
    if key in CALIBRATION:
        return CALIBRATION[key]
    stream = torch.cuda.Stream(device=device)
    record: dict = {"primitive": None}
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        with torch.cuda.device(device):
            _timed(stream, lambda: sleep(1000))  # (the first launch loads the kernel)
            cycles, short = 1_000_000, 0.0
            for _ in range(6):  # a first length of at least 2 ms: launch overhead (microseconds) does not bend the ratio
                short = _timed(stream, lambda: sleep(cycles))
                if short >= 2.0 or short <= 0.0:
                    break
                cycles *= 4
            long = _timed(stream, lambda: sleep(4 * cycles)) if 0.0 < short <= MAX_HOLD_MS / 4 else 0.0
        record.update(sleep_cycles=(cycles, 4 * cycles), sleep_ms=(short, long))
        if short >= 2.0 and 3.2 <= long / short <= 4.8:
            record.update(primitive="torch.cuda._sleep", per_ms=3 * cycles / (long - short))
    if record["primitive"] is None:
        buffer = torch.zeros(1 << 26, dtype=torch.float32, device=device)  # 256 MiB: one pass reads and writes it all
        with torch.cuda.device(device):
            _timed(stream, lambda: buffer.add_(1.0))
            one = _timed(stream, lambda: [buffer.add_(1.0) for _ in range(8)]) / 8
            other = _timed(stream, lambda: [buffer.add_(1.0) for _ in range(32)]) / 32
        record.update(primitive="elementwise passes over 2^26 floats", per_ms=1.0 / max(one, other), pass_ms=(one, other), buffer=buffer)
    CALIBRATION[key] = record
    return record


def hold(stream, ms: float, label: str = "hold") -> Hold:
    """Keep *stream* busy for about *ms* milliseconds from the moment it gets there.  The work is a kernel that ends by itself:
    it spins on the device's clock (or makes passes over memory), never on a flag the host writes or an event recorded later."""
    if not 0.0 < ms <= MAX_HOLD_MS:
        raise ValueError(f"a hold lasts at most {MAX_HOLD_MS} ms, {ms} were asked for")
    calibration = _calibrate(stream.device)
    with torch.cuda.device(stream.device), torch.cuda.stream(stream):
        if calibration["primitive"] == "torch.cuda._sleep":
            torch.cuda._sleep(int(ms * calibration["per_ms"]))
        else:
            for _ in range(max(1, round(ms * calibration["per_ms"]))):
                calibration["buffer"].add_(1.0)
        end = torch.cuda.Event()
        end.record(stream)
    return Hold(stream, ms, end, label)


def teeth_probe(side, candidate, device) -> dict:
    """Does a hold on *side* leave *candidate* running, and does a ``wait_event`` order it?  Plain torch ops only.

    ``x = zeros(1)``; *side* is held and fills ``x`` with 1 behind the hold; *candidate* clones ``x`` WITHOUT waiting and is
    synchronised alone.  The clone reads 0 while the hold is still in force exactly when the two streams are independent:
    the hold reorders them, and a consumer that forgot to wait would be caught.  With ``wait_event`` the clone reads 1."""
    with torch.cuda.device(device):
        x = torch.zeros(1, device=device)
        torch.cuda.current_stream().synchronize()
        held = hold(side, PROBE_HOLD_MS, "probe")
        with torch.cuda.stream(side):
            x.fill_(1.0)
            filled = side.record_event()
        with torch.cuda.stream(candidate):
            unordered = x.clone()
        candidate.synchronize()
        still_held = held.in_force()
        with torch.cuda.stream(candidate):
            candidate.wait_event(filled)
            ordered = x.clone()
        candidate.synchronize()
        side.synchronize()
        result = dict(unordered=float(unordered.item()), ordered=float(ordered.item()), held_after_unordered=still_held)
    result["independent"] = still_held and result["unordered"] == 0.0
    return result


_CHOSEN: dict = {}


def independent_stream(side, device, *, avoid=(), keep=False):
    """A stream of *device* that a hold on *side* does not stall (and none of *avoid*): up to ``MAX_CANDIDATES`` fresh streams
    are tried with the teeth probe, one alive at a time.  The test FAILS when there is none: nothing it compares would mean
    anything.  *keep*: the choice stays for the process (for the library's own side streams, which every test of a scenario
    shares: the per-stream workspaces of the data stream are then set up once, by the plain pass); without it the stream
    lives as long as the caller holds it, so that no more than a few extra streams are alive at once."""
    device = torch.device(device)
    key = (device.index or 0, side.stream_id, tuple(s.stream_id for s in avoid))
    if keep and key in _CHOSEN:
        return _CHOSEN[key]
    tried = []
    for _ in range(MAX_CANDIDATES):
        candidate = torch.cuda.Stream(device=device)
        if candidate.stream_id == side.stream_id or any(candidate.stream_id == s.stream_id for s in avoid):
            continue
        probe = teeth_probe(side, candidate, device)
        tried.append(probe)
        if probe["independent"]:
            if probe["ordered"] != 1.0:
                pytest.fail(f"a stream ordered behind the held one by wait_event read {probe['ordered']}, not 1: {probe}")
            PAIRS.append(dict(side=side.stream_id, chosen=candidate.stream_id, candidates_tried=len(tried), probe=probe))
            if keep:
                _CHOSEN[key] = candidate
            return candidate
        del candidate
    pytest.fail(f"none of {len(tried)} candidate streams runs beside stream {side.stream_id}: a hold on it stalls them all ({tried})")


class Watch:
    """The watched C calls in enqueue order: ``(name, stream id, {label of a hold: was it in force})``."""

    def __init__(self) -> None:
        self.calls: list[tuple[str, int, dict]] = []
        self.holds: list[Hold] = []

    def add(self, held: Hold) -> Hold:
        self.holds.append(held)
        return held

    def names(self) -> list[str]:
        return [name for name, _, _ in self.calls]

    def of(self, name: str, stream=None) -> list[tuple[str, int, dict]]:
        return [call for call in self.calls if call[0] == name and (stream is None or call[1] == stream.stream_id)]


@contextlib.contextmanager
def watch(engine, names):
    """Wrap the engine's C entry points *names* (``engine._call`` looks them up in ``engine._fn``, and so do the few wrappers
    that call the library directly: ``blur_fused``, the noise stream): every call is recorded at the moment of its enqueue —
    the current stream, and for every hold handed to ``Watch.add`` whether it was still in force — and then made."""
    record = Watch()
    originals = {name: engine._fn[name] for name in names}

    def wrapped(name, function):
        def call(*args):
            record.calls.append((name, torch.cuda.current_stream().stream_id, {held.label: held.in_force() for held in record.holds}))
            return function(*args)

        return call

    for name, function in originals.items():
        engine._fn[name] = wrapped(name, function)
    try:
        yield record
    finally:
        engine._fn.update(originals)


class Stopwatch:
    """Host wall time of the enqueue work between ``start`` and ``stop``, summed (milliseconds)."""

    def __init__(self) -> None:
        self.ms = 0.0
        self._since = 0.0

    def start(self) -> None:
        self._since = time.perf_counter()

    def stop(self) -> None:
        self.ms += 1e3 * (time.perf_counter() - self._since)
