"""The pinned staging buffers of the reference's noise stream (``noise_stream.PinnedRing``), rule by rule, without a GPU: a
fake allocator and fake events whose completion the test controls.  Each case restates a finding recorded in the ring's
comments.
"""
from __future__ import annotations

import threading

import torch

from torchio_amd.noise_stream import PinnedRing


class FakeEvent:
    """``torch.cuda.Event`` as the ring uses it: never recorded counts as complete (that is what ``query()`` answers), a recorded
    one is complete when the test says so — or when somebody waits for it."""

    def __init__(self) -> None:
        self.pending = False
        self.waits = 0

    def record(self) -> None:
        self.pending = True

    def query(self) -> bool:
        return not self.pending

    def synchronize(self) -> None:
        self.waits += 1
        self.pending = False

    def complete(self) -> None:
        self.pending = False


def _ring(length: int):
    allocated = []

    def allocate(size, dtype):
        allocated.append(torch.empty(size, dtype=dtype))
        return allocated[-1]

    return PinnedRing(torch.int32, length, allocate=allocate, event=FakeEvent), allocated


def test_a_lent_buffer_without_a_recorded_upload_is_not_handed_out_again():
    """an event that was never recorded answers "complete"; only `lent` says that a native plan job writes the buffer."""
    ring, allocated = _ring(3)
    first = ring.take(100, 0)
    assert ring.take(100, 0) is first  # (not lent, nothing recorded: nobody uses it)
    first.lend()
    assert first.event.query()
    second = ring.take(100, 0)
    assert second is not first and second.tensor is not first.tensor and len(allocated) == 2
    assert second.tensor.numel() == 100 and second.tensor.dtype == torch.int32


def test_a_pending_upload_gets_another_buffer_and_a_full_ring_waits_for_the_first_that_is_not_lent():
    ring, allocated = _ring(2)
    first = ring.take(64, 0)
    first.uploaded()
    second = ring.take(64, 0)
    assert second is not first
    second.uploaded()
    assert first.event.waits == 0 and second.event.waits == 0
    assert ring.take(64, 0) is first and first.event.waits == 1 and len(allocated) == 2  # full: waited on the host, no third buffer
    first.lend()
    second.uploaded()
    assert ring.take(64, 0) is second and second.event.waits == 1 and first.event.waits == 1  # (the first one is the job's)
    first.release()
    first.uploaded()
    second.uploaded()
    second.event.complete()
    assert ring.take(64, 0) is second and second.event.waits == 1  # a completed upload is found without waiting


def test_with_every_buffer_lent_the_ring_grows_beyond_its_length():
    ring, allocated = _ring(2)
    held = []
    for _ in range(2):
        held.append(ring.take(32, 0))
        held[-1].lend()
    third = ring.take(32, 0)
    assert all(third is not buffer for buffer in held) and len(allocated) == 3
    assert [buffer.event.waits for buffer in held] == [0, 0]


def test_a_fifth_size_drops_the_other_sizes_but_never_a_lent_buffer():
    """a ring was dropped while a native job still owned one of its buffers."""
    ring, allocated = _ring(3)
    for size in (10, 20, 30, 40):
        ring.take(size, 0)
    lent = ring.take(20, 0)
    lent.lend()
    assert len(ring.buffers(0)) == 4
    fifth = ring.take(50, 0)
    assert ring.buffers(0) == [lent, fifth] or ring.buffers(0) == [fifth, lent]
    lent.release()
    lent.uploaded()
    lent.event.complete()
    assert ring.take(20, 0) is lent and len(allocated) == 5
    assert ring.take(10, 0) not in (lent, fifth) and len(allocated) == 6  # (a dropped size starts over)


def test_a_buffer_of_a_dropped_ring_can_still_record_its_upload_and_is_not_kept():
    """The event lives with the buffer: a table of events keyed by buffer identity lost the entry when the ring was dropped, and
    the callers that might still hold such a buffer re-created it with `setdefault` — an entry nothing ever removed."""
    ring, allocated = _ring(3)
    early = ring.take(10, 0)
    for size in (20, 30, 40, 50):
        ring.take(size, 0)
    assert early not in ring.buffers(0)
    early.uploaded()  # the caller that still holds it
    assert early.event.pending
    assert early not in ring.buffers(0)
    assert ring.take(10, 0) is not early


def test_rings_are_per_thread_and_per_device():
    ring, allocated = _ring(3)
    taken = {}

    def worker(name):
        taken[name] = ring.take(16, 0)

    threads = [threading.Thread(target=worker, args=(name,)) for name in ("a", "b")]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join()
    mine = ring.take(16, 0)
    assert len({id(taken["a"]), id(taken["b"]), id(mine)}) == 3 and len(allocated) == 3
    assert ring.buffers(0) == [mine]  # (the other threads' buffers are theirs)
    assert ring.take(16, 1) is not mine and ring.take(16, 0) is mine
