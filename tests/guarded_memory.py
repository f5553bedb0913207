"""Guard-banded test buffers: what a value check cannot see.

Three kinds of error leave every value right: a store beyond an output or scratch buffer (the caching allocator rounds
blocks to 512 bytes and no test shape fills its block, so the stray lands in padding), a voxel that is never written (a
recycled block may still hold the previous, equal result) and a base pointer that is element-aligned but not 16-byte
aligned (a dense view such as ``data[1:]``).  An :class:`Arena` hands out tensors that lie in the middle of a buffer
filled with the byte ``0xFF`` — NaN in every float type, -1 in every signed integer, 255 in ``uint8`` — optionally
shifted by a number of elements; afterwards every guard byte must still be ``0xFF`` and no element of an output may be.

A plain module, imported by the guarded tests only (``tests/guarded_cases.py``); nothing in the product knows it.
"""
from __future__ import annotations

import contextlib
import sys
from dataclasses import dataclass

import torch

CANARY = 0xFF
# Each guard: 256 KiB.  A condition, not a measurement: a multiple of 512 bytes (skew 0 keeps the allocator's own alignment)
# and more than two J x K planes of every guarded case (the largest plane there, 50 x 520 float32, is 104 000 bytes).
GUARD_BYTES = 256 * 1024


class GuardError(AssertionError):
    """A guard byte was overwritten, or an output element was left at the canary."""


@dataclass
class _Carve:
    label: str
    raw: torch.Tensor   # the whole uint8 buffer: front guard, tensor, back guard
    start: int          # byte offset of the tensor inside `raw`
    nbytes: int
    shape: tuple
    dtype: torch.dtype

    def describe(self) -> str:
        return f"{self.label} (shape {self.shape}, {self.dtype})"


def _caller_label(depth: int) -> str:
    frame = sys._getframe(depth)
    return f"{frame.f_code.co_name}:{frame.f_lineno}"


class Arena:
    """Every allocation of one guarded call, with its guards."""

    def __init__(self) -> None:
        self.carves: list[_Carve] = []

    def carve(self, shape, dtype: torch.dtype, device, skew: int = 0, label: str | None = None) -> torch.Tensor:
        """A contiguous ``shape`` / ``dtype`` view whose first element lies ``GUARD_BYTES`` + *skew* ELEMENTS into a fresh
        ``0xFF``-filled buffer and whose last element is followed by ``GUARD_BYTES`` more.  The view itself holds the canary."""
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        count = 1
        for extent in shape:
            count *= extent
        nbytes = count * itemsize
        start = GUARD_BYTES + int(skew) * itemsize
        raw = torch.full((start + nbytes + GUARD_BYTES,), CANARY, dtype=torch.uint8, device=device)
        view = raw[start : start + nbytes].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() == raw.data_ptr() + start
        self.carves.append(_Carve(label or _caller_label(2), raw, start, nbytes, shape, dtype))
        return view

    def owns(self, tensor: torch.Tensor) -> bool:
        return any(c.raw.untyped_storage().data_ptr() == tensor.untyped_storage().data_ptr() for c in self.carves)

    def check_guards(self) -> None:
        """Every guard byte of every carve is still ``0xFF``; else name the allocation, the side and the changed bytes'
        offsets relative to the tensor's first byte (negative in front of it, ``>= nbytes`` behind it)."""
        problems = []
        for c in self.carves:
            for side, lo, hi in (("front", 0, c.start), ("back", c.start + c.nbytes, c.raw.numel())):
                guard = c.raw[lo:hi]
                if bool((guard == CANARY).all()):
                    continue
                changed = torch.nonzero(guard != CANARY).reshape(-1)
                first, last = int(changed[0]) + lo - c.start, int(changed[-1]) + lo - c.start
                problems.append(
                    f"{side} guard of {c.describe()} overwritten: {changed.numel()} byte(s), first at byte offset {first}, "
                    f"last at {last} relative to the tensor ({c.nbytes} bytes long)"
                )
        if problems:
            raise GuardError("; ".join(problems))


def canary_mask(tensor: torch.Tensor) -> torch.Tensor:
    """Elements that (still) read as the canary: NaN for floats, -1 for signed integers, 255 for ``uint8``."""
    if tensor.dtype.is_floating_point:
        return torch.isnan(tensor)
    if tensor.dtype == torch.uint8:
        return tensor == 255
    return tensor == -1


def assert_written(tensor: torch.Tensor, label: str = "output") -> None:
    """No element of *tensor* holds the canary (the cases keep it from being a legitimate result: labels in 0..6, fill values
    neither -1 nor 255, finite float inputs — so a NaN is an unwritten voxel or a guard that entered the arithmetic)."""
    mask = canary_mask(tensor)
    if bool(mask.any()):
        where = torch.nonzero(mask)
        raise GuardError(
            f"{label} (shape {tuple(tensor.shape)}, {tensor.dtype}): {where.shape[0]} element(s) still hold the canary, "
            f"first at {tuple(int(v) for v in where[0])}, last at {tuple(int(v) for v in where[-1])}"
        )


def assert_untouched(tensor: torch.Tensor, label: str = "region") -> None:
    """Every byte of a carved region the kernel promises not to write is still ``0xFF``."""
    raw = tensor.contiguous().view(torch.uint8) if tensor.numel() else tensor
    if tensor.numel() and not bool((raw == CANARY).all()):
        raise GuardError(f"{label} (shape {tuple(tensor.shape)}, {tensor.dtype}) was written: {int((raw != CANARY).sum())} byte(s) changed")


def carve_like(tensor: torch.Tensor, arena: Arena, device, skew: int = 0, label: str | None = None) -> torch.Tensor:
    """A carved (optionally skewed) copy of a case's own input or caller-owned output on *device*."""
    out = arena.carve(tensor.shape, tensor.dtype, device, skew, label or _caller_label(2))
    out.copy_(tensor)
    return out


class _TorchShim:
    """Stands in for the ``torch`` module inside ``torchio_amd.ops``: ``empty`` / ``empty_like`` carve from the arena when the
    request is a plain (shape, dtype, device) one; every other attribute and every request with further keywords
    (``pin_memory=...``) is the real ``torch``'s.  Engine allocations are never skewed: they are fresh allocator blocks in
    real use, and ``plan_dev`` must stay 16-byte aligned by contract."""

    def __init__(self, arena: Arena) -> None:
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kwargs):
        if set(kwargs) - {"dtype", "device"}:
            return torch.empty(*size, **kwargs)
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        dtype = kwargs.get("dtype") or torch.get_default_dtype()
        device = kwargs.get("device")
        return self._arena.carve(shape, dtype, "cpu" if device is None else device, label="ops." + _caller_label(2))

    def empty_like(self, tensor, **kwargs):
        if kwargs or not tensor.is_contiguous():
            return torch.empty_like(tensor, **kwargs)
        return self._arena.carve(tensor.shape, tensor.dtype, tensor.device, label="ops." + _caller_label(2))


@contextlib.contextmanager
def guarded_engine_allocations(arena: Arena):
    """Inside the context every output and scratch tensor of ``Engine`` (``torchio_amd/ops.py``) is carved from *arena*.
    Only the ``ops`` module's view of ``torch`` changes; ``torch`` itself is never patched."""
    from torchio_amd import ops

    real = ops.torch
    ops.torch = _TorchShim(arena)
    try:
        yield arena
    finally:
        ops.torch = real
