"""CPU: the guard-banded buffers of ``guarded_memory.py`` checked against themselves, then every guarded case
(``guarded_cases.py``) on the oracle engine at skew 0 and 1 — where the harness is developed; the HIP engine runs the same
table in ``test_gpu_guarded_memory.py``."""
from __future__ import annotations

import pytest
import torch

import guarded_cases
from guarded_cases import CASES
from guarded_cases import run_case
from guarded_memory import GUARD_BYTES
from guarded_memory import Arena
from guarded_memory import GuardError
from guarded_memory import assert_untouched
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations
from torchio_amd import ops


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64])
@pytest.mark.parametrize("skew", [0, 1, 3])
def test_a_carve_holds_the_canary_between_two_guards(dtype, skew):
    arena = Arena()
    view = arena.carve((3, 5, 7), dtype, "cpu", skew, label="probe")
    size = view.element_size()
    assert view.shape == (3, 5, 7) and view.dtype == dtype and view.is_contiguous()
    assert GUARD_BYTES % 512 == 0 and view.data_ptr() == arena.carves[0].raw.data_ptr() + GUARD_BYTES + skew * size
    assert arena.carves[0].raw.numel() == 2 * GUARD_BYTES + (skew + 105) * size
    with pytest.raises(GuardError, match="105 element"):  # NaN for floats, -1 for signed integers, 255 for uint8
        assert_written(view)
    assert_untouched(view)
    arena.check_guards()
    assert arena.owns(view) and arena.owns(view[1]) and not arena.owns(torch.zeros(4))


def test_a_byte_written_into_a_guard_is_reported_with_its_side_and_offset():
    arena = Arena()
    first = arena.carve((4, 6), torch.float32, "cpu", 1, label="first")
    second = arena.carve((10,), torch.int16, "cpu", 0, label="second")
    first.zero_(), second.zero_()
    arena.check_guards()
    raw = arena.carves[0].raw
    start = GUARD_BYTES + 4
    raw[start - 3] = 0  # three bytes in front of the tensor
    with pytest.raises(GuardError, match=r"front guard of first \(shape \(4, 6\), torch.float32\) overwritten: 1 byte\(s\), first at byte offset -3, last at -3"):
        arena.check_guards()
    raw[start - 3] = 0xFF
    raw[start + 96] = 7      # the byte right behind the last element
    raw[start + 96 + 40] = 0
    with pytest.raises(GuardError, match=r"back guard of first .* 2 byte\(s\), first at byte offset 96, last at 136 relative to the tensor \(96 bytes long\)"):
        arena.check_guards()
    raw[start + 96], raw[start + 96 + 40] = 0xFF, 0xFF
    arena.carves[1].raw[-1] = 1  # the very last guard byte of the other allocation
    with pytest.raises(GuardError, match=rf"back guard of second .* first at byte offset {20 + GUARD_BYTES - 1}"):
        arena.check_guards()


def test_an_element_left_at_the_canary_is_reported():
    arena = Arena()
    for dtype in (torch.float32, torch.float16, torch.int16, torch.uint8, torch.int64):
        view = arena.carve((2, 3, 4), dtype, "cpu", 1)
        view.fill_(2)
        assert_written(view)
        view[1, 2, 3] = torch.full((), 0xFF, dtype=torch.uint8).expand(view.element_size()).contiguous().view(dtype)[0]
        with pytest.raises(GuardError, match=r"1 element\(s\) still hold the canary, first at \(1, 2, 3\)"):
            assert_written(view, "probe")
        with pytest.raises(GuardError, match="was written"):
            assert_untouched(view)
    copy = carve_like(torch.arange(24.0).reshape(2, 3, 4), arena, "cpu", skew=1)
    assert torch.equal(copy, torch.arange(24.0).reshape(2, 3, 4)) and copy.data_ptr() % 16 == 4 and arena.owns(copy)


def test_the_shim_carves_only_inside_the_context_and_restores_the_module():
    arena = Arena()
    assert ops.torch is torch
    pattern = torch.ones(2, 3, dtype=torch.float16)
    with guarded_engine_allocations(arena):
        assert ops.torch is not torch and ops.torch.float32 is torch.float32 and ops.torch.cuda is torch.cuda
        a = ops.torch.empty((2, 3), dtype=torch.int16, device="cpu")
        b = ops.torch.empty(7, dtype=torch.float32)
        c = ops.torch.empty_like(pattern)
        d = ops.torch.empty(4, dtype=torch.float32, pin_memory=False)  # a further keyword: the real torch's business
        e = ops.torch.empty_like(pattern, dtype=torch.float32)
        assert torch.empty is not ops.torch.empty  # torch itself is never patched
    assert ops.torch is torch
    assert [arena.owns(t) for t in (a, b, c, d, e)] == [True, True, True, False, False]
    assert (a.shape, a.dtype, b.shape, c.shape, c.dtype) == ((2, 3), torch.int16, (7,), (2, 3), torch.float16)
    assert all(carve.label.startswith("ops.") for carve in arena.carves)
    assert not arena.owns(ops.torch.empty(3))
    with pytest.raises(RuntimeError, match="boom"), guarded_engine_allocations(arena):
        raise RuntimeError("boom")
    assert ops.torch is torch


def test_an_engine_call_allocates_through_the_shim(oracle):
    """``separable_conv3d`` on the oracle: the output and the scratch pair are caught, the result is the unguarded one, and a
    stray byte written behind the output afterwards is reported under the allocation's label."""
    from case_inputs import _data, _taps

    data = _data((1, 1, 6, 7, 9), torch.float32, 5)
    taps, radius = _taps(1, [(0.5, 0.6, 0.7)], 8)
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = oracle.separable_conv3d(carve_like(data, arena, "cpu", 1), taps, radius)
    assert len(arena.carves) == 3 and arena.owns(out)
    arena.check_guards()
    assert_written(out)
    assert torch.equal(out, oracle.separable_conv3d(data, taps, radius))
    owner = next(c for c in arena.carves if c.raw.data_ptr() + c.start == out.data_ptr())
    owner.raw[owner.start + owner.nbytes + 1] = 0
    with pytest.raises(GuardError, match=r"back guard of ops\.separable_conv3d:\d+ \(shape \(1, 1, 6, 7, 9\), torch.float32\) overwritten"):
        arena.check_guards()


_ON_ORACLE = [case for case in CASES if "oracle" in case.engines]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("case", _ON_ORACLE, ids=[case.id for case in _ON_ORACLE])
def test_case_on_the_oracle(oracle, monkeypatch, case, skew):
    guarded_cases._DEVICE[0] = "cpu"
    run_case(case, oracle, "cpu", skew, monkeypatch, oracle)


def test_every_case_has_an_engine_and_the_gpu_only_cases_are_few():
    assert all(case.engines for case in CASES)
    assert [case.id for case in CASES if "oracle" not in case.engines] == [
        "host_stream-randn-1048576", "host_stream-randn-1500003", "host_stream-randn-1050480",
        "host_stream-add_noise-2x1x96x96x96", "host_stream-add_noise-3x2x64x80x71", "resample-folded_minimum",
    ]
