"""GPU: ``ghost_lines``, ``complex_abs_max`` / ``spectrum_peak`` and ``add_spikes`` between ``0xFF`` guards
(``guarded_memory.py``): the inputs carved 16-byte aligned (skew 0) and one element off (skew 1), every output tensor of
``ops.py`` carved through the shim.  After each call: the guards are intact, no output element was left unwritten, and the
result is the unguarded call's."""
from __future__ import annotations

import pytest
import torch

import kspace_artefact_cases as cases
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 6, 9, 70), (1, 1, 3, 5, 67), (1, 1, 1, 1, 1)]
DTYPES = [torch.float32, torch.float64, torch.int16, torch.uint8]  # 4-, 8-, 2- and 1-byte elements
ids = lambda shape: "x".join(map(str, shape))  # noqa: E731


def _data(shape, dtype):
    """Whole numbers in [20, 200) (never the canary: 255, -1 or NaN); small strengths keep the results there."""
    return cases.typed_positive(tuple(shape), dtype, len(shape) + shape[-1])


def _guarded(call, inputs, skew, engine_carves):
    """``call(*inputs)`` with every input carved at ``skew`` and the engine's allocations carved; returns the result."""
    arena = Arena()
    with guarded_engine_allocations(arena):
        out = call(*[carve_like(tensor, arena, "cuda", skew) for tensor in inputs])
    assert len(arena.carves) == len(inputs) + engine_carves
    arena.check_guards()
    plain = call(*[tensor.cuda() for tensor in inputs])
    assert arena.owns(out)
    assert_written(out)
    assert out.dtype == plain.dtype and torch.equal(out, plain)
    return out


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("axis", cases.AXES)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_ghost_lines(hip, shape, dtype, axis, skew):
    data = _data(shape, dtype)
    size = shape[2 + axis]
    few, many = sorted({0, size // 3, size - 1}), list(range(size)) + [size // 2] * 9  # one chunk of the kernel; two and more
    for frequencies in (few, many):
        strength = 0.05 if frequencies is few else 0.01  # (ten times the middle frequency: the results stay positive)
        out = _guarded(lambda x: hip.ghost_lines(x, axis, strength, frequencies), [data], skew, 1)  # noqa: B023
        if dtype.is_floating_point:
            expected = cases.ghost_fft(data, [axis] * shape[0], [cases.mask_from_frequencies(size, frequencies, strength)] * shape[0])
            cases.check(out, expected, f"guarded ghost {ids(shape)} {dtype} axis {axis}")
    # per element: another axis, an empty list, a flag
    axes = [axis, (axis + 1) % 3][: shape[0]]
    lists = [few, []][: shape[0]]
    _guarded(lambda x: hip.ghost_lines(x, axes, 0.05, lists), [data], skew, 1)
    flags = torch.tensor([0, 1][: shape[0]], dtype=torch.uint8)
    out = _guarded(lambda x, active: hip.ghost_lines(x, axis, 0.05, few, active), [data, flags], skew, 1)
    assert torch.equal(out[0].cpu(), data[0])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_spectrum_peak_and_add_spikes(hip, shape, dtype, skew):
    data = _data(shape, dtype)
    spatial = shape[2:]
    peaks = _guarded(hip.spectrum_peak, [data], skew, 1)
    assert peaks.cpu().tolist() == pytest.approx(data.double().sum((-3, -2, -1)).reshape(-1).tolist(), rel=1e-5)  # positive input: the DC term
    triples = [tuple(s // 2 for s in spatial), tuple(s - 1 for s in spatial), (0, 0, 0)]
    peaks = peaks.cpu()
    out = _guarded(lambda x, p: hip.add_spikes(x, triples, 0.02, p), [data, peaks], skew, 1)
    if dtype.is_floating_point:
        indices = [tuple((f + s // 2) % s for f, s in zip(triple, spatial, strict=True)) for triple in triples]
        cases.check(out, cases.spike_fft(data, [indices] * shape[0], [0.02] * shape[0])[0], f"guarded spike {ids(shape)} {dtype}")
    lists = [triples[:1], []][: shape[0]]
    flags = torch.tensor([0, 1][: shape[0]], dtype=torch.uint8)
    out = _guarded(lambda x, p, active: hip.add_spikes(x, lists, -0.02, p, active), [data, peaks, flags], skew, 1)
    assert torch.equal(out.cpu(), data)  # flagged off; no spike


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1031])
def test_complex_abs_max(hip, n, skew):
    generator = torch.Generator().manual_seed(n)
    z = torch.complex(torch.randn(3, n, generator=generator), torch.randn(3, n, generator=generator))
    out = _guarded(hip.complex_abs_max, [z], skew, 1)
    assert torch.allclose(out.cpu(), torch.abs(z).amax(1), rtol=3e-7, atol=0)
