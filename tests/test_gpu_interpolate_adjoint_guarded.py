"""GPU: the three gather adjoints of ``interpolate_adjoint.hip`` in guard-banded and misaligned buffers (``guarded_memory``).

The incoming gradient lies between two ``0xFF`` guards, at skew 1 one element off its 16-byte boundary; the result is carved by
the engine's own allocation.  Afterwards every guard byte is intact, the result equals the unguarded call bit for bit, and NO
element of it still holds the canary: a gather writes every element exactly once into an uninitialised buffer, so a voxel that no
output reads (down-sampling, an unused source of a table) must have been written as zero, not skipped.
"""
from __future__ import annotations

import pytest
import torch

import interpolate_adjoint_reference as ref
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations
from torchio_amd.transforms import anisotropy

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


def _guarded(hip, method: str, grad: torch.Tensor, skew: int, *args):
    plain = getattr(hip, method)(grad.to(DEVICE), *args)
    arena = Arena()
    carved = carve_like(grad, arena, DEVICE, skew, label="gy")
    assert carved.data_ptr() % 16 == (4 * skew) % 16
    with guarded_engine_allocations(arena):
        result = getattr(hip, method)(carved, *args)
    torch.cuda.synchronize()
    arena.check_guards()
    assert arena.owns(result), "the result did not come from the engine's own allocation"
    assert_written(result, method)
    assert torch.equal(result, plain) and torch.equal(carved, grad.to(DEVICE))
    return result


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize(("in_shape", "out_shape"), [((7, 5, 3), (2, 9, 3)), ((9, 10, 70), (4, 5, 33)), ((3, 4, 5), (6, 4, 11)), ((2, 3, 1), (1, 1, 1))],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_interpolate3d_adjoint(hip, in_shape, out_shape, mode, skew):
    result = _guarded(hip, "interpolate3d_adjoint", ref.randn((2, 2, *out_shape), 83), skew, in_shape, mode)
    if mode == "nearest" and all(o < i for i, o in zip(in_shape, out_shape, strict=True) if i > 1):
        assert bool((result == 0).any()), "down-sampling leaves inputs that no output reads: written as zero"


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_gather_lerp_adjoint(hip, axis, mode, skew):
    shape = (5, 6, 67)
    length = shape[axis]
    down_sizes = torch.round(length / torch.tensor([2.5, 1.0, 3.0], dtype=torch.float64)).clamp_min(1).to(torch.long)
    active = torch.tensor([True, False, True])
    if mode == "nearest":
        lower, upper, weight = anisotropy._nearest_source_indices(length, down_sizes), None, None
    else:
        lower, upper, weight = anisotropy._linear_source_indices(length, down_sizes)
    result = _guarded(hip, "axis_gather_lerp_adjoint", ref.randn((3, 2, *shape), 89), skew, axis, lower, upper, weight, active)
    assert bool((result[0] == 0).any()), "a factor of 2.5 leaves sources that no output reads: written as zero"


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
@pytest.mark.parametrize(("in_shape", "padding"), [((3, 4, 2), (2, 1, 0, 3, 1, 1)), ((6, 5, 66), (0, 5, 4, 0, 7, 9))], ids=["3x4x2", "6x5x66"])
def test_pad3d_adjoint(hip, in_shape, padding, mode, skew):
    out_shape = [in_shape[d] + padding[2 * d] + padding[2 * d + 1] for d in range(3)]
    _guarded(hip, "pad3d_adjoint", ref.randn((2, 2, *out_shape), 97), skew, in_shape, padding, mode)
