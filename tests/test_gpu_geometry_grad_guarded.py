"""GPU: ``tio_resample3d_geometry_grad`` between guards (``guarded_memory.py``): the images, the incoming gradients, the mapping, the
control points and the fills carved 16-byte aligned (skew 0) and one element off (skew 1), both outputs and the workspace carved by
the engine's own allocations.  Afterwards every guard byte is intact, every output element is written, and the values meet the
bound of ``test_gpu_geometry_grad.py``.  The case has partial waves, partial row groups and partial slabs (9 x 5 x 70), a fill, and an
elastic component, so that every address computation of the kernel runs: taps, gradients, control reads, LDS box, flush, finish."""
from __future__ import annotations

import pytest
import torch

import geometry_grad_reference as reference
from adjoint_reference import _launch_arguments
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("name", ["8-ko70", "5-out-of-bounds-fill"])
def test_the_geometry_gradient_stays_inside_its_buffers(hip, name, skew):
    case = reference.case(name)
    arena = Arena()
    geo = {key: carve_like(value, arena, "cuda", skew, key) if isinstance(value, torch.Tensor) else value for key, value in case["geo"].items()}
    images = [carve_like(x, arena, "cuda", skew, "image") for x in case["images"]]
    grads = [carve_like(g, arena, "cuda", skew, "grad") for g in case["grads"]]
    fills = [None if f is None else carve_like(f, arena, "cuda", skew, "fill") for f in case["fills"]]
    carved = len(arena.carves)
    with guarded_engine_allocations(arena):
        d_mapping, d_control = hip.resample3d_geometry_grad(images, grads, fills=fills, **_launch_arguments(geo))
    torch.cuda.synchronize()
    assert len(arena.carves) == carved + 3 and arena.owns(d_mapping) and arena.owns(d_control)  # two outputs and the workspace
    arena.check_guards()
    assert_written(d_mapping, "d_mapping")
    assert_written(d_control, "d_control")
    for original, carved_input in zip(case["images"] + case["grads"], images + grads, strict=True):
        assert torch.equal(original, carved_input.cpu())  # the inputs are read, never written
    reference.check(case, d_mapping, d_control)
