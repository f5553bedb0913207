"""GPU: the four parameter-gradient entry points between guards (``guarded_memory.py``): the data, the incoming gradient, the
parameters, the draws and the flags carved 16-byte aligned (skew 0) and one element off (skew 1); the outputs, the workspace and
the tap gradient's two scratch volumes carved by the engine's own allocations.  Afterwards every guard byte is intact, every output
element is written, the inputs are unchanged, and the values equal the unguarded launch's (the two-run rule) and meet the bound of
``test_gpu_param_grad.py``.  The cases have partial waves, partial row groups and partial slabs, a box and a direct bias tile in one
launch, rows that do not start on a Philox block, and every stencil intermediate of the tap gradient."""
from __future__ import annotations

import pytest
import torch

import param_grad_reference as reference
from guarded_memory import Arena
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations
from param_grad_reference import TAU

pytestmark = pytest.mark.gpu


def _same(first, second) -> bool:
    first, second = first.detach().cpu().double(), second.detach().cpu().double()
    return first.shape == second.shape and bool(((first - second).abs() <= torch.maximum(first.abs(), second.abs()) * 2.0 ** -23).all())


def _carved(case, arena, skew, names):
    return {name: None if case[name] is None else carve_like(case[name], arena, "cuda", skew, name) for name in names}


def _finish(arena, case, inputs, outputs, carved_before, engine_carves):
    torch.cuda.synchronize()
    assert len(arena.carves) == carved_before + engine_carves and all(arena.owns(out) for out in outputs)
    arena.check_guards()
    for label, out in enumerate(outputs):
        assert_written(out, f"output {label}")
    for name, tensor in inputs.items():
        assert tensor is None or torch.equal(case[name], tensor.cpu()), name  # the inputs are read, never written


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("name", ["box-limit-beyond", "float16"])
def test_the_bias_gradient_stays_inside_its_buffers(hip, name, skew):
    case, arena = reference.bias_case(name), Arena()
    t = _carved(case, arena, skew, ["x", "gy", "coarse", "skip"])
    before = len(arena.carves)
    with guarded_engine_allocations(arena):
        got = hip.bias_field_grad(t["x"], t["gy"], t["coarse"], divide=case["divide"], skip=t["skip"])
    _finish(arena, case, t, [got], before, 2)  # the output and the workspace
    reference.check(f"guarded bias {name} skew {skew}", got, case["ref"], case["a"], case["c"], TAU)
    plain = hip.bias_field_grad(case["x"].cuda(), case["gy"].cuda(), case["coarse"].cuda(), divide=case["divide"], skip=None if case["skip"] is None else case["skip"].cuda())
    assert _same(got, plain)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("name", ["batched-4099", "bfloat16"])
def test_the_gamma_gradient_stays_inside_its_buffers(hip, name, skew):
    case, arena = reference.gamma_case(name), Arena()
    t = _carved(case, arena, skew, ["x", "gy", "gamma"])
    before = len(arena.carves)
    with guarded_engine_allocations(arena):
        got = hip.gamma_grad(t["x"], t["gy"], t["gamma"])
    _finish(arena, case, t, [got], before, 2)
    reference.check(f"guarded gamma {name} skew {skew}", got, case["ref"], case["a"], reference.C_GAMMA, TAU)
    assert _same(got, hip.gamma_grad(case["x"].cuda(), case["gy"].cuda(), case["gamma"].cuda()))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("name", ["additive-keep", "rician-scalar", "rician-float64"])
def test_the_noise_gradients_stay_inside_their_buffers(hip, name, skew):
    case, arena = reference.noise_case(name), Arena()
    t = _carved(case, arena, skew, ["x", "gy", "mean", "std", "z1", "z2", "keep"])
    before = len(arena.carves)
    with guarded_engine_allocations(arena):
        d_mean, d_std = hip.noise_grad(t["x"], t["gy"], t["mean"], t["std"], rician=case["rician"], base1=t["z1"], base2=t["z2"], keep=t["keep"])
        philox = hip.noise_grad(t["x"], t["gy"], t["mean"], t["std"], rician=case["rician"], philox_seed=5, keep=t["keep"])
    _finish(arena, case, t, [d_mean, d_std, *philox], before, 6)  # twice: two outputs and the workspace
    c_mean, c_std = reference.noise_c(case)
    reference.check(f"guarded noise {name} skew {skew} d_mean", d_mean, *case["mean_ref"], c_mean, 0.0)
    reference.check(f"guarded noise {name} skew {skew} d_std", d_std, *case["std_ref"], c_std, 0.0)
    plain = hip.noise_grad(case["x"].cuda(), case["gy"].cuda(), case["mean"].cuda(), case["std"].cuda(), rician=case["rician"], philox_seed=5,
                           keep=None if case["keep"] is None else case["keep"].cuda())
    assert _same(philox[0], plain[0]) and _same(philox[1], plain[1])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("name", ["r16-1-8", "skip-wide-stride", "bfloat16"])
def test_the_tap_gradient_stays_inside_its_buffers(hip, name, skew):
    case, arena = reference.taps_case(name), Arena()
    t = _carved(case, arena, skew, ["x", "gy", "taps", "skip"])
    before = len(arena.carves)
    with guarded_engine_allocations(arena):
        got = hip.separable_conv3d_taps_grad(t["x"], t["gy"], t["taps"], case["radius"], skip=t["skip"])
    _finish(arena, case, t, [got], before, 3)  # the output, the two scratch volumes (one allocation) and the workspace
    reference.check(f"guarded taps {name} skew {skew}", got, case["ref"], case["a"], case["c"], 0.0)
    plain = hip.separable_conv3d_taps_grad(case["x"].cuda(), case["gy"].cuda(), case["taps"].cuda(), case["radius"], skip=None if case["skip"] is None else case["skip"].cuda())
    assert _same(got, plain)
