"""GPU: ``bias_kernel``, ``noise_kernel``, ``philox_normal_kernel``, ``gamma_kernel`` and ``min_reduce_kernel`` on the cases of
``intensity_pointwise_cases.py`` — every result against the float64 reference at the derived bar (module docstring there),
and against the CPU oracle at the bars ``test_gpu_ops_parity.py`` uses.  ``test_intensity_pointwise_host.py`` runs the same
list through the oracle."""
from __future__ import annotations

import pytest
import torch

import intensity_pointwise_cases as cases
from torchio_amd.ops import EngineError

pytestmark = pytest.mark.gpu

DEV = "cuda"


# -- Philox ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("seed", "stream_id", "n"), cases.PHILOX_CASES)
def test_philox_normal(oracle, hip, seed, stream_id, n):
    gpu = cases.check_philox(hip, DEV, seed, stream_id, n)
    cpu = oracle.philox_normal((n,), seed, stream_id, "cpu")
    d = (gpu - cpu).abs()
    assert float(d.max()) <= 2e-6 and float((d / cpu.abs().clamp_min(1.0)).max()) <= 5e-7


def test_philox_streams_are_uncorrelated(hip):
    cases.check_philox_streams_are_uncorrelated(hip, DEV)


def test_philox_normal_ends_inside_a_block(hip):
    """n = 1, 2, 3, 5 end inside a Philox block: the scalar stores of the last thread, the same stream."""
    z, _ = cases.philox_normal_reference(0, 0, 4003)
    whole = hip.philox_normal((4003,), 0, 0, DEV).cpu()
    for n in (1, 2, 3, 5):
        assert torch.equal(hip.philox_normal((n,), 0, 0, DEV).cpu(), whole[:n])
    assert float((whole.double() - z).abs().max()) <= cases.PHILOX_ABS


# -- BiasField ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", cases.BIAS_IDS)
def test_bias(oracle, hip, case_id):
    gpu = cases.check_bias(hip, DEV, case_id)
    data, coarse, skip = cases.bias_inputs(case_id)
    divide = cases.BIAS_CASES[cases.BIAS_IDS.index(case_id)][4]
    cpu = oracle.bias_field_apply(data, coarse, divide=divide, skip=skip)
    torch.testing.assert_close(gpu, cpu, rtol=cases.ORACLE_RTOL[data.dtype], atol=0)


def test_bias_refuses_a_grid_beyond_the_launch_limit(hip):
    """``grid.z`` = 8 tiles x 8192 = 65536: refused loudly, nothing launched — and the engine works on after it."""
    shape, extents = cases.BIAS_TOO_LARGE
    data = torch.ones(shape, device=DEV)
    coarse = torch.zeros(*shape[:2], *extents, device=DEV)
    with pytest.raises(EngineError, match="too large"):
        hip.bias_field_apply(data, coarse)
    torch.cuda.synchronize()
    cases.check_bias(hip, DEV, "one-voxel")


# -- Noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "rician", "dtype"), cases.NOISE_CASES, ids=cases.NOISE_IDS)
def test_noise_philox(oracle, hip, name, rician, dtype):
    gpu = cases.check_noise_philox(hip, DEV, name, rician, dtype)
    data, mean, std, keep, seed = cases._noise_setup(name, dtype)
    cpu = oracle.add_noise(data, mean, std, rician=rician, philox_seed=seed, keep=keep)
    # test_philox_stream_and_fast_noise: 1e-6 absolute (Rician with explicit draws: 1e-6 relative on top); 16-bit storage can
    # round the two float32 results to neighbouring values: one ulp of the storage type
    ulp = {torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}.get(dtype, 0.0)
    torch.testing.assert_close(gpu.double(), cpu.double(), rtol=(1e-6 if rician else 0.0) + ulp, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_noise_explicit_draws_16bit(oracle, hip, dtype):
    gpu = cases.check_noise_explicit_16bit(hip, DEV, dtype)
    cpu = cases.check_noise_explicit_16bit(oracle, "cpu", dtype)
    assert cases.same_bits(gpu, cpu)


# -- Gamma -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exponent", cases.GAMMA_EXPONENTS, ids=str)
@pytest.mark.parametrize("dtype", cases.GAMMA_DTYPES, ids=str)
def test_gamma(oracle, hip, dtype, exponent):
    gpu = cases.check_gamma(hip, DEV, dtype, exponent)
    gamma = torch.tensor(exponent, dtype=torch.float32) if isinstance(exponent, tuple) else exponent
    cpu = oracle.gamma_pow(cases.gamma_inputs(dtype), gamma)
    torch.testing.assert_close(gpu, cpu, rtol=cases.ORACLE_RTOL[dtype], atol=cases.GAMMA_FLOOR[dtype], equal_nan=True)


# -- channel_min -------------------------------------------------------------------------------------------------------------
def test_channel_min_large(hip):
    cases.check_channel_min_large(hip, DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.float16], ids=str)
def test_channel_min_scalar_loop(hip, dtype):
    cases.check_channel_min_scalar_loop(hip, DEV, dtype)


def test_channel_min_values(hip):
    cases.check_channel_min_values(hip, DEV)


def test_channel_min_workspace_growth(hip):
    cases.check_channel_min_workspace_growth(hip, DEV)
