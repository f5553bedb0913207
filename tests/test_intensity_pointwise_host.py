"""The pointwise / reduction cases of ``intensity_pointwise_cases.py`` without a GPU: the numpy Philox4x32-10 against the
published known answers, and every case of the list through the CPU oracle at the bars the GPU is held to — which validates
the float64 references and the bars before a GPU is involved (the oracle shares the kernels' authorship, not the
references')."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import intensity_pointwise_cases as cases


# -- the reference generator itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("counter", "key", "expected"), cases.KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_numpy_philox_reproduces_the_known_answers(counter, key, expected):
    assert tuple(int(word[0]) for word in cases.philox4x32_10(counter, key)) == expected


def test_numpy_philox_is_the_same_function_on_arrays():
    """All three counters at once under one key equal the three single calls (the reference runs on arrays)."""
    counters = [entry[0] for entry in cases.KNOWN_ANSWERS]
    key = cases.KNOWN_ANSWERS[2][1]
    together = cases.philox4x32_10(tuple(np.array([c[w] for c in counters], dtype=np.uint64) for w in range(4)), key)
    for row, counter in enumerate(counters):
        alone = cases.philox4x32_10(counter, key)
        assert [int(word[row]) for word in together] == [int(word[0]) for word in alone]
    assert [int(word[2]) for word in together] == list(cases.KNOWN_ANSWERS[2][2])


def test_uniforms_round_to_one_and_the_reference_gives_zero_there():
    """``fl32(16777215 + 0.5) = 2^24``: the largest word gives ``u1 == 1.0`` exactly, radius 0."""
    top = (np.uint64(0xFFFFFFFF) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)
    assert top.dtype == np.float32 and float(top) * 2.0**-24 == 1.0
    lowest = (np.float32(0) + np.float32(0.5)) * np.float32(2.0**-24)
    assert float(lowest) == 2.0**-25  # the smallest uniform: the radius is at most sqrt(50 ln 2) = 5.89
    for seed, stream_id, n in cases.PHILOX_CASES:
        z, certain_zero = cases.philox_normal_reference(seed, stream_id, n)
        assert z.dtype == torch.float64 and z.shape == (n,) and bool(z.isfinite().all()) and float(z.abs().max()) < 5.9
        assert bool((z[certain_zero] == 0).all())


def test_reference_normals_are_standard_normal():
    z, _ = cases.philox_normal_reference(42, 1, 1 << 22)
    n = z.numel()
    assert abs(float(z.mean())) < 5 / n**0.5 and abs(float(z.var()) - 1) < 5 * (2 / n) ** 0.5  # five sigma of either estimate
    assert abs(float((z**4).mean()) - 3) < 5 * (96 / n) ** 0.5  # Var(z^4) = 105 - 9


def test_bias_bar_follows_its_formula():
    coarse = torch.zeros(1, 1, 3, 1, 2)
    coarse[0, 0, :, 0, 0] = torch.tensor([0.0, 1.0, -1.0])  # steepest step along I: 2, over n_c - 1 = 2; along K: 1, over 1
    expected = cases.EPS * (8 * 1.0 + 4 * (2 * 2.0 + 1 * 1.0)) + 4 * cases.EPS
    assert cases.bias_bar(coarse, torch.float32) == pytest.approx(expected, rel=1e-12)
    assert cases.bias_bar(coarse, torch.float16) == pytest.approx(expected + 2.0**-11, rel=1e-12)
    assert cases.bias_bar(coarse, torch.bfloat16) == pytest.approx(expected + 2.0**-8, rel=1e-12)


def test_large_case_plants_cover_every_unrolled_load():
    deep8, deep4, tail = cases.min_large_plants()
    stride = 4 * cases.MIN_GRID
    assert [p // stride for p in deep8] == list(range(8)) and [p // stride for p in deep4] == [8, 9, 10, 11]
    assert [p // stride for p in tail] == [12, 13, 14, 14] and tail[-1] == 116 * 128 * 512 - 1
    assert {p % 4 for p in deep8 + deep4 + tail} == {0, 1, 2, 3}  # every component of a 16-byte load


# -- every case through the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("seed", "stream_id", "n"), cases.PHILOX_CASES)
def test_oracle_philox_normal(oracle, seed, stream_id, n):
    cases.check_philox(oracle, "cpu", seed, stream_id, n)


def test_oracle_philox_streams_are_uncorrelated(oracle):
    cases.check_philox_streams_are_uncorrelated(oracle, "cpu")


@pytest.mark.parametrize("case_id", cases.BIAS_IDS)
def test_oracle_bias(oracle, case_id):
    cases.check_bias(oracle, "cpu", case_id)


@pytest.mark.parametrize(("name", "rician", "dtype"), cases.NOISE_CASES, ids=cases.NOISE_IDS)
def test_oracle_noise_philox(oracle, name, rician, dtype):
    cases.check_noise_philox(oracle, "cpu", name, rician, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_oracle_noise_explicit_draws_16bit(oracle, dtype):
    cases.check_noise_explicit_16bit(oracle, "cpu", dtype)


@pytest.mark.parametrize("exponent", cases.GAMMA_EXPONENTS, ids=str)
@pytest.mark.parametrize("dtype", cases.GAMMA_DTYPES, ids=str)
def test_oracle_gamma(oracle, dtype, exponent):
    cases.check_gamma(oracle, "cpu", dtype, exponent)


def test_oracle_channel_min_large(oracle):
    cases.check_channel_min_large(oracle, "cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.float16], ids=str)
def test_oracle_channel_min_scalar_loop(oracle, dtype):
    cases.check_channel_min_scalar_loop(oracle, "cpu", dtype)


def test_oracle_channel_min_values_and_workspace(oracle):
    cases.check_channel_min_values(oracle, "cpu")
    cases.check_channel_min_workspace_growth(oracle, "cpu")
