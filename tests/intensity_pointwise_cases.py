"""Cases, float64 references and bars of the pointwise / reduction kernels of ``intensity.hip`` — ``bias_kernel``,
``noise_kernel``, ``philox_normal_kernel``, ``gamma_kernel``, ``min_reduce_kernel`` (a plain module, no tests in it).

The module imports neither the oracle nor the engine: every ``check_*`` function takes an engine and a device, so
``tests/test_intensity_pointwise_host.py`` runs the list through the CPU oracle and ``tests/test_gpu_intensity_pointwise.py``
through the HIP engine, against the same references at the same bars.  The references are torch / numpy in float64, written
from each operation's definition (none follows a kernel's structure):

* Bias: ``x.double() * exp(F.interpolate(coarse.double(), size, mode="trilinear", align_corners=True))`` (``/`` to divide).
* Philox: a numpy ``uint64`` Philox4x32-10 (Salmon et al., SC'11), counter ``(q & 0xFFFFFFFF, q >> 32, stream_id, 0)``, key
  ``(seed & 0xFFFFFFFF, seed >> 32)``, block ``q`` giving the elements ``4q .. 4q + 3``.  The uniforms belong to the stream's
  definition and are formed in float32 as the header forms them, ``fl32(fl32(word >> 8) + 0.5) * 2**-24`` (near 1 they
  round: ``u1`` can be exactly 1.0); everything after them is float64: ``r = sqrt(-2 ln u1)``, ``z = r cos(2 pi u2),
  r sin(2 pi u2)`` for the word pairs (0, 1) and (2, 3).  ``test_intensity_pointwise_host.py`` holds the numpy Philox to the
  three published known answers.  The counter's HIGH word is zero in every case: a non-zero one needs more than 2^34
  elements in one call (64 GiB of float32), which no test can allocate, and nothing here pretends to reach it.
* Noise: ``x + (mean + std * z1)``, Rician ``sqrt((x + n1)**2 + n2**2)``; ``z1`` / ``z2`` are the streams 0 / 1 of the Philox
  reference indexed by the element's index in the WHOLE tensor.
* Gamma: ``data.sign() * data.abs().pow(gamma)`` (gamma.py:90) by torch on the CPU, in float64 for the finite values; the
  table of special values is classified (NaN / inf / zero, and the sign) by the same expression in the precision the engine
  computes in — float32 for float32 and bfloat16 storage, float64 for float64 storage (the reference, too, computes float64
  data in float64: 3.4e38 ** 2 is finite there).  The exponent is the float32 the C ABI carries (an input's quantisation).
* channel_min: ``data[0].float().amin(dim=(1, 2, 3))``; NaN compares as NaN, -0 and +0 compare with ``==``.

Bars (derived; none is tuned on a GPU's output).  eps = 2^-24.

* Bias, relative to the reference: ``eps * (8 max|coarse| + 4 sum_axes (n_c - 1) max|d coarse along the axis|) + 4 eps``
  (three nested float32 lerps; the two roundings of ``scale * o`` times the steepest coarse step; ``expf`` and the product)
  plus the half-ulp of the storage type (2^-11 float16, 2^-8 bfloat16).  float16 results below 2^-14 are subnormal: there
  the half-ulp is 2^-25 absolute, which is added for float16 alone.
* Philox normals: ``|d| <= 2.6e-6`` and ``|d| / max(|ref|, 1) <= 7.5e-7`` — the oracle's own distance from the reference
  (5.7e-7 / 2.4e-7: the ``sincos_rev`` truncation plus libm) plus what ``test_philox_stream_and_fast_noise`` grants the GPU
  against the oracle (2e-6 / 5e-7).
* Noise: the Philox bar of the element's draw times ``std``, plus one rounding of the storage type (2^-24, 2^-53, 2^-11,
  2^-8 of ``|ref|``).  Rician has two draws: ``y = sqrt(s^2 + n2^2)`` has ``dy/dn1 = s / y`` and ``dy/dn2 = n2 / y``, so the
  draws' bars enter as ``std * (|s| bar(z1) + |n2| bar(z2)) / y`` (never more than ``std * hypot(bar, bar)``).
* Gamma: 2e-6 relative for float32 / float64, 2e-3 float16, 2^-8 bfloat16 (the project's bars; the last is the half-ulp),
  where a finite result is subnormal, the same 16 float32 ulps (2e-6) at the subnormal ulp, 2^-149 (bfloat16: plus 2^-134).
* Bit-exact, nothing left out: noise with explicit draws, skipped / gated rows, the class and sign of the gamma table,
  channel_min.

Measured on an MI355X (the largest figure over each family's cases; the CPU oracle's next to it):

* Philox normals: max |d| 6.07e-7 of 2.6e-6 (oracle 5.64e-7); max |d| / max(|ref|, 1) 2.60e-7 of 7.5e-7 (oracle 2.40e-7).  Two
  draws each of the streams (1234567890123, 1) and (2^64 - 1, 7) have ``u1 == 1.0``; all four came out as exact zeros.  The
  correlation of the streams 0 and 1 of seed 42 is 2.5e-4 against 2.44e-3.
* Bias: float32 / float64 at most 4.48e-6 relative against a bar of 4.96e-5 (``coarse-larger``; the global-memory case
  3.52e-6 of 4.28e-5) — the oracle's figures to three digits; float16 4.84e-4 of 5.29e-4, bfloat16 3.89e-3 of 3.95e-3 (the
  storage type's half-ulp, as it must be).
* Noise, as a fraction of the per-element bar: Gaussian float32 0.43, float64 0.29, Rician float32 0.83 (oracle 0.83),
  float64 0.24; float16 / bfloat16 0.97 - 0.995 (again the half-ulp of the store).
* Gamma, as a fraction of the bar: float32 0.061 (oracle 0.030: the device's ``powf`` is within two ulps, and ``powf(x, 1)``
  is not exactly ``x`` there), float64 1.1e-10, bfloat16 0.994.  The device's ``powf`` takes subnormal inputs and gives
  subnormal results as torch's does: the table's classes and signs agree in every case, so nothing had to be decided.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0**-24
STORAGE_EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
PHILOX_ABS, PHILOX_REL = 2.6e-6, 7.5e-7
# GPU against the oracle: the bars of tests/test_gpu_ops_parity.py.  bfloat16 is not there: two float32 results 1e-6 apart
# can round to neighbouring bfloat16 values, one ulp = 2^-7 relative (the float16 bar, 2e-3, is the same two-ulp reasoning).
ORACLE_RTOL = {torch.float32: 2e-6, torch.float64: 2e-6, torch.float16: 2e-3, torch.bfloat16: 2.0**-7}

FIGURES: list[tuple[str, float, float]] = []  # (what, measured, bar) of every check of this process, in order


def record(what: str, measured: float, bar: float) -> None:
    """Print a figure before the caller asserts on it (``pytest -s`` shows them; a job script keeps them)."""
    FIGURES.append((what, float(measured), float(bar)))
    print(f"[pointwise] {what}: {float(measured):.4g} (bar {float(bar):.4g})")


def _rand(shape, dtype, seed):
    generator = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=generator) * 4 - 1).to(dtype)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _sync(device) -> None:
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# -- Philox4x32-10 -----------------------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # the two multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85  # the key schedule's Weyl increments (golden ratio, sqrt(3) - 1)
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)

KNOWN_ANSWERS = [  # (counter, key, result): the three vectors of Random123's kat_vectors for philox4x32 with 10 rounds
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key):
    """Ten rounds of Philox4x32 on arrays of counters (four ``uint64`` arrays holding 32-bit words) under ONE key."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(word, dtype=np.uint64)) for word in counter)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=16)
def philox_normal_reference(seed: int, stream_id: int, n: int):
    """``(z, certain_zero)``: the float64 normals of elements ``0 .. n - 1`` and a mask of the draws whose ``u1`` is exactly
    1.0 (radius 0).  Cached: do not modify."""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((blocks & _LOW, blocks >> _32, np.full_like(blocks, stream_id), np.zeros_like(blocks)),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    uniforms = [((word >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-24) for word in words]
    assert all(u.dtype == np.float32 for u in uniforms)
    z = np.empty((blocks.size, 4), dtype=np.float64)
    one = np.zeros((blocks.size, 4), dtype=bool)
    for half in range(2):
        u1, u2 = uniforms[2 * half].astype(np.float64), uniforms[2 * half + 1].astype(np.float64)
        radius = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * half] = radius * np.cos(2.0 * np.pi * u2)
        z[:, 2 * half + 1] = radius * np.sin(2.0 * np.pi * u2)
        one[:, 2 * half] = one[:, 2 * half + 1] = u1 == 1.0
    z = torch.from_numpy(z.reshape(-1)[:n].copy())
    return z + 0.0, torch.from_numpy(one.reshape(-1)[:n].copy())  # (+ 0.0: a radius of -0 reads as 0)


def philox_bar(z: torch.Tensor) -> torch.Tensor:
    """Per draw, the distance the bar allows: both conditions at once."""
    return torch.minimum(torch.full_like(z, PHILOX_ABS), PHILOX_REL * z.abs().clamp_min(1.0))


PHILOX_CASES = [(0, 0, 4003), (1234567890123, 1, 1 << 22), (2**64 - 1, 7, 1 << 22), (42, 1, 1 << 22)]


def check_philox(engine, device, seed, stream_id, n) -> torch.Tensor:
    z, certain_zero = philox_normal_reference(seed, stream_id, n)
    out = engine.philox_normal((n,), seed, stream_id, device)
    _sync(device)
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == (n,)
    assert not bool(out.isnan().any())
    assert bool((out[certain_zero] == 0).all())  # u1 == 1.0: the radius is zero, whatever the angle
    d = (out.double() - z).abs()
    name = f"{device}: philox seed={seed} stream={stream_id} n={n}"
    record(f"{name} u1 == 1 draws", int(certain_zero.sum()), n)
    record(f"{name} max|d|", d.max(), PHILOX_ABS)
    record(f"{name} max|d|/max(|ref|,1)", (d / z.abs().clamp_min(1.0)).max(), PHILOX_REL)
    assert float(d.max()) <= PHILOX_ABS and float((d / z.abs().clamp_min(1.0)).max()) <= PHILOX_REL
    return out


def check_philox_streams_are_uncorrelated(engine, device) -> None:
    """The sample correlation of two independent N(0, 1) streams of n draws is N(0, 1/n): five sigma."""
    n = 1 << 22
    a = engine.philox_normal((n,), 42, 0, device).double().cpu()
    b = engine.philox_normal((n,), 42, 1, device).double().cpu()
    a, b = a - a.mean(), b - b.mean()
    correlation = float((a * b).sum() / (a.norm() * b.norm()))
    record(f"{device}: philox correlation of streams 0 and 1, seed 42", abs(correlation), 5 / math.sqrt(n))
    assert abs(correlation) <= 5 / math.sqrt(n)


# -- BiasField ---------------------------------------------------------------------------------------------------------------
# (id, data shape, coarse extents, dtype, divide, skip)
BIAS_CASES = [
    ("global-9261", (1, 1, 24, 22, 70), (21, 21, 21), torch.float32, False, None),  # coarse field read from global memory
    ("global-9261-f64", (1, 1, 24, 22, 70), (21, 21, 21), torch.float64, False, None),
    ("global-9261-f16", (1, 1, 24, 22, 70), (21, 21, 21), torch.float16, False, None),
    ("global-9261-bf16", (1, 1, 24, 22, 70), (21, 21, 21), torch.bfloat16, False, None),
    ("global-9261-skip01", (2, 1, 24, 22, 70), (21, 21, 21), torch.float32, False, [0, 1]),
    ("lds-8192", (1, 1, 24, 22, 70), (16, 16, 32), torch.float32, False, None),  # the last size that is staged in LDS
    ("divide-1x3x2", (2, 1, 9, 5, 65), (1, 3, 2), torch.float32, True, None),  # a coarse axis of length 1
    ("copy-8x4x64", (1, 2, 8, 4, 64), (8, 4, 64), torch.float32, False, None),  # coarse extent == image extent on every axis
    ("coarse-larger", (1, 1, 7, 3, 63), (9, 5, 70), torch.float32, False, None),  # i0 advances by more than one per voxel
    ("one-voxel", (1, 1, 1, 1, 1), (2, 2, 2), torch.float32, False, None),
    ("j1-17x1x130", (1, 1, 17, 1, 130), (4, 4, 4), torch.float32, False, None),
    ("grid-z-65528", (8191, 1, 64, 1, 1), (2, 1, 1), torch.float32, False, None),  # the last batch one launch takes
]
BIAS_IDS = [case[0] for case in BIAS_CASES]
BIAS_TOO_LARGE = ((8192, 1, 64, 1, 1), (2, 1, 1))  # grid.z = 65536: refused


@functools.lru_cache(maxsize=None)
def bias_inputs(case_id: str):
    """``(data, coarse, skip)`` on the CPU (cached: do not modify)."""
    index = BIAS_IDS.index(case_id)
    _, shape, extents, dtype, _, skip = BIAS_CASES[index]
    data = _rand(shape, dtype, 100 + index)
    generator = torch.Generator().manual_seed(200 + index)
    coarse = 0.5 * torch.randn(*shape[:2], *extents, generator=generator)
    return data, coarse, None if skip is None else torch.tensor(skip, dtype=torch.uint8)


def bias_reference(data, coarse, divide) -> torch.Tensor:
    field = torch.exp(F.interpolate(coarse.double(), size=tuple(data.shape[2:]), mode="trilinear", align_corners=True))
    return data.double() / field if divide else data.double() * field


def bias_bar(coarse, dtype) -> float:
    """Relative to the reference (module docstring)."""
    c = coarse.double()
    steepest = sum((c.shape[axis] - 1) * float(c.diff(dim=axis).abs().max()) for axis in (2, 3, 4) if c.shape[axis] > 1)
    bar = EPS * (8 * float(c.abs().max()) + 4 * steepest) + 4 * EPS
    return bar + {torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}.get(dtype, 0.0)


def check_bias(engine, device, case_id) -> torch.Tensor:
    _, _, _, dtype, divide, _ = BIAS_CASES[BIAS_IDS.index(case_id)]
    data, coarse, skip = bias_inputs(case_id)
    out = engine.bias_field_apply(data.to(device), coarse.to(device), divide=divide, skip=None if skip is None else skip.to(device))
    _sync(device)
    out = out.cpu()
    assert out.dtype == dtype and out.shape == data.shape
    reference = bias_reference(data, coarse, divide)
    rows = torch.ones(data.shape[0], dtype=torch.bool) if skip is None else skip == 0
    assert same_bits(out[~rows], data[~rows])  # skipped rows: the input's bits
    bar = bias_bar(coarse, dtype)
    floor = 2.0**-25 if dtype == torch.float16 else 0.0  # half a float16 subnormal step
    error = (out[rows].double() - reference[rows]).abs()
    excess = (error - floor).clamp_min(0) / reference[rows].abs().clamp_min(1e-300)
    record(f"{device}: bias {case_id} max relative error", excess.max(), bar)
    assert bool((error <= bar * reference[rows].abs() + floor).all())
    return out


# -- Noise -------------------------------------------------------------------------------------------------------------------
NOISE_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
# (id, shape, mean, std, keep, seed): 3 x 5 x 29 = 435 = 4 * 108 + 3 elements per row, so rows 1 and 2 start inside a block
NOISE_SHAPES = [
    ("435-per-row", (3, 1, 3, 5, 29), [0.1, 0.0, -0.2], [0.25, 0.0, 0.5], [1, 0, 1], 0x9E3779B97F4A7C15),
    ("4096-per-row", (2, 1, 8, 8, 64), [0.05, -0.1], [0.3, 0.25], None, 99),
]
NOISE_CASES = [(name, rician, dtype) for name, *_ in NOISE_SHAPES for rician in (False, True) for dtype in NOISE_DTYPES]
NOISE_IDS = [f"{name}-{'rician' if rician else 'gaussian'}-{str(dtype).split('.')[-1]}" for name, rician, dtype in NOISE_CASES]


def _noise_setup(name, dtype):
    index = [entry[0] for entry in NOISE_SHAPES].index(name)
    _, shape, mean, std, keep, seed = NOISE_SHAPES[index]
    data = _rand(shape, dtype, 300 + index)
    keep = None if keep is None else torch.tensor(keep, dtype=torch.uint8)
    return data, torch.tensor(mean), torch.tensor(std), keep, seed


def check_noise_philox(engine, device, name, rician, dtype) -> torch.Tensor:
    data, mean, std, keep, seed = _noise_setup(name, dtype)
    out = engine.add_noise(data.to(device), mean, std, rician=rician, philox_seed=seed, keep=None if keep is None else keep.to(device))
    _sync(device)
    out = out.cpu()
    assert out.dtype == dtype and out.shape == data.shape
    shape = (-1, 1, 1, 1, 1)
    mu, sd = mean.double().reshape(shape), std.double().reshape(shape)  # (the float32 parameters, exactly)
    z1 = philox_normal_reference(seed, 0, data.numel())[0].view(data.shape)
    n1 = mu + sd * z1
    if rician:
        z2 = philox_normal_reference(seed, 1, data.numel())[0].view(data.shape)
        s, n2 = data.double() + n1, mu + sd * z2
        reference = torch.sqrt(s * s + n2 * n2)
        draws = sd * (s.abs() * philox_bar(z1) + n2.abs() * philox_bar(z2)) / reference.clamp_min(1e-300)
    else:
        reference = data.double() + n1
        draws = sd * philox_bar(z1)
    bar = draws + STORAGE_EPS[dtype] * reference.abs()
    rows = torch.ones(data.shape[0], dtype=torch.bool) if keep is None else keep != 0
    assert same_bits(out[~rows], data[~rows])  # gated rows: the input's bits
    error = (out[rows].double() - reference[rows]).abs()
    kind = "rician" if rician else "gaussian"
    record(f"{device}: noise {name} {kind} {dtype} max error / bar", (error / bar[rows]).max(), 1.0)
    assert bool((error <= bar[rows]).all())
    return out


def check_noise_explicit_16bit(engine, device, dtype) -> torch.Tensor:
    """Explicit draws in 16-bit storage: bit for bit ``(x.float() + (mean + std * base1)).to(dtype)``."""
    data, mean, std, keep, _ = _noise_setup("435-per-row", dtype)
    generator = torch.Generator().manual_seed(310)
    base1 = torch.randn(data.shape, generator=generator)
    out = engine.add_noise(data.to(device), mean, std, base1=base1.to(device), keep=keep.to(device))
    _sync(device)
    out = out.cpu()
    shape = (-1, 1, 1, 1, 1)
    expected = (data.float() + (mean.reshape(shape) + std.reshape(shape) * base1)).to(dtype)
    expected[keep == 0] = data[keep == 0]
    assert same_bits(out, expected)
    return out


# -- Gamma -------------------------------------------------------------------------------------------------------------------
GAMMA_TABLE = [0.0, -0.0, 1e-40, -1e-42, math.inf, -math.inf, math.nan, 1.0, -1.0, 3.4e38, -2.5, 1e-20]
GAMMA_SHAPE = (3, 2, 9, 11, 31)
GAMMA_EXPONENTS = [0.5, 1.0, 2.0, 0.0, (0.8, 1.0, 1 / 0.8)]
GAMMA_DTYPES = [torch.float32, torch.float64, torch.bfloat16]
GAMMA_RTOL = {torch.float32: 2e-6, torch.float64: 2e-6, torch.float16: 2e-3, torch.bfloat16: 2.0**-8}
# Below the normal range a relative bar means nothing: 2e-6 is 16 float32 ulps, and an ulp there is 2^-149 (1e-20 ** 2 lands
# there); bfloat16 adds half its smallest subnormal, the rounding of the store; no float64 result of these inputs is that small.
GAMMA_FLOOR = {torch.float32: 16 * 2.0**-149, torch.float64: 0.0, torch.bfloat16: 16 * 2.0**-149 + 2.0**-134}


@functools.lru_cache(maxsize=None)
def gamma_inputs(dtype) -> torch.Tensor:
    """Random values in [-1, 3) with the table at the start of EVERY batch element (so each per-element exponent meets it)."""
    data = _rand(GAMMA_SHAPE, torch.float32, 400)
    data[:, 0, 0, 0, : len(GAMMA_TABLE)] = torch.tensor(GAMMA_TABLE, dtype=torch.float64).to(torch.float32)
    return data.to(dtype)


def _gamma_expression(data, exponent):
    return data.sign() * data.abs().pow(exponent)  # gamma.py:90


def check_gamma(engine, device, dtype, exponent) -> torch.Tensor:
    data = gamma_inputs(dtype)
    per_element = isinstance(exponent, tuple)
    gamma = torch.tensor(exponent, dtype=torch.float32) if per_element else float(exponent)
    out = engine.gamma_pow(data.to(device), gamma)
    _sync(device)
    out = out.cpu()
    assert out.dtype == dtype and out.shape == data.shape
    carried = torch.tensor(exponent, dtype=torch.float32).reshape(-1, 1, 1, 1, 1) if per_element else torch.tensor(float(exponent), dtype=torch.float32)
    compute = torch.float64 if dtype == torch.float64 else torch.float32
    classes = _gamma_expression(data.to(compute), carried.to(compute)).to(dtype)  # what torch makes of it in the engine's precision
    reference = _gamma_expression(data.double(), carried.double())
    special = classes.isnan() | classes.isinf() | (classes == 0)
    assert torch.equal(out.isnan(), classes.isnan())
    assert torch.equal(out.isinf(), classes.isinf()) and torch.equal(out == 0, classes == 0)
    signed = ~classes.isnan()
    assert torch.equal(torch.signbit(out)[signed], torch.signbit(classes)[signed])  # of zeros and infinities too
    assert int(special[:, 0, 0, 0, : len(GAMMA_TABLE)].sum()) >= 3 * 2  # the table is in there (its zeros stay zeros under every exponent)
    finite = ~special
    error = (out.double()[finite] - reference[finite]).abs()
    bar = GAMMA_RTOL[dtype] * reference[finite].abs() + GAMMA_FLOOR[dtype]
    record(f"{device}: gamma {dtype} exponent {exponent} max error / bar", (error / bar).max(), 1.0)
    assert bool((error <= bar).all())
    return out


# -- channel_min -------------------------------------------------------------------------------------------------------------
MIN_GRID = 512 * 256  # threads of the capped grid = float4 (or elements, in the scalar loop) per grid stride
MIN_LARGE = (1, 2, 116, 128, 512)  # n / 4 = 1 900 544 = 14.5 grid strides: one 8-deep pass, one 4-deep pass, 2.5 single ones
MIN_SCALAR = (1, 1, 1, 3, 87383)  # n = 262 149 = 2 grid strides + 5, n % 4 == 1: the scalar loop, three passes for 5 threads


def expect_same_minimum(out: torch.Tensor, data: torch.Tensor) -> None:
    expected = data[0].float().amin(dim=(1, 2, 3))
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == expected.shape
    assert torch.equal(out.isnan(), expected.isnan()) and bool((out == expected)[~expected.isnan()].all()), (out, expected)


@functools.lru_cache(maxsize=None)
def _min_base(shape, dtype) -> torch.Tensor:
    """Values in [1, 2) (integers: 1 .. 99), nothing below 1 (cached: do not modify)."""
    generator = torch.Generator().manual_seed(500)
    if dtype.is_floating_point:
        return (torch.rand(*shape, generator=generator) + 1).to(dtype)
    return torch.randint(1, 100, shape, generator=generator).to(dtype)


def min_large_plants():
    """Float4 slots ``(stride, lane, component)`` of the large case -> flat element index in a channel.  The 8-deep pass
    reads the strides 0 .. 7, the 4-deep pass 8 .. 11, the single loop 12, 13 and the half stride 14."""
    n4 = math.prod(MIN_LARGE[2:]) // 4
    element = lambda stride, lane, component: 4 * (stride * MIN_GRID + lane) + component  # noqa: E731
    deep8 = [element(u, 1000 * u + 7, u % 4) for u in range(8)]
    deep4 = [element(8 + u, 70000 + u, (u + 1) % 4) for u in range(4)]
    tail = [element(12, 5, 2), element(13, MIN_GRID - 1, 0), element(14, 0, 1), 4 * n4 - 1]  # (the last: the very last element)
    assert tail[2] < 4 * n4 and 14 * MIN_GRID < n4 < 15 * MIN_GRID
    return deep8, deep4, tail


def check_channel_min_large(engine, device) -> None:
    """One run per unrolled load of each loop: channel 0 walks the 16 slots, channel 1 walks them five slots ahead, so the
    two channels' minima always sit in different places (and, in the runs the comments mark, in different loops)."""
    base = _min_base(MIN_LARGE, torch.float32)
    deep8, deep4, tail = min_large_plants()
    slots = deep8 + deep4 + tail
    on_device = base.to(device).clone()
    host = base.clone()
    for run, slot in enumerate(slots):
        other = slots[(run + 5) % len(slots)]  # run 0: 8-deep / 8-deep ... run 3: 8-deep / 4-deep, run 8: 4-deep / tail, run 12: tail / 8-deep
        for tensor in (on_device, host):
            tensor[0, 0].view(-1)[slot] = 0.25 - 0.001 * run
            tensor[0, 1].view(-1)[other] = -3.0 - run
        expect_same_minimum(engine.channel_min(on_device), host)
        for tensor in (on_device, host):
            tensor[0, 0].view(-1)[slot] = base[0, 0].view(-1)[slot]
            tensor[0, 1].view(-1)[other] = base[0, 1].view(-1)[other]
    expect_same_minimum(engine.channel_min(on_device), host)  # nothing planted: the field's own minimum, >= 1


def check_channel_min_scalar_loop(engine, device, dtype) -> None:
    base = _min_base(MIN_SCALAR, dtype)
    n = base[0, 0].numel()
    assert n % 4 != 0 and n > 2 * MIN_GRID
    for position in (n - 1, 2 * MIN_GRID, MIN_GRID + 17, 3):  # the last stride (its last and first element), the second, the first
        data = base.clone()
        data.view(-1)[position] = 0
        expect_same_minimum(engine.channel_min(data.to(device)), data)
    expect_same_minimum(engine.channel_min(base.to(device)), base)


def check_channel_min_values(engine, device) -> None:
    """NaN wins, -inf wins over everything else, and a channel of zeros of both signs gives a zero."""
    data = _rand((2, 4, 3, 5, 67), torch.float32, 501)
    data[0, 0, 1, 2, 30] = math.nan
    data[0, 0, 2, 4, 66] = -math.inf  # NaN still wins
    data[0, 1, 0, 0, 0] = -math.inf
    data[0, 2] = 0.0
    data[0, 2, :, ::2] = -0.0
    data[0, 3, 2, 4, 66] = math.inf  # +inf never is the minimum of a channel with finite values
    data[1] = -100.0  # only element 0 counts
    expect_same_minimum(engine.channel_min(data.to(device)), data)
    zeros = torch.zeros(1, 2, 1, 1, 2)
    zeros[0, 0, 0, 0, 0] = -0.0  # [-0, 0] and [0, 0]
    expect_same_minimum(engine.channel_min(zeros.to(device)), zeros)
    everything = torch.full((1, 1, 2, 3, 5), math.inf)
    expect_same_minimum(engine.channel_min(everything.to(device)), everything)


def check_channel_min_workspace_growth(engine, device) -> None:
    """3 channels, then 1100 (beyond the 1024 the workspace starts with), then 3 again, 1100 again: the grown workspace
    must come up clean and be left clean."""
    small = _rand((1, 3, 4, 5, 6), torch.float32, 502)
    wide = _rand((1, 1100, 1, 1, 5), torch.float32, 503)
    for data in (small, wide, small, wide, small - 7.0):
        expect_same_minimum(engine.channel_min(data.to(device)), data)
