"""Test-only reference, bounds and cases for the parameter gradients of the intensity ops (``tio_bias_field_grad``,
``tio_gamma_grad``, ``tio_noise_grad``, ``tio_separable_conv3d_taps_grad``): tests/test_param_grad_host.py,
tests/test_gpu_param_grad.py, tests/test_gpu_param_grad_guarded.py.  Nothing here is imported by the product.

The reference restates the reference implementation's four compositions of torch operations in float64 on the CPU and lets
autograd differentiate them:

* bias:   ``x * exp(F.interpolate(coarse, mode="trilinear", align_corners=True))`` (or ``/``)      bias_field.py:237-244
* blur:   ``F.pad(mode="replicate")`` + a correlation per axis, order I, J, K                         blur.py:157-252
* noise:  ``x + (mean + std * z)``; Rician ``sqrt((x + n1)^2 + n2^2)``
* gamma:  ``sign(x) * |x| ** gamma``

For every output component ``p`` it also returns ``A_p``: the same sum with every factor replaced by its absolute value (for the
Rician numerators and the stencil chain the absolute values are taken at the leaves: ``|x| + |mean| + |std z|`` for ``x + n1``).

The bound per component is the one the issue states::

    |got - ref| <= (tau + c * 2^-24) * A_p + 2^-24 * |ref|

``tau = 1e-6`` where a term contains the forward's ``expf`` / ``powf`` / ``logf`` (bias, gamma), 0 elsewhere.  ``c`` counts the float32
roundings along one term's chain in intensity_param_grad.hip (everything above a term is float64 and rounds once, which
``2^-24 |ref|`` covers):

* gamma, ``C_GAMMA = 4``: ``powf`` (1), ``logf`` (1), ``gy * y`` (1), ``* log|x|`` (1).  (float64 data takes float64 expressions.)
* noise, additive: ``d_mean`` sums ``gy`` itself, ``c = 0``; ``d_std`` sums ``fl(gy * z)``, ``c = 1``.
* noise, Rician, ``C_RICIAN = 18``: with ``S`` the leaf sum of a numerator, ``n_i`` carries 2 roundings, ``a = x + n1`` 1, the two
  numerator operations 2: 5, relative to ``S``.  ``y`` carries the 3 of ``a`` and ``n2``, two squares, a sum and a root: 7 roundings
  that move ``y`` by ``7 u S (|a| + |n2|) / y^2 <= 7 sqrt(2) u S / y`` relative - 10.  The division and the product: 2.  17, and 1 for
  the data narrowed where it is float64 elsewhere in the family.
* bias, ``C_BIAS = 12 + 6 * sum_a (n_a - 1)`` over the axes that interpolate (``n_a`` coarse nodes, extent != ``n_a``): the chain has
  the three lerps of the exponent (6, each absolute in a coarse value of modest size: they move ``y`` relatively), the product
  with ``x`` (1; 2 with float64 data narrowed), ``gy * y`` (1), ``w_k * term`` (1), ``w_i * w_j`` (1): 11 at most.  The lerp weights
  themselves are float32: ``real = scale * o`` carries the roundings of ``scale`` and of the product, an ABSOLUTE error of up to
  ``1.5 u (n_a - 1)`` in ``l1`` and ``l0``.  Summed over the ``m`` voxels of a cell that is ``3 u (n_a - 1) m`` against a weight sum of
  ``m`` (an inner node; ``m / 2`` and half the error at an edge node): ``3 u (n_a - 1)`` relative to ``A_p`` for evenly spread
  ``|gy y|``, doubled here for data that is not.
* taps, ``C_TAPS = 1 + sum_a (3 r_a + 2)``: the product ``g * a`` (1); a forward pass along an axis of radius ``r`` accumulates
  ``2 r + 1`` products one after the other (``2 r + 2`` roundings, relative to the absolute-value pass that ``A_p`` contains), a
  transposed pass ``2 r + 1`` fused steps plus up to ``r`` additions of the clamped border sums.  Each of the three gradients
  passes through two of the three axes; the bound takes all three.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
TAU = 1e-6
C_GAMMA = 4
C_RICIAN = 18
DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def c_bias(shape, coarse_shape) -> int:
    return 12 + 6 * sum(n - 1 for extent, n in zip(shape, coarse_shape, strict=True) if extent != n)


def c_taps(radius) -> int:
    return 1 + sum(3 * int(r) + 2 for r in radius)


def _narrowed(x: torch.Tensor) -> torch.Tensor:
    """The values a kernel that loads through float32 computes with (bias, taps): exact for the three narrower dtypes."""
    return x.detach().cpu().to(torch.float32).double()


def _rows(flags, batch: int, ndim: int) -> torch.Tensor:
    """(B, 1, ...) bool: the elements that take part (``flags`` marks the ones that do NOT when it is a skip list)."""
    if flags is None:
        return torch.ones((batch,) + (1,) * (ndim - 1), dtype=torch.bool)
    return (flags.detach().cpu().to(torch.uint8) == 0).reshape((batch,) + (1,) * (ndim - 1))


# ---------------------------------------------------------------------------------------------------------------------
# bias
# ---------------------------------------------------------------------------------------------------------------------
def bias_loss(x64: torch.Tensor, gy64: torch.Tensor, coarse: torch.Tensor, divide: bool, skip=None) -> torch.Tensor:
    field = torch.exp(F.interpolate(coarse, size=x64.shape[2:], mode="trilinear", align_corners=True))
    y = x64 / field if divide else x64 * field
    y = torch.where(_rows(skip, x64.shape[0], 5), y, x64)
    return (gy64 * y).sum()


def bias(x, gy, coarse, divide=False, skip=None):
    """(reference, A) in the shape of ``coarse``."""
    x64, gy64 = _narrowed(x), gy.detach().cpu().double()
    leaf = coarse.detach().cpu().double().requires_grad_(True)
    with torch.enable_grad():
        (ref,) = torch.autograd.grad(bias_loss(x64, gy64, leaf, divide, skip), leaf)
        field = torch.exp(F.interpolate(leaf.detach(), size=x64.shape[2:], mode="trilinear", align_corners=True))
        magnitude = (gy64 * (x64 / field if divide else x64 * field)).abs() * _rows(skip, x64.shape[0], 5)
        weights = F.interpolate(leaf, size=x64.shape[2:], mode="trilinear", align_corners=True)  # linear in the leaf: its gradient is the weights
        (a,) = torch.autograd.grad((magnitude * weights).sum(), leaf)
    return ref, a


# ---------------------------------------------------------------------------------------------------------------------
# gamma
# ---------------------------------------------------------------------------------------------------------------------
def _per_element(value: torch.Tensor, batch: int, ndim: int) -> torch.Tensor:
    return value.reshape((-1,) + (1,) * (ndim - 1)) if value.numel() == batch and batch > 1 else value.reshape(())


def gamma_loss(x64, gy64, gamma):
    return (gy64 * torch.sign(x64) * x64.abs() ** _per_element(gamma, x64.shape[0], x64.ndim)).sum()


def gamma(x, gy, gamma_values):
    """(reference, A), one value per exponent."""
    x64, gy64 = x.detach().cpu().double(), gy.detach().cpu().double()
    leaf = gamma_values.detach().cpu().double().reshape(-1).requires_grad_(True)
    with torch.enable_grad():
        (ref,) = torch.autograd.grad(gamma_loss(x64, gy64, leaf), leaf)
    exponent = _per_element(leaf.detach(), x64.shape[0], x64.ndim)
    logs = torch.where(x64 != 0, x64.abs().clamp_min(1e-300).log().abs(), torch.zeros_like(x64))
    terms = gy64.abs() * x64.abs() ** exponent * logs
    a = terms.reshape(x64.shape[0], -1).sum(dim=1) if leaf.numel() > 1 else terms.sum().reshape(1)
    return ref, a


# ---------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------
def noise_loss(x64, gy64, mean, std, z1, z2, rician: bool, keep=None):
    batch = gy64.shape[0]
    mu, sd = _per_element(mean, batch, gy64.ndim), _per_element(std, batch, gy64.ndim)
    n1 = mu + sd * z1
    if rician:
        n2 = mu + sd * z2
        squared = (x64 + n1) ** 2 + n2 ** 2
        y = torch.where(squared > 0, torch.where(squared > 0, squared, torch.ones_like(squared)).sqrt(), torch.zeros_like(squared))  # y == 0 adds nothing
    else:
        y = x64 + n1
    kept = torch.ones_like(gy64, dtype=torch.bool) if keep is None else (keep.detach().cpu().to(torch.uint8) != 0).reshape((batch,) + (1,) * (gy64.ndim - 1))
    return (gy64 * torch.where(kept, y, torch.zeros_like(y))).sum()


def noise(x, gy, mean, std, z1, z2=None, rician=False, keep=None):
    """((reference, A) of d_mean, (reference, A) of d_std), each with as many values as its parameter."""
    gy64 = gy.detach().cpu().double()
    x64 = torch.zeros_like(gy64) if x is None else x.detach().cpu().double()
    z1 = z1.detach().cpu().double()
    z2 = None if z2 is None else z2.detach().cpu().double()
    batch = gy64.shape[0]
    leaves = [p.detach().cpu().double().reshape(-1).requires_grad_(True) for p in (mean, std)]
    with torch.enable_grad():
        refs = torch.autograd.grad(noise_loss(x64, gy64, leaves[0], leaves[1], z1, z2, rician, keep), leaves)
    mu, sd = (_per_element(p.detach(), batch, gy64.ndim) for p in leaves)
    kept = 1.0 if keep is None else (keep.detach().cpu().to(torch.uint8) != 0).double().reshape((batch,) + (1,) * (gy64.ndim - 1))
    if rician:
        n1, n2 = mu + sd * z1, mu + sd * z2
        y = ((x64 + n1) ** 2 + n2 ** 2).sqrt()
        inverse = torch.where(y > 0, 1.0 / y.clamp_min(1e-300), torch.zeros_like(y)) * gy64.abs() * kept
        leaf_a, leaf_n2 = x64.abs() + mu.abs() + (sd * z1).abs(), mu.abs() + (sd * z2).abs()
        terms = [inverse * (leaf_a + leaf_n2), inverse * (leaf_a * z1.abs() + leaf_n2 * z2.abs())]
    else:
        terms = [gy64.abs() * kept * torch.ones_like(z1), gy64.abs() * kept * z1.abs()]
    out = []
    for ref, leaf, term in zip(refs, leaves, terms, strict=True):
        a = term.reshape(batch, -1).sum(dim=1) if leaf.numel() > 1 else term.sum().reshape(1)
        out.append((ref, a))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------------------------------------------------
def _correlate_axis(x, weights, radius: int, axis: int):
    """``sum_t w[b, t] * x[clamp(v + (t - r) e_axis)]`` on (B, C, I, J, K); weights (1|B, 2 r + 1)."""
    extent = x.shape[2 + axis]
    positions = torch.arange(extent)
    out = torch.zeros_like(x)
    for t in range(2 * radius + 1):
        index = (positions + t - radius).clamp(0, extent - 1)
        out = out + weights[:, t].reshape(-1, 1, 1, 1, 1) * x.index_select(2 + axis, index)
    return out


def taps_loss(x64, gy64, taps, radius, skip=None):
    y = x64
    for axis in range(3):
        if radius[axis] > 0:
            y = _correlate_axis(y, taps[:, axis, : 2 * radius[axis] + 1], radius[axis], axis)
    y = torch.where(_rows(skip, x64.shape[0], 5), y, x64)
    return (gy64 * y).sum()


def taps(x, gy, tap_values, radius, skip=None):
    """(reference, A) in the shape of the taps."""
    x64, gy64 = _narrowed(x), gy.detach().cpu().double()
    leaf = tap_values.detach().cpu().double().requires_grad_(True)
    magnitude = tap_values.detach().cpu().double().abs().requires_grad_(True)
    with torch.enable_grad():
        (ref,) = torch.autograd.grad(taps_loss(x64, gy64, leaf, radius, skip), leaf)
        (a,) = torch.autograd.grad(taps_loss(x64.abs(), gy64.abs(), magnitude, radius, skip), magnitude)
    return ref, a


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def ratio(got: torch.Tensor, ref: torch.Tensor, a: torch.Tensor, c: float, tau: float) -> float:
    """Largest ``error / bound`` over the components (0 where both are 0)."""
    got, ref, a = got.detach().cpu().double().reshape(-1), ref.reshape(-1), a.reshape(-1)
    assert got.shape == ref.shape == a.shape, (got.shape, ref.shape, a.shape)
    assert bool(torch.isfinite(got).all()), "non-finite gradient"
    error, bound = (got - ref).abs(), (tau + c * U) * a + U * ref.abs()
    quotient = torch.where(error == 0, torch.zeros_like(error), error / bound.clamp_min(1e-300))
    return float(quotient.max()) if quotient.numel() else 0.0


def check(label: str, got, ref, a, c: float, tau: float) -> float:
    value = ratio(got, ref, a, c, tau)
    print(f"param-grad {label}: error/bound = {value:.3g}  (c = {c}, tau = {tau:g})")
    assert value <= 1.0, f"{label}: error / bound = {value}"
    return value


# ---------------------------------------------------------------------------------------------------------------------
# cases (built once, shared by the tests, never modified)
# ---------------------------------------------------------------------------------------------------------------------
def _uniform(generator, shape, low=-1.0, high=1.0):
    return torch.rand(shape, generator=generator) * (high - low) + low


BIAS_CASES = {
    # name: (shape (B, C, I, J, K), coarse (si, sj, sk), divide, skip, dtype)
    "ragged-k70": ((2, 2, 9, 6, 70), (4, 4, 4), False, None, torch.float32),          # K crosses a 64-lane tile raggedly; J, I no multiples of the 4 x 8 tile
    "tiny": ((1, 1, 5, 5, 3), (2, 2, 2), False, None, torch.float32),
    "degenerate-k": ((1, 1, 33, 17, 1), (3, 3, 1), False, None, torch.float32),
    "box-limit-inside": ((2, 2, 9, 6, 70), (3, 3, 8), False, None, torch.float32),    # 8 k nodes under the first K tile: the LDS box
    "box-limit-beyond": ((2, 2, 9, 6, 70), (3, 3, 9), False, None, torch.float32),    # 9: that tile adds to the workspace directly, the second K tile keeps its box
    "full-resolution": ((1, 2, 9, 6, 70), (9, 6, 70), False, None, torch.float32),    # every voxel its own node: no box anywhere
    "many-blocks": ((2, 1, 40, 40, 130), (3, 4, 5), False, None, torch.float32),
    "divide": ((2, 2, 9, 6, 70), (4, 4, 4), True, None, torch.float32),
    "skip": ((3, 1, 9, 6, 70), (4, 4, 4), False, (0, 1, 0), torch.float32),
    "float64": ((2, 1, 9, 6, 70), (4, 4, 4), False, None, torch.float64),
    "float16": ((2, 1, 9, 6, 70), (4, 4, 4), True, None, torch.float16),
    "bfloat16": ((2, 1, 9, 6, 70), (4, 4, 4), False, None, torch.bfloat16),
}


@functools.lru_cache(maxsize=None)
def bias_case(name: str) -> dict:
    shape, coarse_shape, divide, skip, dtype = BIAS_CASES[name]
    g = torch.Generator().manual_seed(100 + sorted(BIAS_CASES).index(name))
    x = (_uniform(g, shape, 0.2, 1.5) * torch.where(torch.rand(shape, generator=g) < 0.3, -1.0, 1.0)).to(dtype)
    gy = _uniform(g, shape)
    coarse = _uniform(g, (*shape[:2], *coarse_shape), -0.5, 0.5)
    flags = None if skip is None else torch.tensor(skip, dtype=torch.uint8)
    ref, a = bias(x, gy, coarse, divide, flags)
    return dict(x=x, gy=gy, coarse=coarse, divide=divide, skip=flags, ref=ref, a=a, c=c_bias(shape[2:], coarse_shape))


GAMMA_CASES = {
    # name: (B, n_per_element as a (C, I, J, K) shape, batched, dtype)
    "scalar-7": (2, (1, 1, 1, 7), False, torch.float32),
    "batched-64": (3, (1, 1, 8, 8), True, torch.float32),
    "batched-4099": (2, (1, 1, 1, 4099), True, torch.float32),
    "scalar-4099": (2, (1, 1, 1, 4099), False, torch.float32),
    "float64": (2, (1, 1, 1, 4099), True, torch.float64),
    "float16": (2, (1, 1, 8, 8), True, torch.float16),
    "bfloat16": (2, (1, 1, 8, 8), False, torch.bfloat16),
}


@functools.lru_cache(maxsize=None)
def gamma_case(name: str) -> dict:
    batch, element, batched, dtype = GAMMA_CASES[name]
    g = torch.Generator().manual_seed(200 + sorted(GAMMA_CASES).index(name))
    shape = (batch, *element)
    x = _uniform(g, shape, -2.0, 2.0)
    x[torch.rand(shape, generator=g) < 0.15] = 0.0  # exact zeros: they add nothing
    x = x.to(dtype)
    gy = _uniform(g, shape)
    exponent = _uniform(g, (batch,), 0.6, 1.7) if batched else _uniform(g, (1,), 0.6, 1.7)
    ref, a = gamma(x, gy, exponent)
    assert bool((x == 0).any()) and bool((x < 0).any())
    return dict(x=x, gy=gy, gamma=exponent, ref=ref, a=a)


NOISE_CASES = {
    # name: (B, element shape, batched, rician, keep, dtype)
    "additive-scalar": (2, (1, 3, 5, 7), False, False, None, torch.float32),       # n_per_element = 105, % 4 != 0
    "additive-batched": (3, (2, 4, 4, 8), True, False, None, torch.float32),
    "additive-keep": (3, (1, 3, 5, 7), True, False, (1, 0, 1), torch.float32),
    "rician-scalar": (2, (1, 3, 5, 7), False, True, None, torch.float32),
    "rician-batched-zeros": (2, (1, 4, 4, 8), True, True, None, torch.float32),    # element 0 holds voxels with y == 0
    "rician-keep": (3, (1, 3, 5, 7), True, True, (0, 1, 1), torch.float32),
    "rician-float64": (2, (1, 3, 5, 7), True, True, None, torch.float64),
    "rician-float16": (2, (1, 4, 4, 8), False, True, None, torch.float16),
    "additive-bfloat16": (2, (1, 4, 4, 8), True, False, None, torch.bfloat16),
}


@functools.lru_cache(maxsize=None)
def noise_inputs(name: str) -> dict:
    """The inputs of a noise case without draws and reference (the Philox tests bring the kernel's own draws)."""
    batch, element, batched, rician, keep, dtype = NOISE_CASES[name]
    g = torch.Generator().manual_seed(300 + sorted(NOISE_CASES).index(name))
    shape = (batch, *element)
    x = _uniform(g, shape, -1.0, 2.0).to(dtype)
    gy = _uniform(g, shape)
    mean = _uniform(g, (batch,), -0.3, 0.3) if batched else _uniform(g, (1,), -0.3, 0.3)
    std = torch.tensor([0.75, 1.25, 0.5][:batch]) if batched else torch.tensor([0.75])  # dyadic: std * z is exact for the planted draws below
    flags = None if keep is None else torch.tensor(keep, dtype=torch.uint8)
    return dict(x=x, gy=gy, mean=mean, std=std, rician=rician, keep=flags, shape=shape, generator_state=g.get_state())


@functools.lru_cache(maxsize=None)
def noise_case(name: str) -> dict:
    """A noise case with explicit draws and its reference."""
    case = dict(noise_inputs(name))
    g = torch.Generator()
    g.set_state(case["generator_state"])
    z1, z2 = torch.randn(case["shape"], generator=g), torch.randn(case["shape"], generator=g)
    if name == "rician-batched-zeros":  # y == 0 exactly, in float32 and in float64: mean 0, z2 = 0, x = -(std * z1) with a dyadic product
        case["mean"] = case["mean"].clone()
        case["mean"][0] = 0.0
        x = case["x"].clone()
        for site in ((0, 0, 0, 0, 0), (0, 0, 1, 2, 3), (0, 0, 3, 3, 7)):
            z1[site], z2[site] = 2.0, 0.0
            x[site] = -float(case["std"][0]) * 2.0
        case["x"] = x
    case["z1"], case["z2"] = z1, (z2 if case["rician"] else None)
    case["mean_ref"], case["std_ref"] = noise(case["x"], case["gy"], case["mean"], case["std"], z1, case["z2"], case["rician"], case["keep"])
    return case


def noise_c(case: dict) -> tuple[int, int]:
    return (C_RICIAN, C_RICIAN) if case["rician"] else (0, 1)


TAPS_CASES = {
    # name: (shape, radius, batched, skip, tap_stride, dtype)
    "r123-shared": ((2, 2, 5, 6, 9), (1, 2, 3), False, None, 7, torch.float32),
    "r123-batched": ((2, 1, 5, 6, 9), (1, 2, 3), True, None, 7, torch.float32),
    "r040-short-axis": ((2, 1, 4, 3, 5), (0, 4, 0), True, None, 9, torch.float32),         # J = 3 under radius 4: clamping folds several taps
    "r16-1-8": ((1, 2, 3, 4, 70), (16, 1, 8), False, None, 33, torch.float32),             # I = 3 under radius 16
    "skip-wide-stride": ((3, 1, 5, 6, 9), (1, 2, 3), True, (0, 1, 0), 12, torch.float32),  # tap_stride beyond the widest axis' 7
    "k-only": ((2, 1, 3, 4, 70), (0, 0, 5), False, None, 11, torch.float32),
    "float64": ((2, 1, 5, 6, 9), (1, 2, 3), True, None, 7, torch.float64),
    "float16": ((2, 1, 5, 6, 9), (1, 0, 3), False, None, 7, torch.float16),
    "bfloat16": ((2, 1, 5, 6, 9), (0, 2, 3), True, None, 7, torch.bfloat16),
}


@functools.lru_cache(maxsize=None)
def taps_case(name: str) -> dict:
    shape, radius, batched, skip, stride, dtype = TAPS_CASES[name]
    g = torch.Generator().manual_seed(400 + sorted(TAPS_CASES).index(name))
    x = _uniform(g, shape, -1.0, 2.0).to(dtype)
    gy = _uniform(g, shape)
    weights = torch.zeros(shape[0] if batched else 1, 3, stride)
    for axis, r in enumerate(radius):
        if r > 0:
            values = _uniform(g, (weights.shape[0], 2 * r + 1), -0.2, 1.0)
            weights[:, axis, : 2 * r + 1] = values / values.sum(dim=1, keepdim=True).abs().clamp_min(0.5)
    flags = None if skip is None else torch.tensor(skip, dtype=torch.uint8)
    ref, a = taps(x, gy, weights, radius, flags)
    return dict(x=x, gy=gy, taps=weights, radius=list(radius), skip=flags, ref=ref, a=a, c=c_taps(radius))
