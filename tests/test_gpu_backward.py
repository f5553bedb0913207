"""The closed-form backward passes of torchio_amd/ops.py — bias field, gamma, noise (Gaussian, Rician with explicit and
with in-kernel Philox draws), flip, constant pad — per voxel against float64 autograd through the plain torch formula written
HERE, and the stencil adjoint at the radii 9 - 16 that the forward's fused path takes along I and J.

Shapes: ``B = 3, C = 2``, ragged extents.  ``E = 2^-23`` below is one float32 ulp relative (two unit roundoffs); every
tolerance is per voxel and one of

* a count of float32 roundings of the formula, stated beside the case (exact permutations and identities: equality);
* for ``exp`` / ``pow``, whose error no count gives: the deviation of the CPU engine (the oracle kernel, resp. the same tensor
  algebra on host tensors) from the same float64 reference, measured in the test as the largest relative deviation over the
  voxels; the HIP engine may be twice as far at any voxel.  The CPU engine itself is held to a generous a-priori bound, so
  that the yardstick cannot drift.

CPU-engine deviations measured (largest relative, in units of E; the tests print them with ``-s``): bias field multiply 1.12,
divide 1.08; gamma with a scalar exponent 1.37, per element 1.38 — the same on the development host and on an MI355X host.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import test_stencil_adjoint as stencil

E = 2.0 ** -23
SHAPE = (3, 2, 13, 11, 17)


def _inputs(seed, signed=False):
    g = torch.Generator().manual_seed(seed)
    data = torch.rand(SHAPE, generator=g) + 0.2
    if signed:
        data = data * (torch.randint(0, 2, SHAPE, generator=g) * 2 - 1)
    return data, torch.randn(SHAPE, generator=g), g


def _engine_backward(engine, device, op, data, grad):
    """(forward result, dL/d(data)) of ``op(engine, leaf)`` with the incoming gradient *grad*, on the host."""
    leaf = data.to(device).requires_grad_(True)
    out = op(engine, leaf, device)
    assert out.requires_grad and out.dtype == data.dtype
    (result,) = torch.autograd.grad(out, leaf, grad.to(device))
    assert result.dtype == data.dtype and result.shape == data.shape
    return out.detach().cpu(), result.cpu()


def _float64_backward(formula, data, grad):
    leaf = data.double().requires_grad_(True)
    with torch.enable_grad():
        out = formula(leaf)
    (result,) = torch.autograd.grad(out, leaf, grad.double())
    return out.detach(), result


def _assert_per_voxel(actual, reference, tolerance, what):
    error = (actual.double() - reference).abs()
    bad = error > tolerance
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} voxels beyond their tolerance, worst error / tolerance {float((error / tolerance.clamp_min(1e-300)).max()):.3g}"


def _relative_deviation(actual, reference):
    live = reference != 0
    return float(((actual.double() - reference).abs()[live] / reference.abs()[live]).max())


def _check_against_the_cpu_engine(engine, device, oracle, op, formula, data, grad, a_priori, what, exact_rows=None):
    """The `exp` / `pow` rule of the module docstring.  *a_priori*: the per-voxel relative bound the CPU engine is held to.
    *exact_rows*: batch elements whose gradient must be the incoming gradient bit for bit (skipped rows)."""
    _, reference = _float64_backward(formula, data, grad)
    _, theirs = _engine_backward(oracle, "cpu", op, data, grad)
    _assert_per_voxel(theirs, reference, a_priori * reference.abs(), f"{what} (cpu engine, a priori)")
    own = _relative_deviation(theirs, reference)
    print(f"\n{what}: the cpu engine deviates {own / E:.2f} E from float64 autograd")
    assert own > 0
    _, ours = _engine_backward(engine, device, op, data, grad)
    _assert_per_voxel(ours, reference, 2 * own * reference.abs(), what)
    if exact_rows is not None:
        assert torch.equal(ours[exact_rows], grad[exact_rows])


# -- bias field ---------------------------------------------------------------------------------------------------------
def _bias_field(engine, device, oracle, divide):
    data, grad, g = _inputs(5)
    coarse = 0.4 * torch.randn(3, 2, 4, 3, 5, generator=g)
    skip = torch.tensor([0, 1, 0], dtype=torch.uint8)

    def op(e, leaf, dev):
        return e.bias_field_apply(leaf, coarse.to(dev), divide=divide, skip=skip.to(dev))

    def formula(leaf):
        field = torch.exp(F.interpolate(coarse.double(), size=SHAPE[2:], mode="trilinear", align_corners=True))
        return torch.where(skip.bool().view(-1, 1, 1, 1, 1), leaf, leaf / field if divide else leaf * field)

    # a priori, relative: the exponent is three levels of two-point blends (two products and a sum each, of weights that carry
    # three roundings themselves): |d| <= 18 u max|coarse|, which exp turns into a relative error; exp itself within an ulp
    # (2 u), the multiply or divide u: (9 max|coarse| + 1.5) E, taken as (9 max|coarse| + 2) E
    a_priori = (9 * float(coarse.abs().max()) + 2) * E
    _check_against_the_cpu_engine(engine, device, oracle, op, formula, data, grad, a_priori, f"bias field divide={divide}", exact_rows=skip.bool())


# -- gamma ----------------------------------------------------------------------------------------------------------------
def _gamma(engine, device, oracle, per_element):
    data, grad, _ = _inputs(6, signed=True)
    assert bool((data < 0).any()) and bool((data > 0).any())
    gamma = torch.tensor([0.7, 1.0, 1.9]) if per_element else 1.35

    def op(e, leaf, dev):
        return e.gamma_pow(leaf, gamma)

    def formula(leaf):
        exponent = gamma.double().view(-1, 1, 1, 1, 1) if per_element else float(torch.tensor(gamma, dtype=torch.float32))
        return torch.sign(leaf) * leaf.abs() ** exponent

    # a priori, relative: g |x|^(g - 1) grad — the exponent g - 1 rounds once (u |(g - 1) ln|x|| on the power), pow within two
    # ulp (4 u), two products (2 u): (|(g - 1) ln|x|| / 2 + 3) E with |g - 1| <= 1 and |ln|x|| <= ln 5 on [0.2, 1.2]: 4 E
    _check_against_the_cpu_engine(engine, device, oracle, op, formula, data, grad, 4 * E, f"gamma per_element={per_element}")


# -- noise ----------------------------------------------------------------------------------------------------------------
def _gaussian_noise(engine, device):
    """Additive: the gradient is the incoming gradient, bit for bit (gated-out rows are copies: the same)."""
    data, grad, g = _inputs(7)
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8)
    std = torch.tensor([0.2, 0.3, 0.1])
    for draws in (torch.randn(SHAPE, generator=g), None):
        def op(e, leaf, dev, draws=draws):
            return e.add_noise(leaf, 0.1, std, base1=None if draws is None else draws.to(dev), philox_seed=77, keep=keep.to(dev))

        out, result = _engine_backward(engine, device, op, data, grad)
        assert torch.equal(result, grad)
        assert torch.equal(out[1], data[1]) and not torch.equal(out[0], data[0])


def _rician_reference(data, grad, mean, std, z1, z2, keep):
    """float64 autograd through ``sqrt((x + n1)^2 + n2^2)``, ``n = mean + std z`` (the float32 parameters and draws as they
    are), and the per-voxel rounding allowances of the float32 forward and backward.

    With ``a = x + n1``, ``b = n2``, ``y = sqrt(a^2 + b^2)``, ``M1 = |x| + |mean| + |std z1|``, ``M2 = |mean| + |std z2|``:
    ``a`` is three roundings of intermediates below ``M1`` (|da| <= 3 u M1), ``b`` two below ``M2`` (taken as 3 u M2);
    ``dy <= (|a| da + |b| db) / y + (u/2 + u/2 + u) y <= da + db + 2 u y``: forward tolerance ``E (1.5 (M1 + M2) + y)``.
    The backward is ``grad * a / y`` with the float32 ``y``: ``d(a / y) <= da / y + |a| dy / y^2 <= (2 da + db) / y + 2 u |a / y|``,
    the division and the product one rounding each: ``|grad| E ((3 M1 + 1.5 M2) / y + 2 |a / y|)``."""
    shape = (-1, 1, 1, 1, 1)
    mean64 = mean.double().view(shape) if isinstance(mean, torch.Tensor) else float(torch.tensor(mean, dtype=torch.float32))
    std64 = std.double().view(shape) if isinstance(std, torch.Tensor) else float(torch.tensor(std, dtype=torch.float32))
    rows = torch.ones(SHAPE[0], dtype=torch.bool) if keep is None else keep.bool()

    def formula(leaf):
        noisy = torch.sqrt((leaf + (mean64 + std64 * z1.double())) ** 2 + (mean64 + std64 * z2.double()) ** 2)
        return torch.where(rows.view(shape), noisy, leaf)

    out, reference = _float64_backward(formula, data, grad)
    zeros = torch.zeros(SHAPE, dtype=torch.float64)
    m1 = data.double().abs() + (zeros + mean64).abs() + (std64 * z1.double()).abs()
    m2 = (zeros + mean64).abs() + (std64 * z2.double()).abs()
    a = data.double() + (mean64 + std64 * z1.double())
    forward_tolerance = E * (1.5 * (m1 + m2) + out)
    backward_tolerance = grad.double().abs() * E * ((3 * m1 + 1.5 * m2) / out + 2 * (a / out).abs())
    forward_tolerance[~rows] = 0  # gated-out rows: copies, slope exactly 1
    backward_tolerance[~rows] = 0
    return out, reference, forward_tolerance, backward_tolerance


def _rician(engine, device, philox, per_element, with_keep):
    data, grad, g = _inputs(8 + per_element)
    mean = torch.tensor([0.05, -0.1, 0.2]) if per_element else 0.1
    std = torch.tensor([0.3, 0.15, 0.25]) if per_element else 0.2
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8) if with_keep else None
    seed = 20261017
    if philox:  # the draws the kernel makes: stream 0 and stream 1 of its seed, by flat index of the whole batch
        z1, z2 = (engine.philox_normal(SHAPE, seed, stream, device).cpu() for stream in (0, 1))
        assert abs(float(z1.mean())) < 0.05 and abs(float(z1.std()) - 1) < 0.05 and not torch.equal(z1, z2)
    else:
        z1, z2 = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)

    def op(e, leaf, dev):
        if philox:
            return e.add_noise(leaf, mean, std, rician=True, philox_seed=seed, keep=None if keep is None else keep.to(dev))
        return e.add_noise(leaf, mean, std, rician=True, base1=z1.to(dev), base2=z2.to(dev), keep=None if keep is None else keep.to(dev))

    expected, reference, forward_tolerance, backward_tolerance = _rician_reference(data, grad, mean, std, z1, z2, keep)
    out, result = _engine_backward(engine, device, op, data, grad)
    # the forward first: a draw in the kernel that is not `philox_normal`'s shows here, not as a wrong slope
    _assert_per_voxel(out, expected, forward_tolerance, "rician forward")
    _assert_per_voxel(result, reference, backward_tolerance, "rician backward")
    if with_keep:
        assert torch.equal(out[1], data[1]) and torch.equal(result[1], grad[1])  # slope exactly 1 on the gated-out row
        assert not torch.equal(result[0], grad[0])


# -- flip / pad -------------------------------------------------------------------------------------------------------------
def _flip(engine, device):
    """A permutation: the gradient is the same permutation of the incoming gradient, bit for bit."""
    data, grad, _ = _inputs(10)
    flags = torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 1]], dtype=torch.uint8)
    for axes, per_element in (((0, 2), None), (None, flags), ((1,), flags)):
        def op(e, leaf, dev, axes=axes, per_element=per_element):
            return e.flip3d(leaf, axes, None if per_element is None else per_element.to(dev))

        def formula(leaf, axes=axes, per_element=per_element):
            rows = []
            for b in range(SHAPE[0]):
                mask = [False] * 3
                for axis in axes or ():
                    mask[axis] = True
                if per_element is not None:  # (flags given: they decide, as in the kernel)
                    mask = [bool(v) for v in per_element[b]]
                dims = [1 + d for d in range(3) if mask[d]]
                rows.append(torch.flip(leaf[b], dims) if dims else leaf[b])
            return torch.stack(rows)

        expected, reference = _float64_backward(formula, data, grad)
        out, result = _engine_backward(engine, device, op, data, grad)
        assert torch.equal(out.double(), expected), "the flip test's own formula does not describe the forward"
        assert torch.equal(result.double(), reference)


def _pad(engine, device):
    """Constant padding with per-element fills: the data's gradient is the interior of the incoming one (equality); each fill's
    gradient is the sum over its element's border, computed as the sum of everything minus the sum of the interior: two float32
    sums of ``n`` and ``m`` terms in whatever order, within ``(n - 1) u sum|g|`` and ``(m - 1) u sum|g_inner|``, one subtraction."""
    data, _, g = _inputs(11)
    padding = (2, 1, 0, 3, 4, 2)
    fills = torch.tensor([0.5, -1.0, 2.0])
    padded = (SHAPE[0], SHAPE[1], SHAPE[2] + 3, SHAPE[3] + 3, SHAPE[4] + 6)
    grad = torch.randn(padded, generator=g)
    leaf, fill_leaf = data.to(device).requires_grad_(True), fills.to(device).requires_grad_(True)
    out = engine.pad3d(leaf, padding, "constant", 0.0, fill_leaf)
    grad_data, grad_fill = torch.autograd.grad(out, [leaf, fill_leaf], grad.to(device))
    leaf64, fill64 = data.double().requires_grad_(True), fills.double().requires_grad_(True)
    expected = fill64.view(-1, 1, 1, 1, 1).expand(padded).clone()
    expected[:, :, 2 : 2 + SHAPE[2], 0 : SHAPE[3], 4 : 4 + SHAPE[4]] = leaf64
    reference_data, reference_fill = torch.autograd.grad(expected, [leaf64, fill64], grad.double())
    assert torch.equal(out.detach().cpu().double(), expected.detach())
    assert torch.equal(grad_data.cpu().double(), reference_data)
    inner = grad[:, :, 2 : 2 + SHAPE[2], 0 : SHAPE[3], 4 : 4 + SHAPE[4]].double().abs().sum(dim=(1, 2, 3, 4))
    everything = grad.double().abs().sum(dim=(1, 2, 3, 4))
    n, m = grad[0].numel(), data[0].numel()
    tolerance = (E / 2) * ((n - 1) * everything + (m - 1) * inner + (everything + inner))
    assert grad_fill.shape == fills.shape and grad_fill.dtype == fills.dtype
    _assert_per_voxel(grad_fill.cpu(), reference_fill, tolerance, "gradient of the fills")
    assert float(reference_fill.abs().min()) > 0


# radii 9 - 16 along I and J (the forward's fused J + K pass and its I pass take them; the adjoint tests stopped at 8)
WIDE_STENCILS = [
    ((2, 1, 40, 36, 20), (9, 16, 3), True, None),
    ((1, 2, 24, 40, 33), (16, 12, 0), False, None),
    ((2, 1, 20, 18, 70), (13, 9, 8), True, [0, 1]),
    ((1, 1, 7, 10, 12), (16, 11, 2), False, None),  # extents below the radius
]


# -- the CPU half: the same checkers on the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("divide", [False, True])
def test_oracle_bias_field_backward(oracle, divide):
    _bias_field(oracle, "cpu", oracle, divide)


@pytest.mark.parametrize("per_element", [False, True])
def test_oracle_gamma_backward(oracle, per_element):
    _gamma(oracle, "cpu", oracle, per_element)


def test_oracle_gaussian_noise_backward(oracle):
    _gaussian_noise(oracle, "cpu")


@pytest.mark.parametrize("philox", [False, True])
@pytest.mark.parametrize("per_element,with_keep", [(False, False), (True, True), (False, True)])
def test_oracle_rician_backward(oracle, philox, per_element, with_keep):
    _rician(oracle, "cpu", philox, per_element, with_keep)


def test_oracle_flip_and_pad_backward(oracle):
    _flip(oracle, "cpu")
    _pad(oracle, "cpu")


@pytest.mark.parametrize("case", WIDE_STENCILS)
def test_oracle_stencil_adjoint_at_wide_radii(oracle, case):
    stencil._check(oracle, "cpu", case)


# -- the GPU half -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("divide", [False, True])
def test_hip_bias_field_backward(hip, oracle, divide):
    _bias_field(hip, "cuda", oracle, divide)


@pytest.mark.gpu
@pytest.mark.parametrize("per_element", [False, True])
def test_hip_gamma_backward(hip, oracle, per_element):
    _gamma(hip, "cuda", oracle, per_element)


@pytest.mark.gpu
def test_hip_gaussian_noise_backward(hip):
    _gaussian_noise(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("philox", [False, True])
@pytest.mark.parametrize("per_element,with_keep", [(False, False), (True, True), (False, True)])
def test_hip_rician_backward(hip, philox, per_element, with_keep):
    _rician(hip, "cuda", philox, per_element, with_keep)


@pytest.mark.gpu
def test_hip_flip_and_pad_backward(hip):
    _flip(hip, "cuda")
    _pad(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_STENCILS)
def test_hip_stencil_adjoint_at_wide_radii(hip, oracle, case):
    stencil._check(hip, "cuda", case, other=oracle)
