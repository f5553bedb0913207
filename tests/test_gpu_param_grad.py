"""GPU: the parameter gradients of the intensity ops - ``tio_bias_field_grad``, ``tio_gamma_grad``, ``tio_noise_grad``,
``tio_separable_conv3d_taps_grad`` - per component against float64 autograd through the reference's own compositions
(``param_grad_reference``: the reference, ``A_p`` and the count ``c`` of float32 roundings behind the bound
``(tau + c 2^-24) A_p + 2^-24 |ref|``), known answers held to equality, and the plumbing above the kernels: the ``Engine`` forwards
with parameter leaves, ``torch.ops.tio_hip``, ``torchio_amd.functional``.

Largest ``error / bound`` per family on the MI355X (every run prints each case's with ``-s``); a ratio above 1 would mean that a
kernel or the count of its roundings is wrong:

    family (cases)                           largest ratio     at
    bias (12)                                0.081             full-resolution (the direct road); the box road: 0.026
    gamma (7)                                0.022             batched-64
    noise, additive, d_mean (c = 0)          0.91              additive-batched: the one float32 rounding of the result
    noise, additive, d_std                   0.11              additive-keep
    noise, Rician, explicit draws            0.0066            rician-batched-zeros d_std
    noise, Philox draws regenerated          0.093 / 0.0025    additive-batched d_std / rician-keep d_mean
    taps (9)                                 0.0074            r040-short-axis
    between guards, any family               as above (the same values)

The additive ``d_mean`` sums ``gy`` itself: no float32 rounding precedes the last one, so its bound is ``2^-24 |ref|`` alone and a
ratio close to 1 is the rounding of the result to float32, not an error that could grow.
"""
from __future__ import annotations

import pytest
import torch

import param_grad_reference as reference
import torchio_amd as tio
from param_grad_reference import TAU
from torchio_amd._lib import EngineError

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


def _dev(tensor):
    return None if tensor is None else tensor.to(DEVICE)


def _same(first, second) -> bool:
    """Two runs of a kernel on the same inputs: equal up to the last float32 rounding (the float64 atomics have no fixed order)."""
    first, second = first.detach().cpu().double(), second.detach().cpu().double()
    return first.shape == second.shape and bool(((first - second).abs() <= torch.maximum(first.abs(), second.abs()) * 2.0 ** -23).all())


# ---------------------------------------------------------------------------------------------------------------------
# bias
# ---------------------------------------------------------------------------------------------------------------------
def _bias(engine, case):
    return engine.bias_field_grad(_dev(case["x"]), _dev(case["gy"]), _dev(case["coarse"]), divide=case["divide"], skip=_dev(case["skip"]))


@pytest.mark.parametrize("name", sorted(reference.BIAS_CASES))
def test_the_coarse_grid_gradient_is_within_its_bound(hip, name):
    case = reference.bias_case(name)
    got = _bias(hip, case)
    assert got.shape == case["coarse"].shape and got.dtype == torch.float32
    reference.check(f"bias {name}", got, case["ref"], case["a"], case["c"], TAU)
    assert _same(got, _bias(hip, case))
    if case["skip"] is not None:  # a skipped element is exactly zero while its neighbours are not
        rows = case["skip"].bool()
        assert bool((got.cpu()[rows] == 0).all()) and bool((got.cpu()[~rows] != 0).any(dim=(1, 2, 3, 4)).all())


def test_a_zero_bias_on_dyadic_weights_equals_float64_autograd(hip):
    """``coarse == 0``: the field is ``expf(0) == 1``; a 2-node grid on extents ``2^n + 1`` has lerp weights that are multiples of
    1/4, 1/2 and 1/8, exact in float32 and in the float64 reference; with small integers in ``x`` and ``gy`` every product and every
    sum is exact: the kernel must agree with float64 autograd to the last bit (multiply and divide, both roads: the 2 x 2 x 2 box
    and, on the full-resolution grid of extent == nodes, the direct one)."""
    g = torch.Generator().manual_seed(11)
    shape = (2, 2, 5, 3, 9)
    x = torch.randint(-8, 9, shape, generator=g).float()
    gy = torch.randint(-4, 5, shape, generator=g).float()
    for coarse_shape in ((2, 2, 2), (5, 3, 9)):
        coarse = torch.zeros(2, 2, *coarse_shape)
        for divide in (False, True):
            ref, _ = reference.bias(x, gy, coarse, divide)
            got = hip.bias_field_grad(_dev(x), _dev(gy), _dev(coarse), divide=divide)
            assert float(ref.abs().max()) > 0 and torch.equal(got.cpu().double(), ref), (coarse_shape, divide)


# ---------------------------------------------------------------------------------------------------------------------
# gamma
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(reference.GAMMA_CASES))
def test_the_exponent_gradient_is_within_its_bound(hip, name):
    case = reference.gamma_case(name)
    got = hip.gamma_grad(_dev(case["x"]), _dev(case["gy"]), _dev(case["gamma"]))
    assert got.shape == case["gamma"].shape and got.dtype == torch.float32
    reference.check(f"gamma {name}", got, case["ref"], case["a"], reference.C_GAMMA, TAU)
    if case["gamma"].numel() == 1:  # the shared exponent as a host tensor and as a plain number: the same launch arguments' values
        assert _same(got, hip.gamma_grad(_dev(case["x"]), _dev(case["gy"]), case["gamma"]))
        assert _same(got, hip.gamma_grad(_dev(case["x"]), _dev(case["gy"]), float(case["gamma"].float())))


def test_exact_zeros_add_nothing_to_the_exponent_gradient(hip):
    x = torch.zeros(2, 1, 1, 1, 130)
    x[1, 0, 0, 0, 5] = 2.0
    gy = torch.ones_like(x)
    got = hip.gamma_grad(_dev(x), _dev(gy), torch.tensor([1.5, 2.0])).cpu()
    assert float(got[0]) == 0.0 and abs(float(got[1]) - 4.0 * 0.6931471805599453) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------
def _noise(engine, case, z1, z2, **extra):
    return engine.noise_grad(_dev(case["x"]), _dev(case["gy"]), _dev(case["mean"]), _dev(case["std"]), rician=case["rician"], base1=_dev(z1),
                             base2=_dev(z2), keep=_dev(case["keep"]), **extra)


def _check_noise(label, case, d_mean, d_std, mean_ref, std_ref):
    c_mean, c_std = reference.noise_c(case)
    if d_mean is not None:
        assert d_mean.shape == case["mean"].shape
        reference.check(f"noise {label} d_mean", d_mean, *mean_ref, c_mean, 0.0)
    if d_std is not None:
        assert d_std.shape == case["std"].shape
        reference.check(f"noise {label} d_std", d_std, *std_ref, c_std, 0.0)


@pytest.mark.parametrize("name", sorted(reference.NOISE_CASES))
def test_the_noise_gradients_with_explicit_draws_are_within_their_bounds(hip, name):
    case = reference.noise_case(name)
    d_mean, d_std = _noise(hip, case, case["z1"], case["z2"])
    _check_noise(name, case, d_mean, d_std, case["mean_ref"], case["std_ref"])
    if case["keep"] is not None:
        gated = ~case["keep"].bool()
        assert bool((d_mean.cpu()[gated] == 0).all()) and bool((d_std.cpu()[gated] == 0).all()) and bool((d_std.cpu()[~gated] != 0).all())
    only_mean, none = _noise(hip, case, case["z1"], case["z2"], want_std=False)
    assert none is None and _same(only_mean, d_mean)
    none, only_std = _noise(hip, case, case["z1"], case["z2"], want_mean=False)
    assert none is None and _same(only_std, d_std)
    if not case["rician"]:  # additive noise does not read x
        without_x = hip.noise_grad(torch.zeros_like(_dev(case["x"])), _dev(case["gy"]), _dev(case["mean"]), _dev(case["std"]), base1=_dev(case["z1"]),
                                   keep=_dev(case["keep"]))
        assert _same(without_x[0], d_mean) and _same(without_x[1], d_std)


@pytest.mark.parametrize("name", ["additive-scalar", "additive-batched", "rician-scalar", "rician-keep", "rician-float64"])
def test_the_philox_draws_are_regenerated_bit_for_bit(hip, name):
    """With ``base1 == None`` the kernel draws ``z`` itself: the result equals the explicit-draw launch on ``tio_philox_normal``'s
    own output (stream ids 0 and 1) up to the two-run rule, and meets the bound against the reference on those draws.
    (``additive-scalar``, ``rician-scalar``, ``rician-keep``: 105 values per element - rows that do not start on a Philox block.)"""
    case = reference.noise_inputs(name)
    seed = 0x1234_5678_9ABC_DEF0 + len(name)
    z1 = hip.philox_normal(case["shape"], seed, 0, DEVICE)
    z2 = hip.philox_normal(case["shape"], seed, 1, DEVICE) if case["rician"] else None
    regenerated = hip.noise_grad(_dev(case["x"]), _dev(case["gy"]), _dev(case["mean"]), _dev(case["std"]), rician=case["rician"], philox_seed=seed,
                                 keep=_dev(case["keep"]))
    explicit = _noise(hip, case, z1, z2)
    assert _same(regenerated[0], explicit[0]) and _same(regenerated[1], explicit[1])
    mean_ref, std_ref = reference.noise(case["x"], case["gy"], case["mean"], case["std"], z1, z2, case["rician"], case["keep"])
    _check_noise(f"{name} philox", case, *regenerated, mean_ref, std_ref)


def test_a_single_mean_next_to_per_element_deviations_receives_the_batch_sum(hip):
    case = reference.noise_case("additive-batched")
    shared = torch.tensor([0.25])
    d_mean, d_std = hip.noise_grad(_dev(case["x"]), _dev(case["gy"]), shared, _dev(case["std"]), base1=_dev(case["z1"]))
    (mean_ref, mean_a), std_ref = reference.noise(case["x"], case["gy"], shared, case["std"], case["z1"])
    assert d_mean.shape == (1,) and d_std.shape == case["std"].shape
    reference.check("noise mixed d_mean", d_mean, mean_ref, mean_a, 1, 0.0)  # one more float32 rounding: the per-element sums are float32
    reference.check("noise mixed d_std", d_std, *std_ref, 1, 0.0)


def test_integer_draws_equal_float64_autograd(hip):
    g = torch.Generator().manual_seed(12)
    shape = (3, 1, 3, 5, 7)
    gy = torch.randint(-4, 5, shape, generator=g).float()
    z = torch.randint(-3, 4, shape, generator=g).float()
    for mean, std in ((torch.tensor([1.0, -2.0, 0.0]), torch.tensor([2.0, 1.0, 3.0])), (torch.tensor([1.0]), torch.tensor([2.0]))):
        (mean_ref, _), (std_ref, _) = reference.noise(None, gy, mean, std, z)
        d_mean, d_std = hip.noise_grad(torch.zeros(shape, device=DEVICE), _dev(gy), mean, std, base1=_dev(z))
        assert float(std_ref.abs().max()) > 0
        assert torch.equal(d_mean.cpu().double(), mean_ref) and torch.equal(d_std.cpu().double(), std_ref)


# ---------------------------------------------------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------------------------------------------------
def _taps(engine, case):
    return engine.separable_conv3d_taps_grad(_dev(case["x"]), _dev(case["gy"]), _dev(case["taps"]), case["radius"], skip=_dev(case["skip"]))


@pytest.mark.parametrize("name", sorted(reference.TAPS_CASES))
def test_the_tap_gradient_is_within_its_bound(hip, name):
    case = reference.taps_case(name)
    got = _taps(hip, case)
    assert got.shape == case["taps"].shape and got.dtype == torch.float32
    reference.check(f"taps {name}", got, case["ref"], case["a"], case["c"], 0.0)
    assert _same(got, _taps(hip, case))
    host = got.cpu()
    for axis, r in enumerate(case["radius"]):  # zero beyond 2 r + 1 and on inactive axes; skipped rows of batched taps are zero
        assert bool((host[:, axis, (2 * r + 1 if r > 0 else 0):] == 0).all())
    if case["skip"] is not None and case["taps"].shape[0] > 1:
        rows = case["skip"].bool()
        assert bool((host[rows] == 0).all()) and bool((host[~rows] != 0).any(dim=(1, 2)).all())


def test_integer_data_under_dyadic_taps_equals_float64_autograd(hip):
    """Taps that are multiples of 1/4, integer data and gradients: every intermediate of the stencil passes, every product and every
    sum is exact in float32 and in float64.  J = 2 under radius 2 folds taps at both borders."""
    g = torch.Generator().manual_seed(13)
    shape = (2, 2, 5, 2, 9)
    x = torch.randint(-8, 9, shape, generator=g).float()
    gy = torch.randint(-4, 5, shape, generator=g).float()
    taps = torch.zeros(2, 3, 5)
    taps[:, 0, :3] = torch.tensor([[0.25, 0.5, 0.25], [0.5, 0.5, 0.0]])
    taps[:, 1, :5] = torch.tensor([[0.25, 0.0, 0.5, 0.25, 0.0], [0.0, 0.25, 0.25, 0.25, 0.25]])
    taps[:, 2, :3] = torch.tensor([[0.0, 0.75, 0.25], [0.25, 0.5, 0.25]])
    for weights in (taps, taps[:1]):
        ref, _ = reference.taps(x, gy, weights, [1, 2, 1])
        got = hip.separable_conv3d_taps_grad(_dev(x), _dev(gy), _dev(weights), [1, 2, 1])
        assert float(ref.abs().max()) > 0 and torch.equal(got.cpu().double(), ref)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_the_forwards_attach_the_parameter_backward_next_to_the_data_backward(hip):
    """One ``backward()`` delivers the data gradient and the parameter gradient; the parameter's arrives in the leaf's dtype on the
    leaf's device (a host float64 leaf here), and equals the explicit engine call; the forward's values are the plain call's."""
    bias, gam, noi, tap = reference.bias_case("ragged-k70"), reference.gamma_case("batched-64"), reference.noise_case("rician-scalar"), reference.taps_case("r123-batched")
    runs = [
        (lambda x, p: hip.bias_field_apply(x, p), bias["x"], bias["coarse"], bias["gy"], lambda: _bias(hip, bias)),
        (lambda x, p: hip.gamma_pow(x, p), gam["x"], gam["gamma"], gam["gy"], lambda: hip.gamma_grad(_dev(gam["x"]), _dev(gam["gy"]), gam["gamma"])),
        (lambda x, p: hip.add_noise(x, noi["mean"], p, rician=True, base1=_dev(noi["z1"]), base2=_dev(noi["z2"])), noi["x"], noi["std"], noi["gy"],
         lambda: _noise(hip, noi, noi["z1"], noi["z2"])[1]),
        (lambda x, p: hip.separable_conv3d(x, p, tap["radius"]), tap["x"], tap["taps"], tap["gy"], lambda: _taps(hip, tap)),
    ]
    for forward, x, parameter, gy, explicit in runs:
        data = _dev(x).requires_grad_(True)
        leaf = parameter.double().requires_grad_(True)  # host, float64
        out = forward(data, leaf)
        with torch.no_grad():
            plain = forward(_dev(x), _dev(parameter))
        assert torch.equal(out.detach(), plain) and out.requires_grad
        (out * _dev(gy)).sum().backward()
        assert leaf.grad.dtype == torch.float64 and leaf.grad.device.type == "cpu" and leaf.grad.shape == leaf.shape
        assert _same(leaf.grad, explicit().reshape(leaf.shape)) and float(leaf.grad.abs().max()) > 0
        assert data.grad is not None and data.grad.shape == data.shape and float(data.grad.abs().max()) > 0
        only_data = _dev(x).requires_grad_(True)
        (forward(only_data, _dev(parameter)) * _dev(gy)).sum().backward()
        assert torch.equal(only_data.grad, data.grad)  # the data's own backward is the one it had


def test_a_second_differentiation_raises(hip):
    case = reference.gamma_case("batched-64")
    leaf = _dev(case["gamma"]).requires_grad_(True)
    out = hip.gamma_pow(_dev(case["x"]), leaf)
    with pytest.raises(EngineError, match="cannot be differentiated again"):
        torch.autograd.grad((out * _dev(case["gy"])).sum(), leaf, create_graph=True)


def test_functional_and_the_custom_ops_give_the_engines_gradients(hip):
    import torchio_amd.torch_ops  # noqa: F401, PLC0415

    F = tio.functional
    bias, gam, tap = reference.bias_case("divide"), reference.gamma_case("scalar-4099"), reference.taps_case("r123-shared")
    additive, rician = reference.noise_case("additive-batched"), reference.noise_inputs("rician-scalar")

    def grads(forward, gy, *leaves):
        leaves = [leaf.clone().requires_grad_(True) for leaf in leaves]
        (forward(*leaves) * _dev(gy)).sum().backward()
        return [leaf.grad for leaf in leaves]

    # bias
    expected = _bias(hip, bias)
    assert _same(grads(lambda c: F.bias_field(_dev(bias["x"]), c, divide=True), bias["gy"], bias["coarse"])[0], expected)
    assert _same(grads(lambda c: torch.ops.tio_hip.bias_field_apply(_dev(bias["x"]), c, True), bias["gy"], _dev(bias["coarse"]))[0], expected)
    # gamma
    expected = hip.gamma_grad(_dev(gam["x"]), _dev(gam["gy"]), gam["gamma"])
    assert _same(grads(lambda e: F.gamma(_dev(gam["x"]), e), gam["gy"], gam["gamma"])[0], expected)
    assert _same(grads(lambda e: torch.ops.tio_hip.gamma_pow(_dev(gam["x"]), e), gam["gy"], gam["gamma"])[0], expected)
    # noise: explicit draws, and Rician with Philox draws (regenerated in the backward pass; the data gradient as well)
    expected = _noise(hip, additive, additive["z1"], None)
    got = grads(lambda m, s: F.noise(_dev(additive["x"]), m, s, draws=additive["z1"]), additive["gy"], additive["mean"], additive["std"])
    assert _same(got[0], expected[0]) and _same(got[1], expected[1])
    got = grads(lambda m, s: torch.ops.tio_hip.add_noise(_dev(additive["x"]), m, s, False, _dev(additive["z1"])), additive["gy"], _dev(additive["mean"]), _dev(additive["std"]))
    assert _same(got[0], expected[0]) and _same(got[1], expected[1])
    expected = hip.noise_grad(_dev(rician["x"]), _dev(rician["gy"]), rician["mean"], rician["std"], rician=True, philox_seed=99)
    got = grads(lambda m, s: F.noise(_dev(rician["x"]), m, s, seed=99, rician=True), rician["gy"], rician["mean"], rician["std"])
    assert _same(got[0], expected[0]) and _same(got[1], expected[1])
    data = _dev(rician["x"]).requires_grad_(True)
    got = grads(lambda m, s: torch.ops.tio_hip.add_noise(data, m, s, True, None, None, 99), rician["gy"], rician["mean"], rician["std"])
    assert _same(got[0], expected[0]) and _same(got[1], expected[1])
    engine_data = _dev(rician["x"]).requires_grad_(True)
    (hip.add_noise(engine_data, rician["mean"], rician["std"], rician=True, philox_seed=99) * _dev(rician["gy"])).sum().backward()
    torch.testing.assert_close(data.grad, engine_data.grad, rtol=1e-6, atol=1e-6)
    # taps, and the sigmas behind them
    expected = _taps(hip, tap)
    assert _same(grads(lambda w: torch.ops.tio_hip.separable_conv3d(_dev(tap["x"]), w, tap["radius"]), tap["gy"], _dev(tap["taps"]))[0], expected)
    sigmas = torch.tensor([1.1, 0.6, 0.9], dtype=torch.float64)
    (from_blur,) = grads(lambda s: F.blur(_dev(tap["x"]), s), tap["gy"], sigmas)
    leaf = sigmas[None].clone().requires_grad_(True)
    weights, radius, _ = F._gaussian_taps(leaf, False)
    d_weights = hip.separable_conv3d_taps_grad(_dev(tap["x"]), _dev(tap["gy"]), weights.detach(), radius)
    (by_hand,) = torch.autograd.grad(weights, leaf, d_weights.cpu())
    torch.testing.assert_close(from_blur, by_hand.reshape(3), rtol=1e-6, atol=1e-9)
    assert from_blur.dtype == torch.float64 and bool((from_blur != 0).all())


def test_the_custom_ops_pass_opcheck_with_parameters_that_require_a_gradient(hip):
    import torchio_amd.torch_ops  # noqa: F401, PLC0415

    g = torch.Generator(device=DEVICE).manual_seed(3)
    x = torch.rand(2, 1, 6, 5, 12, generator=g, device=DEVICE) + 0.2
    grad = torch.rand(x.shape, generator=g, device=DEVICE)
    coarse = torch.randn(2, 1, 3, 3, 3, generator=g, device=DEVICE) * 0.2
    taps = torch.tensor([[[0.25, 0.5, 0.25]] * 3], device=DEVICE)
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    torch.library.opcheck(torch.ops.tio_hip.bias_field_apply, (leaf(x), leaf(coarse)))
    torch.library.opcheck(torch.ops.tio_hip.gamma_pow, (leaf(x), leaf(torch.tensor([0.8, 1.3], device=DEVICE))))
    torch.library.opcheck(torch.ops.tio_hip.add_noise, (leaf(x), leaf(torch.tensor(0.1)), leaf(torch.tensor(0.3)), False, None, None, 7))
    torch.library.opcheck(torch.ops.tio_hip.add_noise, (leaf(x), leaf(torch.tensor(0.1)), leaf(torch.tensor(0.3)), True, None, None, 7))
    torch.library.opcheck(torch.ops.tio_hip.separable_conv3d, (leaf(x), leaf(taps), [1, 1, 1]))
    torch.library.opcheck(torch.ops.tio_hip.bias_field_grad, (x, grad, coarse, True, None))
    torch.library.opcheck(torch.ops.tio_hip.gamma_grad, (x, grad, torch.tensor([0.8, 1.3], device=DEVICE)))
    torch.library.opcheck(torch.ops.tio_hip.noise_grad, (x, grad, torch.tensor([0.1]), torch.tensor([0.3, 0.4], device=DEVICE), True, None, None, 7, None))
    torch.library.opcheck(torch.ops.tio_hip.separable_conv3d_taps_grad, (x, grad, taps, [1, 1, 1], None))


def test_five_adam_steps_on_a_coarse_bias_grid_lower_the_error(hip):
    """The README's loop: recover a smooth bias field from a biased image."""
    g = torch.Generator().manual_seed(21)
    clean = _dev(torch.rand(1, 1, 17, 18, 40, generator=g) + 0.5)
    truth = _dev((torch.rand(1, 1, 3, 3, 3, generator=g) - 0.5) * 0.6)
    with torch.no_grad():
        biased = tio.functional.bias_field(clean, truth)
    coarse = torch.zeros(1, 1, 3, 3, 3, device=DEVICE, requires_grad=True)
    optimiser = torch.optim.Adam([coarse], lr=0.05)
    losses = []
    for _ in range(5):
        optimiser.zero_grad()
        loss = ((tio.functional.bias_field(clean, coarse) - biased) ** 2).mean()
        loss.backward()
        optimiser.step()
        losses.append(float(loss))
    assert all(later < earlier for earlier, later in zip(losses, losses[1:], strict=False)), losses
    assert losses[-1] < 0.7 * losses[0], losses
