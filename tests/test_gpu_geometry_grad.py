"""GPU: ``tio_resample3d_geometry_grad`` - the gradient of the trilinear resampling with respect to the mapping and the control
points - per component against float64 autograd (``geometry_grad_reference``: the reference, the rounding bound ``R_p`` and the kink
allowance ``K_p``; the host test shows that every case meets the conditions of the allowance), known answers held to equality, and
the plumbing above the kernel: ``Engine.resample3d`` with geometry leaves, ``torch.ops.tio_hip``, ``torchio_amd.warp``.

Largest ``error / (R_p + K_p)`` seen on the MI355X per case (every run prints them with ``-s``); a ratio above 1 would mean that the
kernel or the count of its roundings is wrong.  The ratios are small because ``R_p`` is dominated by the ``60 u c`` a sampling
coordinate is allowed, of which the kernel's chain uses a small part:

    case                    d_mapping   d_control
    1-batched               0.00016     0.0024
    2-chained-spacing       0.00018     0.0036
    3-shared                0.00012     0.0063
    4-flags                 0.00032     0.001
    5-out-of-bounds         0.00024     0.0088
    5-out-of-bounds-fill    0.00026     0.0032
    6-norm-shape            0.00019     0.0017
    7-two-dimensional       0.00018     0.0046
    8-ko70                  9e-06       0.00021
    8-ko3                   0.00012     0.0025
    9-two-images            0.00023     0.002
    9-dtypes                0.0001      0.0024
    10-many-blocks          4.8e-06     0.00094
"""
from __future__ import annotations

import pytest
import torch

import geometry_grad_reference as reference
import torchio_amd as tio
from adjoint_reference import _launch_arguments
from adjoint_reference import geometry
from adjoint_reference import on_device
from torchio_amd import ops

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


def _explicit(engine, geo, images, grads, fills, **extra):
    geo = on_device(geo, DEVICE)
    return engine.resample3d_geometry_grad([x.to(DEVICE) for x in images], [g.to(DEVICE) for g in grads],
                                           fills=[None if f is None else f.to(DEVICE) for f in fills], **_launch_arguments(geo), **extra)


def _run_case(engine, case, **extra):
    return _explicit(engine, case["geo"], case["images"], case["grads"], case["fills"], **extra)


@pytest.mark.parametrize("name", reference.CASE_NAMES)
def test_every_component_is_within_its_rounding_bound_and_kink_allowance(hip, name):
    case = reference.case(name)
    d_mapping, d_control = _run_case(hip, case)
    reference.check(case, d_mapping, d_control)
    if name == "4-flags":  # skipped rows are exactly zero; the element without control points still moves its mapping
        assert bool((d_mapping[2] == 0).all()) and bool((d_control[1:] == 0).all()) and bool((d_mapping[1] != 0).any())
    if name == "7-two-dimensional":
        assert bool((d_mapping[:, 0] == 0).all()) and bool((d_control[..., 0] == 0).all())


def test_only_the_wanted_gradient_is_computed_and_it_is_the_same(hip):
    case = reference.case("1-batched")
    both = _run_case(hip, case)
    only_mapping = _run_case(hip, case, want_control_points=False)
    only_control = _run_case(hip, case, want_mapping=False)
    assert only_mapping[1] is None and only_control[0] is None
    reference.check(case, only_mapping[0], both[1])
    reference.check(case, both[0], only_control[1])


def _same(first, second) -> bool:
    """Two runs of the kernel on the same inputs: equal up to the last float32 rounding (the float64 atomics have no fixed order)."""
    first, second = first.detach().cpu().double(), second.detach().cpu().double()
    return bool(((first - second).abs() <= torch.maximum(first.abs(), second.abs()) * 2.0 ** -23).all())


def _integer_case():
    """The identity on integer coordinates: every coordinate sits ON a voxel, the last one on ``S - 1``.  Extents of 2^n + 1 and a
    2-node control grid make the normalisation (2 / (S - 1)) and the lerp weights (multiples of 1/4, 1/2, 1/8) exact in float32 AND in
    the float64 reference, and with the small integers below every product and every sum is exact: the kernel must agree with
    float64 autograd to the last bit."""
    generator = torch.Generator().manual_seed(5)
    shape = (5, 3, 9)
    image = torch.randint(-8, 9, (2, 2, *shape), generator=generator).float()
    grad = torch.randint(-4, 5, (2, 2, *shape), generator=generator).float()
    mapping = torch.eye(3, 4)[None].repeat(2, 1, 1)
    control = torch.zeros(1, 2, 2, 2, 3)
    return geometry(in_shape=shape, out_shape=shape, mapping=mapping, control_points=control), image, grad


def test_the_identity_on_integer_coordinates_equals_float64_autograd(hip):
    """Pins the ``floor`` cell at exact integers and at ``S - 1``: the derivative there is the one-sided difference towards the upper
    neighbour, zero-padded beyond the volume (ATen's rule)."""
    geo, image, grad = _integer_case()
    d_mapping, d_control = _explicit(hip, geo, [image], [grad], [None])
    expected_mapping, expected_control = reference.autograd_reference(geo, [image], [grad], [None])
    assert float(expected_mapping.abs().max()) > 0 and float(expected_control.abs().max()) > 0
    assert torch.equal(d_mapping.cpu().double(), expected_mapping)
    assert torch.equal(d_control.cpu().double(), expected_control)
    no_control = geometry(in_shape=geo["in_shape"], out_shape=geo["out_shape"], mapping=geo["mapping"])
    alone, none = _explicit(hip, no_control, [image], [grad], [None])
    assert none is None and torch.equal(alone, d_mapping)


def test_known_zeros_and_full_overwrite(hip):
    case = reference.case("1-batched")
    geo = dict(case["geo"])
    # everything out of bounds: all zeros
    away = geo["mapping"].clone()
    away[:, :, 3] += 100.0
    d_mapping, d_control = _explicit(hip, {**geo, "mapping": away}, case["images"], case["grads"], case["fills"])
    assert bool((d_mapping == 0).all()) and bool((d_control == 0).all())
    # g = 0: all zeros
    d_mapping, d_control = _explicit(hip, geo, case["images"], [torch.zeros_like(g) for g in case["grads"]], case["fills"])
    assert bool((d_mapping == 0).all()) and bool((d_control == 0).all())


def test_outputs_filled_with_nan_are_overwritten_and_two_calls_agree_to_an_ulp(hip):
    """The C entry point itself: caller-owned outputs that hold NaN, ONE workspace used twice (its contents on entry do not matter)."""
    import ctypes as C  # noqa: PLC0415

    from torchio_amd import _abi  # noqa: PLC0415

    case = reference.case("10-many-blocks")
    geo = on_device(case["geo"], DEVICE)
    image, grad = case["images"][0].to(DEVICE).contiguous(), case["grads"][0].to(DEVICE).contiguous()
    geom, keep = hip._resample_geom(image.shape[0], geo["in_shape"], geo["out_shape"], geo["mapping"], geo["control_points"], geo["in_spacing"],
                                    geo["out_spacing"], geo["affine_first"], None, None, None, "exact")
    desc = (_abi.ResampleImage * 1)()
    desc[0].in_, desc[0].out, desc[0].channels, desc[0].dtype, desc[0].interp = image.data_ptr(), grad.data_ptr(), 1, _abi.F32, _abi.LINEAR
    nbytes = int(hip._fn["resample3d_geometry_grad_workspace_bytes"](C.byref(geom)))
    workspace = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEVICE)
    results = []
    for _ in range(2):
        d_mapping = torch.full_like(keep[0], float("nan"))
        d_control = torch.full_like(keep[1], float("nan"))
        hip._call("resample3d_geometry_grad", image, C.byref(geom), 1, desc, C.c_void_p(d_mapping.data_ptr()), C.c_void_p(d_control.data_ptr()),
                  C.c_void_p(workspace.data_ptr()), nbytes, hip._stream(image))
        assert not bool(torch.isnan(d_mapping).any()) and not bool(torch.isnan(d_control).any())
        results.append((d_mapping.cpu(), d_control.cpu()))
    reference.check(case, *results[0])
    for first, second in zip(*results, strict=True):
        assert _same(first, second)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _forward(engine, case, mapping, control, images, **extra):
    geo = on_device(case["geo"], DEVICE)
    arguments = {**_launch_arguments(geo), "mapping": mapping, "control_points": control, **extra}
    return engine.resample3d(images, interps=["linear"] * len(images), fills=[None if f is None else f.to(DEVICE) for f in case["fills"]], **arguments)


@pytest.mark.parametrize("leaves", ["mapping", "control", "both", "both+image"])
def test_resample3d_with_geometry_leaves_gives_the_explicit_gradient(hip, leaves):
    case = reference.case("9-two-images")
    expected = _run_case(hip, case)
    mapping, control = case["geo"]["mapping"].to(DEVICE), case["geo"]["control_points"].to(DEVICE)
    if leaves != "control":
        mapping.requires_grad_(True)
    if leaves != "mapping":
        control.requires_grad_(True)
    images = [x.to(DEVICE) for x in case["images"]]
    if leaves == "both+image":
        images[1].requires_grad_(True)
    outputs = _forward(hip, case, mapping, control, images)
    assert all(out.requires_grad for out in outputs)
    loss = sum((out * g.to(DEVICE)).sum() for out, g in zip(outputs, case["grads"], strict=True))
    loss.backward()
    if leaves != "control":
        assert mapping.grad.dtype == torch.float32 and _same(mapping.grad, expected[0])
    else:
        assert mapping.grad is None
    if leaves != "mapping":
        assert _same(control.grad, expected[1])
    else:
        assert control.grad is None
    if leaves == "both+image":
        from adjoint_reference import adjoint  # noqa: PLC0415

        explicit = adjoint(hip, case["grads"][1].to(DEVICE), on_device(case["geo"], DEVICE), None)
        torch.testing.assert_close(images[1].grad, explicit, rtol=0, atol=1e-5 * float(explicit.abs().max()))
        assert images[0].grad is None


def test_a_host_float64_mapping_leaf_receives_a_float64_gradient_and_a_label_map_rides_along(hip):
    case = reference.case("1-batched")
    expected, _ = _run_case(hip, case, want_control_points=False)
    mapping = case["geo"]["mapping"].double().requires_grad_(True)  # on the host
    image = case["images"][0].to(DEVICE)
    labels = torch.randint(0, 4, image.shape, dtype=torch.int16, device=DEVICE)
    geo = on_device(case["geo"], DEVICE)
    out, moved = hip.resample3d([image, labels], interps=["linear", "nearest"], fills=[None, None],
                                **{**_launch_arguments(geo), "mapping": mapping})
    assert out.requires_grad and not moved.requires_grad and moved.dtype == torch.int16
    (out * case["grads"][0].to(DEVICE)).sum().backward()
    assert mapping.grad.dtype == torch.float64 and mapping.grad.device.type == "cpu"
    assert _same(mapping.grad, expected)


def test_a_tight_forward_gives_the_gradient_of_the_exact_one(hip):
    case = reference.case("1-batched")
    results = []
    for precision in ("exact", "tight"):
        mapping = case["geo"]["mapping"].to(DEVICE).requires_grad_(True)
        (out,) = _forward(hip, case, mapping, case["geo"]["control_points"].to(DEVICE), [case["images"][0].to(DEVICE)], precision=precision)
        (out * case["grads"][0].to(DEVICE)).sum().backward()
        results.append(mapping.grad)
    assert _same(*results)


def test_double_backward_is_refused_in_words(hip):
    case = reference.case("1-batched")
    mapping = case["geo"]["mapping"].to(DEVICE).requires_grad_(True)
    (out,) = _forward(hip, case, mapping, case["geo"]["control_points"].to(DEVICE), [case["images"][0].to(DEVICE)])
    with pytest.raises(ops.EngineError, match="double backward"):
        torch.autograd.grad((out * case["grads"][0].to(DEVICE)).sum(), mapping, create_graph=True)


def test_a_call_whose_geometry_needs_no_gradient_launches_what_it_launched_before(hip, monkeypatch):
    case = reference.case("1-batched")
    calls = []
    real = ops.Engine._call

    def logged(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(ops.Engine, "_call", logged)
    mapping, control = case["geo"]["mapping"].to(DEVICE), case["geo"]["control_points"].to(DEVICE)
    image = case["images"][0].to(DEVICE).requires_grad_(True)
    (out,) = _forward(hip, case, mapping, control, [image])
    (out * case["grads"][0].to(DEVICE)).sum().backward()
    assert calls == ["resample3d", "resample3d"]  # the forward and the images' adjoint: nothing new
    calls.clear()
    with torch.no_grad():  # a geometry that requires a gradient is plain data when nobody records
        (out,) = _forward(hip, case, mapping.clone().requires_grad_(True), control, [image.detach()])
    assert calls == ["resample3d"] and not out.requires_grad
    calls.clear()
    (out,) = _forward(hip, case, mapping.clone().requires_grad_(True), control, [image.detach()])
    out.sum().backward()
    assert calls == ["resample3d", "resample3d_geometry_grad"]


def test_the_custom_op_fills_the_geometry_slots_and_passes_opcheck(hip):
    import torchio_amd.torch_ops  # noqa: F401, PLC0415

    case = reference.case("5-out-of-bounds-fill")
    expected = _run_case(hip, case)
    geo = case["geo"]
    mapping, control = geo["mapping"].to(DEVICE).requires_grad_(True), geo["control_points"].to(DEVICE).requires_grad_(True)
    image, grad, fill = case["images"][0].to(DEVICE), case["grads"][0].to(DEVICE), case["fills"][0].to(DEVICE)
    arguments = ([1], mapping, control, list(geo["in_spacing"]), list(geo["out_spacing"]), list(geo["out_shape"]), geo["affine_first"], [fill])
    (out,) = torch.ops.tio_hip.resample3d([image], *arguments)
    (out * grad).sum().backward()
    assert _same(mapping.grad, expected[0]) and _same(control.grad, expected[1])
    d_mapping, d_control = torch.ops.tio_hip.resample3d_geometry_grad([image], [grad], mapping.detach(), control.detach(), *arguments[3:])
    assert _same(d_mapping, expected[0]) and _same(d_control, expected[1])
    torch.library.opcheck(torch.ops.tio_hip.resample3d, ([image.clone().requires_grad_(True)], *arguments))
    torch.library.opcheck(torch.ops.tio_hip.resample3d_geometry_grad, ([image], [grad], mapping.detach(), control.detach(), *arguments[3:]))
    torch.library.opcheck(torch.ops.tio_hip.resample3d_geometry_grad, ([image], [grad], mapping.detach(), None, *arguments[3:]))


def test_warp_recovers_a_translation_by_gradient_descent(hip):
    """Ten plain gradient steps from a 0.7-voxel translation error on a smooth 16^3 volume: the squared error falls at every step."""
    axes = [torch.arange(16, dtype=torch.float32) for _ in range(3)]
    i, j, k = torch.meshgrid(*axes, indexing="ij")
    volume = (torch.sin(0.4 * i + 0.3) * torch.cos(0.35 * j) + torch.sin(0.3 * k + 0.2 * j))[None, None].to(DEVICE)
    truth = torch.eye(3, 4, device=DEVICE)
    truth[:, 3] = torch.tensor([0.4, -0.4, 0.41])  # |error| = 0.7 voxels
    target = tio.warp(volume, truth)
    mapping = torch.eye(3, 4, device=DEVICE).requires_grad_(True)
    losses = []
    for _ in range(10):
        loss = ((tio.warp(volume, mapping) - target) ** 2).sum()
        (step,) = torch.autograd.grad(loss, mapping)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            mapping[:, 3] -= 1e-3 * step[:, 3]
    losses.append(float(((tio.warp(volume, mapping.detach()) - target) ** 2).sum()))
    assert all(later < earlier for earlier, later in zip(losses, losses[1:], strict=False)), losses
    assert losses[-1] < 0.5 * losses[0], losses
