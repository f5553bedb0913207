"""Host side of the parameter gradients of the intensity ops (``tio_bias_field_grad``, ``tio_gamma_grad``, ``tio_noise_grad``,
``tio_separable_conv3d_taps_grad``): the test reference against central finite differences of its own float64 forward on every
case the GPU tests use, the ABI as ``ctypes`` sees it, the argument checks, the taps of ``functional.blur`` against the transform's
bit for bit, the new ``functional`` names, and the oracle engine's refusal."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import param_grad_reference as reference
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.transforms.blur import _stacked_gaussian_taps


# ---------------------------------------------------------------------------------------------------------------------
# the reference against finite differences of its own forward
# ---------------------------------------------------------------------------------------------------------------------
def _finite_differences(loss, leaf: torch.Tensor, ref: torch.Tensor, a: torch.Tensor, seed: int, used=None) -> None:
    """Central differences of ``loss`` along 3 random directions and along up to 12 single components of ``leaf``, against
    ``<ref, direction>``; the step error is O(h^2) of a smooth function, the tolerance is relative to ``<A, |direction|>``."""
    g = torch.Generator().manual_seed(seed)
    leaf = leaf.detach().cpu().double()
    mask = torch.ones_like(leaf) if used is None else used.double()
    directions = [(torch.rand(leaf.shape, generator=g, dtype=torch.float64) - 0.5) * mask for _ in range(3)]
    candidates = torch.nonzero(mask.reshape(-1)).reshape(-1)
    for pick in candidates[torch.randperm(candidates.numel(), generator=g)[:12]]:
        single = torch.zeros(leaf.numel(), dtype=torch.float64)
        single[pick] = 1.0
        directions.append(single.reshape(leaf.shape))
    assert float(a.max()) > 0 and bool((a + 1e-300 >= ref.abs() * (1 - 1e-12)).all())  # A dominates the reference, component by component
    h = 1e-5
    for direction in directions:
        slope = (loss(leaf + h * direction) - loss(leaf - h * direction)) / (2 * h)
        expected = float((ref * direction).sum())
        scale = float((a * direction.abs()).sum())
        assert abs(float(slope) - expected) <= 1e-6 * scale + 1e-12, (float(slope), expected, scale)


@pytest.mark.parametrize("name", sorted(reference.BIAS_CASES))
def test_the_bias_reference_equals_finite_differences(name):
    case = reference.bias_case(name)
    x64, gy64 = reference._narrowed(case["x"]), case["gy"].double()
    _finite_differences(lambda c: reference.bias_loss(x64, gy64, c, case["divide"], case["skip"]), case["coarse"], case["ref"], case["a"], 1)
    if case["skip"] is not None:
        rows = case["skip"].bool()
        assert bool((case["ref"][rows] == 0).all()) and bool((case["ref"][~rows] != 0).any())


@pytest.mark.parametrize("name", sorted(reference.GAMMA_CASES))
def test_the_gamma_reference_equals_finite_differences(name):
    case = reference.gamma_case(name)
    x64, gy64 = case["x"].double(), case["gy"].double()
    _finite_differences(lambda e: reference.gamma_loss(x64, gy64, e), case["gamma"], case["ref"], case["a"], 2)


@pytest.mark.parametrize("name", sorted(reference.NOISE_CASES))
def test_the_noise_reference_equals_finite_differences(name):
    case = reference.noise_case(name)
    x64, gy64, z1 = case["x"].double(), case["gy"].double(), case["z1"].double()
    z2 = None if case["z2"] is None else case["z2"].double()
    mean64, std64 = case["mean"].double(), case["std"].double()
    if name == "rician-batched-zeros":  # |a| is not differentiable at the planted y == 0 voxels: the reference's rule there is "adds nothing"
        assert int(((x64 + mean64.reshape(-1, 1, 1, 1, 1) + std64.reshape(-1, 1, 1, 1, 1) * z1) ** 2 + (mean64.reshape(-1, 1, 1, 1, 1) + std64.reshape(-1, 1, 1, 1, 1) * z2) ** 2 == 0).sum()) == 3
        gy64 = gy64.clone()
        for site in ((0, 0, 0, 0, 0), (0, 0, 1, 2, 3), (0, 0, 3, 3, 7)):
            gy64[site] = 0.0
        (mean_ref, mean_a), (std_ref, std_a) = reference.noise(case["x"], gy64, case["mean"], case["std"], z1, z2, True, case["keep"])
        for got, expected in ((mean_ref, case["mean_ref"][0]), (std_ref, case["std_ref"][0])):
            torch.testing.assert_close(got, expected, rtol=1e-13, atol=1e-13)  # the planted voxels add nothing to the case's reference either
    else:
        (mean_ref, mean_a), (std_ref, std_a) = case["mean_ref"], case["std_ref"]
    _finite_differences(lambda m: reference.noise_loss(x64, gy64, m, std64, z1, z2, case["rician"], case["keep"]), case["mean"], mean_ref, mean_a, 3)
    _finite_differences(lambda s: reference.noise_loss(x64, gy64, mean64, s, z1, z2, case["rician"], case["keep"]), case["std"], std_ref, std_a, 4)
    if case["keep"] is not None and case["mean"].numel() > 1:
        gated = ~case["keep"].bool()
        assert bool((mean_ref[gated] == 0).all()) and bool((std_ref[gated] == 0).all()) and bool((std_ref[~gated] != 0).all())


@pytest.mark.parametrize("name", sorted(reference.TAPS_CASES))
def test_the_taps_reference_equals_finite_differences(name):
    case = reference.taps_case(name)
    x64, gy64 = reference._narrowed(case["x"]), case["gy"].double()
    used = torch.zeros_like(case["taps"], dtype=torch.bool)
    for axis, r in enumerate(case["radius"]):
        if r > 0:
            used[:, axis, : 2 * r + 1] = True
    if case["skip"] is not None and case["taps"].shape[0] > 1:
        used[case["skip"].bool()] = False
    assert bool((case["ref"][~used] == 0).all())  # beyond 2 r + 1, on inactive axes and in skipped rows: exactly zero
    _finite_differences(lambda w: reference.taps_loss(x64, gy64, w, case["radius"], case["skip"]), case["taps"], case["ref"], case["a"], 5, used)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_four_entry_points_and_the_library_exports_them():
    vp, i32, i64, f32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64
    i32x3 = C.POINTER(C.c_int32)
    expected = {
        "bias_field_grad_workspace_bytes": (i64, [i32, i32, i32x3]),
        "bias_field_grad": (C.c_int, [vp, vp, i32, i32, i32, i32x3, vp, i32x3, i32, vp, vp, vp, i64, vp]),
        "gamma_grad_workspace_bytes": (i64, [i32, i32]),
        "gamma_grad": (C.c_int, [vp, vp, i32, i32, i64, f32, vp, i32, vp, vp, i64, vp]),
        "noise_grad_workspace_bytes": (i64, [i32, i32]),
        "noise_grad": (C.c_int, [vp, vp, i32, i32, i64, f32, f32, vp, vp, i32, i32, vp, vp, u64, vp, vp, vp, vp, i64, vp]),
        "separable_conv3d_taps_grad_workspace_bytes": (i64, [i32, i32]),
        "separable_conv3d_taps_grad": (C.c_int, [vp, i32, vp, vp, i32, i32, i32x3, vp, i32, i32, i32x3, vp, vp, vp, i64, vp]),
    }
    for name, prototype in expected.items():
        assert _abi.HIP_ONLY_PROTOTYPES[name] == prototype, name
        assert name not in _abi.PROTOTYPES and name not in _abi.ORACLE_ENTRY_POINTS and "tio_" + name in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 18  # additive
    library, functions = _lib.load()
    for name in expected:
        assert hasattr(library, "tio_" + name) and name in functions


def test_the_library_checks_its_arguments_without_a_gpu():
    _, f = _lib.load()
    buffers = [C.create_string_buffer(1 << 14) for _ in range(8)]
    x, gy, par, out, ws, taps, scratch, out2 = [C.c_void_p((C.addressof(b) + 15) & ~15) for b in buffers]
    three = lambda *v: (C.c_int32 * 3)(*v)  # noqa: E731

    def refused(name, arguments, word, status=-1):
        assert f[name](*arguments) == status, (name, word, f["last_error"]())
        message = f["last_error"]()
        assert ("tio_" + name).encode() in message and word in message, message

    # bias
    assert f["bias_field_grad_workspace_bytes"](2, 3, three(4, 5, 6)) == 2 * 3 * 4 * 5 * 6 * 8
    assert f["bias_field_grad_workspace_bytes"](2, 0, three(4, 5, 6)) == 0 and f["bias_field_grad_workspace_bytes"](2, 1, None) == 0
    nbytes = 2 * 8 * 8
    bias = lambda **kw: [kw.get("x", x), kw.get("gy", gy), kw.get("dtype", _abi.F32), 2, 1, kw.get("shape", three(4, 4, 4)), par, kw.get("coarse_shape", three(2, 2, 2)), 0,  # noqa: E731
                         None, kw.get("out", out), kw.get("ws", ws), kw.get("nbytes", nbytes), None]
    refused("bias_field_grad", bias(x=None), b"null")
    refused("bias_field_grad", bias(gy=None), b"null")
    refused("bias_field_grad", bias(out=None), b"null")
    for unknown in (9, -1, 1000):
        refused("bias_field_grad", bias(dtype=unknown), b"dtype", -2)
    refused("bias_field_grad", bias(dtype=_abi.I16), b"dtype", -2)
    refused("bias_field_grad", bias(shape=three(4, 0, 4)), b"shape")
    refused("bias_field_grad", bias(coarse_shape=three(2, 2, 0)), b"shape")
    refused("bias_field_grad", bias(ws=None), b"workspace")
    refused("bias_field_grad", bias(nbytes=nbytes - 8), b"workspace")
    refused("bias_field_grad", bias(ws=C.c_void_p(ws.value + 4)), b"aligned")
    # gamma
    assert f["gamma_grad_workspace_bytes"](3, 1) == 3 * f["gamma_grad_workspace_bytes"](3, 0) > 0
    nbytes = f["gamma_grad_workspace_bytes"](2, 1)
    gamma = lambda **kw: [kw.get("x", x), kw.get("gy", gy), kw.get("dtype", _abi.F32), kw.get("batch", 2), kw.get("n", 16), 1.5, kw.get("gamma_dev", par), 1,  # noqa: E731
                          kw.get("out", out), kw.get("ws", ws), kw.get("nbytes", nbytes), None]
    refused("gamma_grad", gamma(x=None), b"null")
    refused("gamma_grad", gamma(out=None), b"d_gamma")
    refused("gamma_grad", gamma(gamma_dev=None), b"gamma_dev")
    refused("gamma_grad", gamma(n=-1), b"negative")
    for unknown in (9, -1, 1000):
        refused("gamma_grad", gamma(dtype=unknown), b"dtype", -2)
    refused("gamma_grad", gamma(dtype=_abi.U8), b"dtype", -2)
    refused("gamma_grad", gamma(nbytes=nbytes - 8), b"workspace")
    refused("gamma_grad", gamma(ws=C.c_void_p(ws.value + 4)), b"aligned")
    # noise
    nbytes = f["noise_grad_workspace_bytes"](2, 0)
    noise = lambda **kw: [kw.get("x", x), kw.get("gy", gy), kw.get("dtype", _abi.F32), 2, 16, 0.0, 1.0, kw.get("mean_dev", None), None, kw.get("batched", 0), kw.get("rician", 0),  # noqa: E731
                          kw.get("base1", None), None, 7, None, kw.get("d_mean", out), kw.get("d_std", out2), kw.get("ws", ws), kw.get("nbytes", nbytes), None]
    refused("noise_grad", noise(d_mean=None, d_std=None), b"neither")
    refused("noise_grad", noise(gy=None), b"gy")
    refused("noise_grad", noise(x=None, rician=1), b"rician")
    refused("noise_grad", noise(batched=1), b"params_batched")
    refused("noise_grad", noise(rician=1, base1=par), b"base2_dev")
    refused("noise_grad", noise(ws=None), b"workspace")
    for unknown in (9, -1, 1000, _abi.I16):
        refused("noise_grad", noise(dtype=unknown), b"dtype", -2)
    # taps
    nbytes = f["separable_conv3d_taps_grad_workspace_bytes"](2, 1)
    assert nbytes == 2 * f["separable_conv3d_taps_grad_workspace_bytes"](2, 0) > 0
    conv = lambda **kw: [kw.get("x", x), kw.get("dtype", _abi.F32), gy, kw.get("scratch", scratch), 2, 1, three(4, 4, 4), kw.get("taps", taps), 1, kw.get("stride", 5),  # noqa: E731
                         kw.get("radius", three(1, 2, 0)), None, kw.get("out", out), kw.get("ws", ws), kw.get("nbytes", nbytes), None]
    refused("separable_conv3d_taps_grad", conv(out=None), b"null")
    refused("separable_conv3d_taps_grad", conv(x=None), b"null")
    refused("separable_conv3d_taps_grad", conv(scratch=None), b"null")
    refused("separable_conv3d_taps_grad", conv(taps=None), b"null")
    refused("separable_conv3d_taps_grad", conv(radius=three(1, 3, 0)), b"tap_stride")
    refused("separable_conv3d_taps_grad", conv(radius=three(17, 0, 0), stride=35), b"exceeds")
    for unknown in (9, -1, 1000):
        refused("separable_conv3d_taps_grad", conv(dtype=unknown), b"dtype", -2)
    refused("separable_conv3d_taps_grad", conv(dtype=_abi.I32), b"dtype", -2)
    refused("separable_conv3d_taps_grad", conv(nbytes=nbytes - 8), b"workspace")
    del buffers


def test_the_fake_kernels_give_the_shapes_of_the_parameters():
    import torchio_amd.torch_ops  # noqa: F401, PLC0415
    from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: PLC0415

    with FakeTensorMode():
        x, g = torch.empty(2, 3, 6, 5, 8, device="cuda", dtype=torch.float16), torch.empty(2, 3, 6, 5, 8, device="cuda")
        d = torch.ops.tio_hip.bias_field_grad(x, g, torch.empty(2, 3, 4, 4, 2, device="cuda"), True, None)
        assert d.shape == (2, 3, 4, 4, 2) and d.dtype == torch.float32 and d.device.type == "cuda"
        assert torch.ops.tio_hip.gamma_grad(x, g, torch.empty(2, device="cuda")).shape == (2,)
        assert torch.ops.tio_hip.gamma_grad(x, g, torch.empty(1)).shape == (1,)
        d_mean, d_std = torch.ops.tio_hip.noise_grad(x, g, torch.empty(1), torch.empty(2, device="cuda"), True, None, None, 5, None)
        assert d_mean.shape == (1,) and d_std.shape == (2,) and d_std.dtype == torch.float32
        d = torch.ops.tio_hip.separable_conv3d_taps_grad(x, g, torch.empty(1, 3, 7, device="cuda"), [1, 2, 3], None)
        assert d.shape == (1, 3, 7) and d.dtype == torch.float32
        assert torch.ops.tio_hip.philox_normal_like(x, 3, 1).dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# functional
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    ("rows", "per_element"),
    [
        ([[1.2, 0.7, 2.5]], False),
        ([[1.2, 0.0, 2.5]], False),  # a sigma of 0 on one axis
        ([[5.3, 0.3, 1.0]], False),
        ([[1.2, 0.7, 2.5], [0.4, 1.9, 0.8]], True),  # every element blurs every axis: the one-chain form
        ([[1.2, 0.0, 2.5], [0.4, 1.9, 0.0], [0.9, 0.0, 1.1]], True),  # per axis, with zeros
        ([[1.2, 0.0, 2.5], [0.0, 0.0, 0.0]], True),  # a row that is skipped
    ],
)
def test_the_differentiable_taps_equal_the_transforms_bit_for_bit(rows, per_element):
    taps, radius, skip = _stacked_gaussian_taps(np.asarray(rows, dtype=np.float64), per_element=per_element)
    for dtype in (torch.float64, torch.float32):
        sigmas = torch.tensor(rows, dtype=dtype, requires_grad=True)
        exact = np.asarray(sigmas.detach().double().numpy())
        expected = (taps, radius, skip) if dtype == torch.float64 else _stacked_gaussian_taps(exact, per_element=per_element)
        mine, my_radius, my_skip = tio.functional._gaussian_taps(sigmas, per_element)
        assert mine.dtype == torch.float32 and mine.requires_grad and torch.equal(mine.detach(), expected[0])
        assert my_radius == list(expected[1]) and ((my_skip is None and expected[2] is None) or np.array_equal(my_skip, expected[2]))
        # (a weighting that is not linear along a row: the normalised, symmetric taps carry no gradient against a linear one)
        (mine * (torch.arange(mine.numel(), dtype=torch.float32) ** 2).reshape(mine.shape)).sum().backward()
        assert sigmas.grad.dtype == dtype and bool(torch.isfinite(sigmas.grad).all())
        active = torch.tensor(rows) > 0
        assert bool((sigmas.grad[~active] == 0).all()) and bool((sigmas.grad[active] != 0).all())


def test_the_sigma_chain_of_blur_equals_finite_differences_of_the_taps():
    sigmas = torch.tensor([[1.3, 0.8, 2.1]], dtype=torch.float64, requires_grad=True)
    weights = torch.randn(1, 3, 15, generator=torch.Generator().manual_seed(0)).double()
    taps, _, _ = tio.functional._gaussian_taps(sigmas, False)
    (taps.double() * weights).sum().backward()
    for axis in range(3):
        h = 1e-3
        step = torch.zeros(1, 3, dtype=torch.float64)
        step[0, axis] = h
        up, _, _ = tio.functional._gaussian_taps(sigmas.detach() + step, False)
        down, _, _ = tio.functional._gaussian_taps(sigmas.detach() - step, False)
        slope = float(((up.double() - down.double()) * weights).sum() / (2 * h))
        assert abs(slope - float(sigmas.grad[0, axis])) <= 2e-4 * max(1.0, abs(slope))  # float32 taps: 1e-7 / h


def test_the_functional_names_exist_and_validate_their_shapes():
    F = tio.functional
    assert list(inspect.signature(F.bias_field).parameters) == ["data", "coarse", "divide"]
    assert list(inspect.signature(F.gamma).parameters) == ["data", "gamma"]
    assert list(inspect.signature(F.noise).parameters) == ["data", "mean", "std", "seed", "draws", "rician"]
    assert list(inspect.signature(F.blur).parameters) == ["data", "sigma_vox"]
    assert inspect.signature(F.noise).parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    volume = torch.zeros(2, 1, 4, 4, 4)
    for call in (lambda: F.bias_field(volume[0], torch.zeros(2, 1, 2, 2, 2)), lambda: F.gamma(volume[0], 1.0),
                 lambda: F.noise(volume[0], 0.0, 1.0, seed=1), lambda: F.blur(volume[0], [1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match=r"\(B, C, I, J, K\)"):
            call()
    with pytest.raises(ValueError, match="coarse"):
        F.bias_field(volume, torch.zeros(3, 1, 2, 2, 2))
    with pytest.raises(ValueError, match="coarse"):
        F.bias_field(volume, torch.zeros(2, 2))
    with pytest.raises(ValueError, match="gamma must hold 1 or 2"):
        F.gamma(volume, torch.ones(3))
    with pytest.raises(ValueError, match="std must hold 1 or 2"):
        F.noise(volume, 0.0, torch.ones(5), seed=1)
    with pytest.raises(ValueError, match="either"):
        F.noise(volume, 0.0, 1.0)
    with pytest.raises(ValueError, match="either"):
        F.noise(volume, 0.0, 1.0, seed=1, draws=torch.zeros_like(volume))
    with pytest.raises(ValueError, match="two tensors"):
        F.noise(volume, 0.0, 1.0, draws=torch.zeros_like(volume), rician=True)
    with pytest.raises(ValueError, match="shaped like"):
        F.noise(volume, 0.0, 1.0, draws=torch.zeros(2, 1, 4, 4, 5))
    with pytest.raises(ValueError, match="sigma_vox"):
        F.blur(volume, torch.ones(3, 3))
    with pytest.raises(ValueError, match="sigma_vox"):
        F.blur(volume, [1.0, 2.0])
    assert F.blur(volume, [0.0, 0.0, 0.0]) is volume  # every sigma <= 0: the identity, as the transform


# ---------------------------------------------------------------------------------------------------------------------
# the oracle engine has no such kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_the_oracle_engine_refuses_parameters_that_require_a_gradient(oracle):
    data = torch.rand(2, 1, 4, 4, 4) + 0.5
    leaf = lambda *shape: torch.rand(*shape).requires_grad_(True)  # noqa: E731
    calls = {
        "tio_bias_field_grad": lambda: oracle.bias_field_apply(data, leaf(2, 1, 2, 2, 2)),
        "tio_gamma_grad": lambda: oracle.gamma_pow(data, leaf(2)),
        "tio_noise_grad": lambda: oracle.add_noise(data, 0.0, leaf(1), base1=torch.randn(data.shape)),
        "tio_separable_conv3d_taps_grad": lambda: oracle.separable_conv3d(data, leaf(1, 3, 3), [1, 1, 1]),
    }
    for kernel, call in calls.items():
        with pytest.raises(NotImplementedError, match=f"requires a gradient.*oracle engine has no {kernel}"):
            call()
    with torch.no_grad():  # without autograd a tensor that requires a gradient is just data
        out = oracle.gamma_pow(data, leaf(2))
    assert out.shape == data.shape and not out.requires_grad
    assert oracle.bias_field_apply(data, torch.zeros(2, 1, 2, 2, 2)).shape == data.shape  # plain parameters run as before
