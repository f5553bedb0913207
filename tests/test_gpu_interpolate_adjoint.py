"""GPU: the gather adjoints of ``interpolate_adjoint.hip`` - ``Engine.interpolate3d_adjoint``, ``axis_gather_lerp_adjoint`` and
``pad3d_adjoint`` - and the backward passes they give ``interpolate3d`` / ``axis_gather_lerp`` / ``pad3d``.

1. the exact transpose at the smallest shapes that can go wrong, against ``A^T g`` with ``A`` the forward's own matrix
   (``interpolate_adjoint_reference.dense_matrix``), ``(N_v + 6) u S_v`` (``(N_v + 1) u S_v`` for padding), two runs bit-identical;
2. float64 autograd through ``F.interpolate`` / ``F.pad`` at launch sizes, one case beyond one sweep of the streaming launcher;
3. the plumbing: leaves of every float dtype, the calls without a gradient launch what they launched before.

Every run prints the worst ``error / bound`` per case (``-s``).  Seen on the MI355X: against the dense matrix 0.13 (interpolate3d, both
modes; 0 where every column holds one entry), 0.22 (axis_gather_lerp), 0.46 (pad3d); against float64 autograd 0.24 (trilinear), 0.38
(nearest), 0.47 (pad3d), 0.22 (axis_gather_lerp at 129^3).
"""
from __future__ import annotations

import pytest
import torch

import interpolate_adjoint_reference as ref
from torchio_amd import ops
from torchio_amd.transforms import anisotropy

pytestmark = pytest.mark.gpu
DEVICE = "cuda"

INTERPOLATE_SHAPES = [((3, 4, 5), (5, 4, 2)), ((1, 6, 2), (4, 1, 7)), ((7, 5, 3), (2, 9, 3)), ((4, 4, 4), (4, 4, 4)), ((2, 3, 1), (1, 1, 1))]


def _twice(run):
    first, second = run(), run()
    assert torch.equal(first, second), "two runs of a gather adjoint differ"
    assert first.dtype == torch.float32
    return first


# ---------------------------------------------------------------------------------------------------------------------
# 1. the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize(("in_shape", "out_shape"), INTERPOLATE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_interpolate3d_adjoint_is_the_transpose_of_the_forward(hip, in_shape, out_shape, mode):
    matrix = ref.dense_matrix(lambda x: hip.interpolate3d(x, out_shape, mode), in_shape, device=DEVICE)
    grad = ref.randn((2, 2, *out_shape), 3).to(DEVICE)
    result = _twice(lambda: hip.interpolate3d_adjoint(grad, in_shape, mode))
    assert result.shape == (2, 2, *in_shape)
    ref.check_against_dense(matrix, grad, result, 6, f"interpolate3d {mode} {in_shape} -> {out_shape}")


def _axis_tables(length: int, mode: str, kind: str):
    """(lower, upper, weight, active) for a batch of 3 along an axis of *length*."""
    if kind == "monotone":  # the transform's own tables, a different factor per element; element 1 is inactive (a copy)
        down_sizes = torch.round(length / torch.tensor([2.5, 1.0, 1.7], dtype=torch.float64)).clamp_min(1).to(torch.long)
        active = torch.tensor([True, False, True])
        if mode == "nearest":
            return anisotropy._nearest_source_indices(length, down_sizes), None, None, active
        return (*anisotropy._linear_source_indices(length, down_sizes), active)
    # hand-made and NOT monotone: repeated sources, unused sources, lower == upper, lower > upper
    g = torch.Generator().manual_seed(length)
    lower = torch.randint(0, length, (3, length), generator=g)
    lower[0] = length - 1 - torch.arange(length)  # a reversal
    lower[2] = lower[2].clamp(max=max(length - 3, 0))  # the last sources of element 2 are never read through `lower`
    if mode == "nearest":
        return lower, None, None, None
    upper = torch.randint(0, length, (3, length), generator=g)
    upper[1, : length // 2] = lower[1, : length // 2]
    return lower, upper, torch.rand(3, length, generator=g), None


@pytest.mark.parametrize("kind", ["monotone", "hand-made"])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_gather_lerp_adjoint_is_the_transpose_of_the_forward(hip, axis, mode, kind):
    shape = (5, 6, 7)
    lower, upper, weight, active = _axis_tables(shape[axis], mode, kind)
    matrix = ref.dense_matrix(lambda x: hip.axis_gather_lerp(x, axis, lower, upper, weight, active), shape, batch=3, device=DEVICE)
    grad = ref.randn((3, 2, *shape), 5).to(DEVICE)
    result = _twice(lambda: hip.axis_gather_lerp_adjoint(grad, axis, lower, upper, weight, active))
    ref.check_against_dense(matrix, grad, result, 6, f"axis_gather_lerp {mode} {kind} axis {axis}")
    if active is not None:
        assert torch.equal(result[1], grad[1]), "an inactive element is a copy both ways"


PAD_SHAPE = (3, 4, 2)
PAD_LARGEST = {"reflect": lambda n: n - 1, "circular": lambda n: n, "replicate": lambda n: 2 * n + 1}  # replicate has no limit


def _pad_cases():
    for mode in ("reflect", "replicate", "circular"):
        yield mode, (2, 1, 0, 3, 1, 1)
        for axis in range(3):  # the largest the mode allows on one axis, zero elsewhere
            largest = PAD_LARGEST[mode](PAD_SHAPE[axis])
            padding = [0] * 6
            padding[2 * axis] = padding[2 * axis + 1] = largest
            yield mode, tuple(padding)


@pytest.mark.parametrize(("mode", "padding"), list(_pad_cases()), ids=lambda v: v if isinstance(v, str) else "-".join(str(p) for p in v))
def test_pad3d_adjoint_is_the_transpose_of_the_forward(hip, mode, padding):
    matrix = ref.dense_matrix(lambda x: hip.pad3d(x, padding, mode), PAD_SHAPE, device=DEVICE)
    out_shape = [PAD_SHAPE[d] + padding[2 * d] + padding[2 * d + 1] for d in range(3)]
    grad = ref.randn((2, 2, *out_shape), 7).to(DEVICE)
    result = _twice(lambda: hip.pad3d_adjoint(grad, PAD_SHAPE, padding, mode))
    ref.check_against_dense(matrix, grad, result, 1, f"pad3d {mode} {padding}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. float64 autograd at launch sizes
# ---------------------------------------------------------------------------------------------------------------------
LAUNCH_SHAPES = [((2, 1), (33, 20, 47), (17, 40, 50)), ((1, 1), (129, 129, 129), (64, 64, 64))]  # the second: > 256 * 32 * 256 results


@pytest.mark.parametrize(("bc", "in_shape", "out_shape"), LAUNCH_SHAPES, ids=["33x20x47", "129-two-sweeps"])
def test_interpolate3d_linear_adjoint_against_float64_autograd(hip, bc, in_shape, out_shape):
    grad = ref.randn((*bc, *out_shape), 11).to(DEVICE)
    result = hip.interpolate3d_adjoint(grad, in_shape, "linear")
    ref.assert_within(result, ref.interpolate_reference(grad, in_shape, "linear"), ref.linear_bound(grad, in_shape), f"linear {in_shape} <- {out_shape}")


@pytest.mark.parametrize(("bc", "in_shape", "out_shape"), LAUNCH_SHAPES, ids=["33x20x47", "129-two-sweeps"])
def test_interpolate3d_nearest_adjoint_against_float64_autograd(hip, bc, in_shape, out_shape):
    for n_in, n_out in zip(in_shape, out_shape, strict=True):  # a source index that falls differently would be a whole contribution
        index32, index64 = ref.nearest_tables(n_in, n_out)
        assert torch.equal(index32, index64), (n_in, n_out)
    grad = ref.randn((*bc, *out_shape), 13).to(DEVICE)
    result = hip.interpolate3d_adjoint(grad, in_shape, "nearest")
    bound = ref.exact_weight_bound(lambda g: ref.interpolate_reference(g, in_shape, "nearest"), grad)
    ref.assert_within(result, ref.interpolate_reference(grad, in_shape, "nearest"), bound, f"nearest {in_shape} <- {out_shape}")


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
@pytest.mark.parametrize(("bc", "in_shape", "padding"), [((2, 1), (33, 20, 47), (5, 3, 0, 7, 4, 6)), ((1, 1), (129, 129, 129), (1, 2, 3, 0, 2, 1))],
                         ids=["33x20x47", "129-two-sweeps"])
def test_pad3d_adjoint_against_float64_autograd(hip, bc, in_shape, padding, mode):
    out_shape = [in_shape[d] + padding[2 * d] + padding[2 * d + 1] for d in range(3)]
    grad = ref.randn((*bc, *out_shape), 17).to(DEVICE)
    result = hip.pad3d_adjoint(grad, in_shape, padding, mode)
    bound = ref.exact_weight_bound(lambda g: ref.pad_reference(g, in_shape, padding, mode), grad)
    ref.assert_within(result, ref.pad_reference(grad, in_shape, padding, mode), bound, f"pad3d {mode} {in_shape} + {padding}")


def test_axis_gather_lerp_adjoint_beyond_one_sweep(hip):
    """129^3 results: the grid-stride loop takes a second trip.  Reference: float64 autograd through ``gather`` with the tables'
    own float32 weights widened; ``(N_v + 6) u G_v`` (``1 - w`` is rounded in float32 by the engine, exact in the reference: one
    more ``u`` per weight than against the dense matrix, inside the same slack)."""
    shape, axis = (129, 129, 129), 2
    lower, upper, weight = anisotropy._linear_source_indices(shape[axis], torch.tensor([52]))
    grad = ref.randn((1, 1, *shape), 19).to(DEVICE)
    result = hip.axis_gather_lerp_adjoint(grad, axis, lower, upper, weight)
    lo, hi, w = (t.to(DEVICE).view(1, 1, 1, 1, -1).expand(1, 1, *shape) for t in (lower, upper, weight.double()))

    def forward64(x, taken_as_one=False):
        low, high = x.gather(4, lo), x.gather(4, hi)
        return low + high if taken_as_one else low * (1.0 - w) + high * w

    reference = ref._autograd64(forward64, shape, grad)
    counts = ref._autograd64(lambda x: forward64(x, True), shape, torch.ones_like(grad))
    sums = ref._autograd64(lambda x: forward64(x, True), shape, grad.abs())
    ref.assert_within(result, reference, (counts + 6) * ref.U * sums, "axis_gather_lerp 129^3")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _calls_with_backward(hip):
    """name -> (call(data) -> result, explicit(grad) -> float32 dL/d data) on a (3, 1, 6, 5, 7) batch."""
    lower, upper, weight, active = _axis_tables(5, "linear", "monotone")
    return {
        "interpolate3d-linear": (lambda x: hip.interpolate3d(x, (4, 7, 9), "linear"), lambda g: hip.interpolate3d_adjoint(g, (6, 5, 7), "linear")),
        "interpolate3d-nearest": (lambda x: hip.interpolate3d(x, (4, 7, 9), "nearest"), lambda g: hip.interpolate3d_adjoint(g, (6, 5, 7), "nearest")),
        "axis_gather_lerp": (lambda x: hip.axis_gather_lerp(x, 1, lower, upper, weight, active),
                             lambda g: hip.axis_gather_lerp_adjoint(g, 1, lower, upper, weight, active)),
        "pad3d-reflect": (lambda x: hip.pad3d(x, (2, 1, 0, 3, 1, 1), "reflect"), lambda g: hip.pad3d_adjoint(g, (6, 5, 7), (2, 1, 0, 3, 1, 1), "reflect")),
        "pad3d-replicate": (lambda x: hip.pad3d(x, (2, 1, 0, 3, 1, 1), "replicate"), lambda g: hip.pad3d_adjoint(g, (6, 5, 7), (2, 1, 0, 3, 1, 1), "replicate")),
        "pad3d-circular": (lambda x: hip.pad3d(x, (2, 1, 0, 3, 1, 1), "circular"), lambda g: hip.pad3d_adjoint(g, (6, 5, 7), (2, 1, 0, 3, 1, 1), "circular")),
    }


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("name", ["interpolate3d-linear", "interpolate3d-nearest", "axis_gather_lerp", "pad3d-reflect", "pad3d-replicate", "pad3d-circular"])
def test_a_leaf_of_every_float_dtype_receives_the_explicit_launch(hip, name, dtype):
    call, explicit = _calls_with_backward(hip)[name]
    leaf = ref.randn((3, 1, 6, 5, 7), 23).to(device=DEVICE, dtype=dtype).requires_grad_(True)
    out = call(leaf)
    assert out.requires_grad and out.dtype == dtype and torch.equal(out.detach(), call(leaf.detach()))
    grad = ref.randn(out.shape, 29).to(device=DEVICE, dtype=dtype)
    out.backward(grad)
    assert leaf.grad.dtype == dtype and torch.equal(leaf.grad, explicit(grad).to(dtype))


def test_calls_without_a_gradient_launch_what_they_launched_before(hip, monkeypatch):
    calls = []
    real = ops.Engine._call

    def logged(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(ops.Engine, "_call", logged)
    expected = {"interpolate3d-linear": "interpolate3d", "interpolate3d-nearest": "interpolate3d", "axis_gather_lerp": "axis_gather_lerp",
                "pad3d-reflect": "pad3d", "pad3d-replicate": "pad3d", "pad3d-circular": "pad3d"}
    data = ref.randn((3, 1, 6, 5, 7), 31).to(DEVICE)
    for name, (call, _) in _calls_with_backward(hip).items():
        calls.clear()
        plain = call(data)
        assert calls == [expected[name]] and not plain.requires_grad, name
        calls.clear()
        with torch.no_grad():  # a tensor that requires a gradient is plain data when nobody records
            silent = call(data.clone().requires_grad_(True))
        assert calls == [expected[name]] and not silent.requires_grad and torch.equal(silent, plain), name
        calls.clear()
        recorded = call(data.clone().requires_grad_(True))
        recorded.sum().backward()
        assert calls == [expected[name], expected[name] + "_adjoint"] and torch.equal(recorded.detach(), plain), name


def test_refusals(hip, oracle):
    grad = torch.zeros(1, 1, 4, 4, 4, device=DEVICE)
    with pytest.raises(ValueError, match="mode"):
        hip.interpolate3d_adjoint(grad, (4, 4, 4), "cubic")
    with pytest.raises(ValueError, match="mode"):
        hip.pad3d_adjoint(grad, (2, 2, 2), (1, 1, 1, 1, 1, 1), "constant")
    with pytest.raises(ValueError, match="padded by"):
        hip.pad3d_adjoint(grad, (2, 2, 2), (1, 1, 1, 1, 1, 0), "reflect")
    with pytest.raises(ops.EngineError, match="reflect padding must be smaller"):
        hip.pad3d_adjoint(torch.zeros(1, 1, 5, 1, 1, device=DEVICE), (1, 1, 1), (2, 2, 0, 0, 0, 0), "reflect")
    with pytest.raises(ops.EngineError, match="fill values take no part"):
        hip.pad3d(grad, (1, 1, 1, 1, 1, 1), "reflect", fill_per_element=torch.zeros(1, device=DEVICE, requires_grad=True))
    for call in (lambda x: oracle.interpolate3d(x, (3, 3, 3), "linear"), lambda x: oracle.pad3d(x, (1, 1, 1, 1, 1, 1), "reflect"),
                 lambda x: oracle.axis_gather_lerp(x, 0, torch.zeros(1, 4, dtype=torch.long))):
        with pytest.raises(NotImplementedError, match="exist on the HIP engine only"):
            call(torch.zeros(1, 1, 4, 4, 4, requires_grad=True))
