"""The backward passes of Ghosting and Motion, which need no kernel of their own: both operators are symmetric matrices
(DESIGN.md 4.23), so ``ghost_lines`` and ``kspace_segment_mix`` applied to the incoming gradient ARE the gradients.

GPU: the gradient of ``<op(x), g>`` against float64 autograd through the FFT formulation - for Ghosting the route of
``kspace_artefact_cases.ghost_fft`` (restated with ``torch.fft`` so that autograd can follow it, and held to the numpy original
first), for Motion the reference's own sequence (rigid ``affine_grid`` / ``grid_sample`` moves, ``fftn``, slabs of planes along the
first axis, ``ifftn``, as ``test_kspace_segment_mix_matches_the_fft_route`` restates the compositing).  Bar: ``1e-5 max|expected|``,
the project's bar for these operators' forwards - the backward is the same operator applied to ``g``.
Host: ``tio_kspace_mix_table``'s blocks equal their transposes bit for bit; the inversion of the axis tables against a loop.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import interpolate_adjoint_reference as ref
import kspace_artefact_cases as kc
from parity_harness import use_engine
from torchio_amd import _lib
from torchio_amd import ops
from torchio_amd.transforms import motion

DEVICE = "cuda"


# ---------------------------------------------------------------------------------------------------------------------
# Ghosting
# ---------------------------------------------------------------------------------------------------------------------
def _ghost64(x: torch.Tensor, axes, masks) -> torch.Tensor:
    """``kspace_artefact_cases.ghost_fft`` with ``torch.fft`` on a float64 tensor (differentiable)."""
    out = []
    for b, (axis, mask) in enumerate(zip(axes, masks, strict=True)):
        if mask is None:
            out.append(x[b])
            continue
        spectrum = torch.fft.fftshift(torch.fft.fftn(x[b], dim=(-3, -2, -1)), dim=(-3, -2, -1))
        view = [1, 1, 1, 1]
        view[axis + 1] = -1
        spectrum = spectrum * torch.as_tensor(np.asarray(mask, dtype=np.float64), device=x.device).reshape(view)
        out.append(torch.fft.ifftn(torch.fft.ifftshift(spectrum, dim=(-3, -2, -1)), dim=(-3, -2, -1)).real)
    return torch.stack(out)


GHOST_SHAPE = (2, 2, 12, 9, 10)
GHOST_CASES = {  # axes, strengths, frequency lists (UNSHIFTED), active
    "axis0": ([0, 0], [0.7, 0.7], [[0, 3, 6, 9]] * 2, None),
    "axis1": ([1, 1], [0.4, 0.4], [[1, 4, 7]] * 2, None),
    "axis2": ([2, 2], [1.2, 1.2], [[0, 5]] * 2, None),
    "inactive-element": ([0, 0], [0.7, 0.7], [[0, 3, 6, 9]] * 2, [1, 0]),
    "per-element-axes": ([2, 1], [0.5, 0.9], [[2, 4, 6, 8], [0, 3, 6]], None),
    "nine-planes": ([0, 0], [0.6, 0.6], [[0, 1, 2, 3, 5, 7, 8, 10, 11]] * 2, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GHOST_CASES))
def test_ghost_lines_backward_against_float64_autograd(hip, name):
    axes, strengths, lists, active = GHOST_CASES[name]
    data = kc.signed_image(GHOST_SHAPE)
    masks = [None if active is not None and not active[b] else kc.mask_from_frequencies(GHOST_SHAPE[2 + axes[b]], lists[b], strengths[b])
             for b in range(GHOST_SHAPE[0])]
    # the differentiable restatement is the imported FFT route
    assert np.abs(_ghost64(data.double(), axes, masks).numpy() - kc.ghost_fft(data, axes, masks)).max() <= 1e-9
    grad = ref.randn(GHOST_SHAPE, 43)
    leaf64 = data.double().to(DEVICE).requires_grad_(True)
    (expected,) = torch.autograd.grad(_ghost64(leaf64, axes, masks), leaf64, grad.double().to(DEVICE))
    flags = None if active is None else torch.tensor(active, dtype=torch.uint8, device=DEVICE)
    leaf = data.to(DEVICE).requires_grad_(True)
    out = hip.ghost_lines(leaf, axes, strengths, lists, flags)
    assert torch.equal(out.detach(), hip.ghost_lines(leaf.detach(), axes, strengths, lists, flags))
    out.backward(grad.to(DEVICE))
    worst = float((leaf.grad.double() - expected).abs().max())
    print(f"[ghost backward] {name}: max|d| = {worst:.3e}, bar = {kc.FLOAT_BAR * float(expected.abs().max()):.3e}")
    assert worst <= kc.FLOAT_BAR * float(expected.abs().max())
    if active is not None:
        assert torch.equal(leaf.grad[1], grad[1].to(DEVICE)), "an inactive element is a copy both ways"


# ---------------------------------------------------------------------------------------------------------------------
# Motion
# ---------------------------------------------------------------------------------------------------------------------
def _motion64(x: torch.Tensor, transforms: list[dict]) -> torch.Tensor:
    """The reference's ``_apply_motion_segments`` for ONE element list, float64 throughout: ``x`` is ``(B, C, I, J, K)``."""
    batch, channels, *shape = x.shape
    bounds = motion._segment_bounds(len(transforms) + 1, shape[0])
    spectrum = torch.fft.fftn(x, dim=(-3, -2, -1))
    planes = torch.arange(shape[0], device=x.device).view(1, 1, -1, 1, 1)
    for index, transform in enumerate(transforms, start=1):
        degrees = torch.tensor([transform["degrees"]] * batch, dtype=torch.float32)
        translation = torch.tensor([transform["translation"]] * batch, dtype=torch.float32)
        theta = torch.cat([motion._rotation_matrices(degrees), (translation / (torch.tensor(shape, dtype=torch.float32) / 2))[:, :, None]], dim=2)
        grid = F.affine_grid(theta.double().to(x.device), [batch, 1, *shape], align_corners=True)
        moved = F.grid_sample(x.reshape(batch * channels, 1, *shape), grid.repeat_interleave(channels, dim=0), mode="bilinear",
                              padding_mode="zeros", align_corners=True).reshape(x.shape)
        inside = (planes >= bounds[index]) & (planes < bounds[index + 1])
        spectrum = torch.where(inside, torch.fft.fftn(moved, dim=(-3, -2, -1)), spectrum)
    return torch.fft.ifftn(spectrum, dim=(-3, -2, -1)).real


MOTION_TRANSFORMS = [{"degrees": (4.0, -7.0, 5.5), "translation": (1.5, -2.0, 0.75)}, {"degrees": (-6.0, 3.0, 8.0), "translation": (-1.0, 2.5, -1.25)}]


@pytest.mark.gpu
def test_motion_backward_against_float64_autograd(hip):
    shape = (2, 1, 12, 10, 8)
    data, grad = kc.signed_image(shape), ref.randn(shape, 47)
    leaf64 = data[:1].double().to(DEVICE).requires_grad_(True)
    (expected,) = torch.autograd.grad(_motion64(leaf64, MOTION_TRANSFORMS), leaf64, grad[:1].double().to(DEVICE))
    leaf = data.to(DEVICE).requires_grad_(True)
    with use_engine(hip):
        out = motion._apply_motion_per_instance(leaf, [MOTION_TRANSFORMS, []])  # element 1 is gated out
        with torch.no_grad():
            plain = motion._apply_motion_per_instance(leaf, [MOTION_TRANSFORMS, []])
    assert torch.equal(out.detach(), plain) and torch.equal(plain[1], data[1].to(DEVICE))
    forward64 = _motion64(data[:1].double().to(DEVICE), MOTION_TRANSFORMS)
    assert float((plain[:1].double() - forward64).abs().max()) <= kc.FLOAT_BAR * float(forward64.abs().max())  # the restatement is Motion
    out.backward(grad.to(DEVICE))
    worst = float((leaf.grad[:1].double() - expected).abs().max())
    print(f"[motion backward] max|d| = {worst:.3e}, bar = {kc.FLOAT_BAR * float(expected.abs().max()):.3e}")
    assert worst <= kc.FLOAT_BAR * float(expected.abs().max())
    assert torch.equal(leaf.grad[1], grad[1].to(DEVICE)), "the gated-out element's gradient is the incoming one, exactly"


@pytest.mark.gpu
def test_shared_motion_and_other_leaf_dtypes(hip):
    """The shared road (no inactive rows) on a float16 leaf: the still image is ``data.float()`` and the incoming gradient is
    taken to float32, so the float16 leaf receives the float32 road's gradient of the same values, rounded once."""
    shape = (2, 1, 12, 10, 8)
    data16 = (kc.signed_image(shape) / 64).to(DEVICE).half()
    leaf, leaf16 = data16.float().requires_grad_(True), data16.clone().requires_grad_(True)
    grad16 = ref.randn(shape, 53).to(DEVICE).half()
    with use_engine(hip):
        motion._apply_motion(leaf, MOTION_TRANSFORMS).backward(grad16.float())
        out16 = motion._apply_motion(leaf16, MOTION_TRANSFORMS)
        out16.backward(grad16)
    assert out16.dtype == torch.float16 and leaf16.grad.dtype == torch.float16
    # one float16 rounding of the float32 value (2^-11 relative); the 2^-20 term covers the order in which autograd adds the
    # three float32 contributions of a leaf (a few 2^-24 of their magnitudes) and float16's subnormal step
    scale = float(leaf.grad.abs().max())
    assert scale > 0
    assert bool(((leaf16.grad.float() - leaf.grad).abs() <= 2.0**-11 * leaf.grad.abs() + 2.0**-20 * scale).all())


@pytest.mark.gpu
def test_ghosting_and_motion_without_a_gradient_launch_what_they_launched_before(hip, monkeypatch):
    calls = []
    real = ops.Engine._call

    def logged(self, name, *args):
        calls.append(name)
        return real(self, name, *args)

    monkeypatch.setattr(ops.Engine, "_call", logged)
    data = kc.signed_image(GHOST_SHAPE).to(DEVICE)
    axes, strengths, lists, _ = GHOST_CASES["per-element-axes"]
    segments = [data, data.flip(2).contiguous(), data.roll(1, 3).contiguous()]
    bounds = [0, 4, 8, 12]
    runs = {
        "kspace_ghost_lines": lambda x: hip.ghost_lines(x, axes, strengths, lists),
        "kspace_segment_mix": lambda x: hip.kspace_segment_mix([x, *segments[1:]], bounds, torch.float32),
    }
    for name, run in runs.items():
        calls.clear()
        plain = run(data)
        assert calls == [name] and not plain.requires_grad
        calls.clear()
        with torch.no_grad():
            silent = run(data.clone().requires_grad_(True))
        assert calls == [name] and not silent.requires_grad and torch.equal(silent, plain)
        calls.clear()
        recorded = run(data.clone().requires_grad_(True))
        recorded.sum().backward()
        assert calls == [name, name] and torch.equal(recorded.detach(), plain)  # the same kernel on the gradient: no new launch kind


@pytest.mark.gpu
def test_segment_mix_backward_is_the_transpose_per_segment(hip):
    """Every segment as a leaf: ``<mix(x_0, x_1, x_2), g> = sum_s <x_s, dL/dx_s>`` (the mix is linear), in float64 sums."""
    shape = (2, 2, 12, 9, 7)
    segments = [ref.randn(shape, 60 + s).to(DEVICE).requires_grad_(True) for s in range(3)]
    grad = ref.randn(shape, 59).to(DEVICE)
    active = torch.tensor([1, 0], dtype=torch.uint8, device=DEVICE)
    out = hip.kspace_segment_mix(segments, [0, 4, 8, 12], torch.float32, active=active)
    out.backward(grad)
    lhs = float((out.detach()[:1].double() * grad[:1].double()).sum())
    rhs = float(sum((s.detach()[:1].double() * s.grad[:1].double()).sum() for s in segments))
    scale = float(sum((s.detach()[:1].double().abs() * s.grad[:1].double().abs()).sum() for s in segments))
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)
    for s in segments:
        assert not bool(s.grad[1].any()), "the rows of an inactive element take no part in the mix"


# ---------------------------------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("length", "bounds"), [(12, [0, 4, 8, 12]), (7, [0, 2, 4, 7]), (33, [0, 11, 22, 33]), (5, [0, 5]), (6, [0, 0, 6])])
def test_every_block_of_the_mix_table_equals_its_transpose_bit_for_bit(length, bounds):
    _, functions = _lib.load()
    table = torch.empty(len(bounds) - 1, length, length, dtype=torch.float32)
    status = functions["kspace_mix_table"](length, len(bounds) - 1, (C.c_int32 * len(bounds))(*bounds), C.c_void_p(table.data_ptr()))
    assert status == 0
    assert torch.equal(table, table.transpose(1, 2)), "W[s][i'][i] depends on i - i' through a cosine: symmetric"


@pytest.mark.parametrize("nearest", [False, True])
def test_the_inverted_axis_tables_against_a_loop(nearest):
    g = torch.Generator().manual_seed(71)
    batch, length = 4, 9
    lower = torch.randint(0, length, (batch, length), generator=g)
    lower[1] = torch.arange(length)
    lower[2] = 3  # one source read by every output, the others unused
    upper = None if nearest else torch.randint(0, length, (batch, length), generator=g)
    weight = None if nearest else torch.rand(batch, length, generator=g)
    offsets, positions, weights = ops.Engine.axis_gather_lists(lower.to(torch.int32), None if nearest else upper.to(torch.int32), weight)
    assert offsets.dtype == torch.int32 and positions.dtype == torch.int32 and offsets.shape == (batch, length + 1)
    assert (weights is None) == nearest and positions.shape == (batch, length if nearest else 2 * length)
    expected = ref.brute_force_lists(lower, upper, weight)
    for b in range(batch):
        assert int(offsets[b, 0]) == 0 and int(offsets[b, -1]) == positions.shape[1]
        for p in range(length):
            begin, end = int(offsets[b, p]), int(offsets[b, p + 1])
            got = [(int(positions[b, e]), 1.0 if nearest else float(weights[b, e])) for e in range(begin, end)]
            assert got == expected[b][p], (b, p)
