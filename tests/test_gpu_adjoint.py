"""The trilinear adjoint scatter (``TIO_LINEAR_ADJOINT``), the autograd glue of ``Engine.resample3d`` and
``torch.ops.tio_hip.resample3d_adjoint``, per voxel, against references of the same operation (tests/adjoint_reference.py).

1. ``DENSE_CASES``: at <= ~400 input voxels the forward of the one-hot volumes is the matrix ``A`` in the float32 weights the
   kernels use; the adjoint must be ``A^T g`` up to the order of its additions: ``|acc_v - ref_v| <= (N_v + 1) u S_v`` at
   every voxel, no constant involved.  The cases cross the options at which the coordinate chain and the scatter branch.
2. ``LAUNCH_CASES``: real launch sizes.  HIP against the oracle's adjoint per voxel within ``2 (N_v + 1) u G_v`` (same
   weights and gates, another order; no voxel left out), the float64 dot-product identity with HIP's own forward, and float64
   autograd through ``F.grid_sample``: HIP may deviate from it at most twice as far as the oracle does (the factor covers the
   order of the additions; the deviation itself is the float32 rounding of the coordinates, which both engines share bit for
   bit).  Where a fill gate fell differently in float32 and in float64 — read off the oracle's FORWARD, never off an adjoint —
   the taps of that output voxel are left out of this third comparison; a case may leave out 1e-5 of its voxels and asserts it.
3. The autograd plumbing (leaf dtypes, several images, the chunk loop, precision modes, plans made ahead, refusals) and the
   custom op, each against an explicit ``linear_adjoint`` launch within the tolerance of 2.

The CPU halves run the same checkers on the oracle (whose scatter adds in its threads' order: the bounds hold for it as
they do for the kernel).

Largest deviation from the float64 ``grid_sample`` reference, as a fraction of ``max |ref|``.  It is no property of the engines
alone: it follows the magnitude of the coordinates (a float32 ulp doubles at 128) and the host, whose matrix product the
reference's float32 grid goes through.  Hence no constant bounds it; the oracle is held per voxel to
``adjoint_reference.coordinate_rounding_bound`` instead.
    on the development host (oracle)             48 x 40 x 56: 2.7e-6 / 4.1e-6    96 x 80 x 112: 5.4e-6 / 4.9e-6
                                                 (2, 3, 100, 90, 130): 6.1e-6 / 5.8e-6    256^3: 1.75e-5 / 1.65e-5    8 x 128^3: 7.8e-6
    on an MI355X host (oracle and HIP, equal to the three digits printed)
        (2, 3, 100, 90, 130) elastic + fill 2.09e-5, affine 2.33e-5; 256^3 elastic 5.31e-5, affine + fill 4.93e-5 (4 voxels
        left out); 8 x 128^3 elastic + fill 2.33e-5 (8 voxels left out)
    HIP against the oracle: at most 0.025 of the order tolerance; <A x, g> - <x, A^T g> at most 1e-6 of its bound.
"""
from __future__ import annotations

import pytest
import torch

import adjoint_reference as ar
from torchio_amd import ops

SPACING = (1.5, 0.8, 2.0)


def _control(generator, batch, shape, amplitude):
    return (torch.rand(batch, *shape, 3, generator=generator) - 0.5) * 2 * amplitude


def _dense_cases() -> dict:
    """name -> (geometry, batch, channels, fill kind: None / "zeros" / "values")"""
    g = torch.Generator().manual_seed(2026)
    cases = {}
    box = (6, 7, 8)

    def stack(*mappings):
        return torch.stack(list(mappings))

    cases["affine_shared"] = (ar.geometry(in_shape=box, out_shape=box, mapping=stack(ar.scaled_mapping(box, box, zoom=0.95, skew=0.06))), 2, 1, None)
    per_element = stack(ar.scaled_mapping(box, box, zoom=1.05, skew=0.05, shift=(0.4, -0.3, 0.2)),
                        ar.scaled_mapping(box, box, zoom=1.2, skew=-0.08, shift=(-0.6, 0.5, 0.3)),
                        ar.scaled_mapping(box, box, zoom=1.1, skew=0.1, shift=(0.2, 0.7, -0.5)))
    cases["per_element_mapping_fill"] = (ar.geometry(in_shape=box, out_shape=box, mapping=per_element), 3, 1, "values")
    cases["elastic_shared_three_channels_zero_fill"] = (
        ar.geometry(in_shape=box, out_shape=box, mapping=stack(ar.scaled_mapping(box, box, zoom=1.15, skew=0.04)),
                    control_points=_control(g, 1, (4, 4, 4), 1.0)), 2, 3, "zeros")
    cases["per_element_control_points_cp_skip_field_first_spacing"] = (
        ar.geometry(in_shape=box, out_shape=box, mapping=per_element, control_points=_control(g, 3, (4, 5, 4), 1.2), cp_skip=torch.tensor([0, 1, 0], dtype=torch.uint8),
                    affine_first=False, in_spacing=(1, 1, 1), out_spacing=SPACING), 3, 1, "values")
    cases["affine_first_spacing"] = (
        ar.geometry(in_shape=box, out_shape=box, mapping=stack(ar.scaled_mapping(box, box, zoom=1.0, skew=0.05)), control_points=_control(g, 1, (5, 4, 4), 1.2),
                    affine_first=True, in_spacing=SPACING, out_spacing=(1, 1, 1)), 2, 1, None)
    small, large = (5, 6, 7), (8, 9, 11)
    cases["upsample"] = (ar.geometry(in_shape=small, out_shape=large, mapping=stack(ar.scaled_mapping(small, large, zoom=1.1, skew=0.03)),
                                     control_points=_control(g, 1, (4, 4, 4), 0.8)), 2, 1, "values")
    big, few = (8, 8, 6), (5, 5, 4)
    cases["downsample"] = (ar.geometry(in_shape=big, out_shape=few, mapping=stack(ar.scaled_mapping(big, few, zoom=1.05, skew=0.04))), 2, 1, None)
    norm = (8, 9, 10)
    cases["norm_shape"] = (ar.geometry(in_shape=box, out_shape=box, mapping=stack(ar.scaled_mapping(box, box, zoom=1.1, skew=0.05, norm_shape=norm)), norm_shape=norm,
                                       control_points=_control(g, 1, (4, 4, 4), 0.8)), 2, 1, "values")
    cases["passthrough_middle_element"] = (
        ar.geometry(in_shape=box, out_shape=box, mapping=per_element, control_points=_control(g, 3, (4, 4, 4), 1.0),
                    passthrough=torch.tensor([0, 1, 0], dtype=torch.uint8)), 3, 2, "values")
    cases["control_grid_in_global_memory"] = (  # 13 * 13 * 13 * 3 = 6591 floats > 6144: the kernel reads the grid from global memory
        ar.geometry(in_shape=box, out_shape=box, mapping=per_element[:2], control_points=_control(g, 2, (13, 13, 13), 1.5)), 2, 1, "zeros")
    line, plane = (1, 9, 1), (5, 1, 7)
    line_map = ar.scaled_mapping(line, (3, 4, 2), zoom=1.0)
    line_map[1, 0], line_map[1, 2], line_map[1, 3] = 0.9, 0.45, -0.9  # (the other output axes move along the line: 24 voxels reach its 9)
    cases["degenerate_line"] = (ar.geometry(in_shape=line, out_shape=(3, 4, 2), mapping=stack(line_map)), 2, 1, None)
    cases["degenerate_plane"] = (ar.geometry(in_shape=plane, out_shape=plane, mapping=stack(ar.scaled_mapping(plane, plane, zoom=1.1, skew=0.05)),
                                             control_points=_control(g, 1, (4, 2, 4), 0.8)), 2, 1, "values")
    # most of the output grid looks past the volume: 1.6 input voxels per output voxel (every input voxel still within one
    # voxel of a sample), moved by a third of the extent
    cases["translation_out_of_view"] = (
        ar.geometry(in_shape=box, out_shape=box, mapping=stack(ar.scaled_mapping(box, box, zoom=1.6, skew=0.03, shift=(1.6, -1.9, 2.2)))), 2, 1, "values")
    tiny, wide = (5, 5, 6), (26, 26, 31)
    cases["zoom_out_contention"] = (  # five output voxels per input voxel and axis: ~10^3 of them add into an interior voxel
        ar.geometry(in_shape=tiny, out_shape=wide, mapping=stack(ar.scaled_mapping(tiny, wide, zoom=1.04, skew=0.004)),
                    control_points=_control(g, 1, (4, 4, 4), 0.3)), 1, 2, "zeros")
    return cases


DENSE_CASES = _dense_cases()


def _fill(kind, channels, device):
    if kind is None:
        return None
    return (torch.zeros(channels) if kind == "zeros" else torch.linspace(0.7, -1.3, channels)).to(device)


def _dense_problem(name, oracle):
    """The case's geometry, its exact matrix (always from the oracle's forward: the reference does not depend on the engine
    under test) and a gradient; asserts that the case cannot pass vacuously."""
    geo, batch, channels, kind = DENSE_CASES[name]
    matrix = ar.dense_matrix(oracle, geo, batch, kind is not None)
    grad = torch.randn(batch, channels, *geo["out_shape"], generator=torch.Generator().manual_seed(len(name)))
    empty = (matrix != 0).sum(dim=2) == 0
    assert float(empty.double().mean(dim=1).max()) <= 0.2, f"{name}: {empty.double().mean(dim=1).tolist()} of the columns are empty"
    if name == "zoom_out_contention":
        assert int((matrix != 0).sum(dim=2).max()) >= 500
    if name == "translation_out_of_view":
        ungated = ar.dense_matrix(oracle, geo, batch, False)
        assert float(((ungated != 0).sum(dim=1) == 0).double().mean()) > 0.5, "most of the output should leave the view"
    if kind is not None:
        ungated = ar.dense_matrix(oracle, geo, batch, False)
        live = torch.ones(batch, dtype=torch.bool) if geo["passthrough"] is None else ~geo["passthrough"].bool()
        row_sum, kept = ungated.sum(dim=1)[live], (matrix != 0).any(dim=1)[live]
        dropped = ((ungated != 0).any(dim=1)[live] & ~kept).sum()  # in-bounds weight in (0, 1/2]: the fill was taken
        partly_out = (kept & (row_sum < 0.999)).sum()  # kept although some of its taps are out of bounds
        assert int(dropped) >= 1 and int(partly_out) >= 1, (name, int(dropped), int(partly_out))
    return geo, batch, channels, kind, matrix, grad


def _check_dense(engine, device, name, oracle):
    geo, batch, channels, kind, matrix, grad = _dense_problem(name, oracle)
    result = ar.adjoint(engine, grad.to(device), ar.on_device(geo, device), _fill(kind, channels, device))
    figures = ar.check_against_dense(matrix, grad, result)
    if geo["passthrough"] is not None:  # the backward of the bit-exact copy is the identity, bit for bit
        rows = geo["passthrough"].bool()
        assert torch.equal(result.cpu()[rows], grad[rows])
    return figures


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_oracle_adjoint_is_the_exact_transpose(oracle, name):
    _check_dense(oracle, "cpu", name, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_hip_adjoint_is_the_exact_transpose(hip, oracle, name):
    geo, batch, channels, kind = DENSE_CASES[name]
    if name != "zoom_out_contention":  # the matrix the bound is taken from is the HIP forward's as well (bit for bit)
        assert torch.equal(ar.dense_matrix(hip, ar.on_device(geo, "cuda"), batch, kind is not None, "cuda").cpu(), ar.dense_matrix(oracle, geo, batch, kind is not None))
    _check_dense(hip, "cuda", name, oracle)


# ---------------------------------------------------------------------------------------------------------------------
# 2. launch sizes
# ---------------------------------------------------------------------------------------------------------------------
def _launch_geometry(shape, batch_geometry, elastic, seed, zoom=1.0):
    g = torch.Generator().manual_seed(seed)
    count = shape[0] if batch_geometry else 1
    mapping = zoom * torch.eye(3, 4).repeat(count, 1, 1)
    mapping[:, :, :3] += 0.08 * (torch.rand(count, 3, 3, generator=g) - 0.5)
    centre = torch.tensor([(s - 1) / 2 for s in shape[2:]])
    shift = (torch.rand(count, 3, generator=g) - 0.5) * 6
    mapping[:, :, 3] = centre + shift - (mapping[:, :, :3] @ centre)
    control = None
    if elastic:
        control = _control(g, count, (7, 7, 7), 0.03 * min(shape[2:]))
    return ar.geometry(in_shape=shape[2:], out_shape=shape[2:], mapping=mapping, control_points=control)


# name -> (shape, per-element geometry, elastic, fill[, zoom])
# (the eight elements zoom in a little: fewer of their 48 faces cross the fill gate, where a float32 and a float64 chain can
# disagree — the share of voxels a case may leave out for that is capped, and how often they disagree depends on the host whose
# matrix product the reference's float32 grid goes through)
LAUNCH_CASES = {
    "batch2_c3_elastic_fill": ((2, 3, 100, 90, 130), True, True, True),
    "batch2_c3_affine": ((2, 3, 100, 90, 130), False, False, False),
    "bench_volume_elastic": ((1, 1, 256, 256, 256), False, True, False),
    "bench_volume_affine_fill": ((1, 1, 256, 256, 256), False, False, True),
    "eight_elements_elastic_fill": ((8, 1, 128, 128, 128), True, True, True, 0.96),
}
CPU_LAUNCH_CASES = {
    "elastic_fill": ((2, 2, 48, 40, 56), True, True, True),
    "affine": ((1, 1, 96, 80, 112), False, False, False),
    "elastic": ((1, 2, 96, 80, 112), False, True, False),
    "affine_fill": ((2, 1, 48, 40, 56), True, False, True),
}
FLIP_SHARE = 1e-5  # of the input voxels: what a case may leave out of the comparison with float64 autograd for flipped fill gates


def _launch_problem(case, seed):
    shape, batch_geometry, elastic, with_fill = case[:4]
    geo = _launch_geometry(shape, batch_geometry, elastic, seed, *case[4:])
    g = torch.Generator().manual_seed(seed + 1)
    data, grad = torch.rand(shape, generator=g), torch.randn(shape, generator=g)
    fill = torch.linspace(0.4, -0.8, shape[1]) if with_fill else None
    return geo, data, grad, fill


def _oracle_against_autograd(oracle, geo, grad, fill, device):
    """The oracle's adjoint, the float64 autograd reference (on *device*), the input voxels left out for flipped fill gates
    (at most ``FLIP_SHARE`` of them) and the oracle's largest deviation from the reference over the others.  No constant says
    how far a float32 chain may be from float64: the oracle is held, per voxel, to the rounding of its coordinates."""
    theirs = ar.adjoint(oracle, grad, geo, fill)
    reference, kept = ar.aten_reference_adjoint(geo, grad, fill, device)
    leave_out = None
    if fill is not None:
        leave_out = ar.flipped_gates(oracle, geo, grad.shape[0], kept)
        share = float(leave_out.double().mean())
        assert share <= FLIP_SHARE, f"{share:.3g} of the voxels are within reach of a flipped fill gate: pick another seed"
    bound = ar.coordinate_rounding_bound(ar.on_device(geo, device), grad.to(device))
    if leave_out is not None:
        bound = bound.masked_fill(leave_out.expand_as(bound), float("inf"))
    ar.assert_within(theirs.to(device), reference, bound, "oracle against float64 autograd")
    own = ar.deviation(theirs, reference, leave_out)
    assert own > 0
    return theirs, reference, leave_out, own


def _dot_product_identity(engine, geo, data, grad, fill):
    """``<A x, g>`` against ``<x, A^T g>`` with the engine's own forward, for ``x >= 0`` and ``g = |grad| >= 0``: the a-priori
    rounding bound of either side grows with the number of terms, and so must the effect of a systematic error — with
    gradients of both signs a dropped tap would move the sums by a random walk's worth, below the bound."""
    positive = grad.abs()
    linear = ar.forward(engine, data, geo, fill)
    if fill is not None:
        linear = linear - ar.forward(engine, torch.zeros_like(data), geo, fill)
    return ar.dot_product_gap(geo, data, positive, linear, ar.adjoint(engine, positive, geo, fill))


@pytest.mark.parametrize("name", list(CPU_LAUNCH_CASES))
def test_oracle_launch_sizes(oracle, name):
    """The launch-size checkers on the oracle.  Its scatter adds in its threads' order, so a second run of it stands in for
    "another engine with the same weights" in the per-voxel check.  Its deviation from float64 autograd was 2.3e-6 of max|ref|
    at 48 x 40 x 56 and 7.2e-6 at 96 x 80 x 112 when this test was written, with no fill gate flipped; the figure follows the
    coordinates' magnitude (one float32 ulp of a coordinate doubles at 128) and the host's matrix product, which the
    reference's float32 grid goes through."""
    geo, data, grad, fill = _launch_problem(CPU_LAUNCH_CASES[name], 11)
    theirs, reference, leave_out, own = _oracle_against_autograd(oracle, geo, grad, fill, "cpu")
    print(f"\n{name}: oracle deviates {own:.3g} of max|ref| from float64 autograd, {0 if leave_out is None else int(leave_out.sum())} voxels left out")
    gap, bound = _dot_product_identity(oracle, geo, data, grad, fill)
    assert gap <= bound, (gap, bound)
    again = ar.adjoint(oracle, grad, geo, fill)
    ar.assert_within(again, theirs, ar.order_tolerance(geo, grad), name)
    assert ar.deviation(again, reference, leave_out) <= 2 * own


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAUNCH_CASES))
def test_hip_adjoint_at_launch_sizes(hip, oracle, name):
    geo, data, grad, fill = _launch_problem(LAUNCH_CASES[name], 23)
    theirs, reference, leave_out, own = _oracle_against_autograd(oracle, geo, grad, fill, "cuda")
    geo_dev, grad_dev, data_dev = ar.on_device(geo, "cuda"), grad.cuda(), data.cuda()
    fill_dev = None if fill is None else fill.cuda()
    ours = ar.adjoint(hip, grad_dev, geo_dev, fill_dev)
    # (a) per voxel against the oracle, no voxel left out: same weights, same gates, another order of the additions
    tolerance = ar.order_tolerance(geo_dev, grad_dev)
    worst = ar.assert_within(ours, theirs.cuda(), tolerance, name)
    # (b) <A x, g> == <x, A^T g> in float64, with the forward taken from HIP
    gap, bound = _dot_product_identity(hip, geo_dev, data_dev, grad_dev, fill_dev)
    assert gap <= bound, (gap, bound)
    # (c) float64 autograd through grid_sample: at most twice as far from it as the oracle is
    mine = ar.deviation(ours, reference, leave_out)
    print(f"\n{name}: from float64 autograd, of max|ref|: oracle {own:.3g}, hip {mine:.3g}, {0 if leave_out is None else int(leave_out.sum())} voxels left out; "
          f"hip - oracle at most {worst:.3g} of the order tolerance; <Ax, g> - <x, A^T g> = {gap:.3g} (bound {bound:.3g})")
    assert mine <= 2 * own, (mine, own)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the autograd plumbing: everything against an explicit `linear_adjoint` launch, within `order_tolerance`
# ---------------------------------------------------------------------------------------------------------------------
PLUMBING_SHAPE = (2, 2, 40, 36, 44)
# relative half-ulp of the type a gradient is stored in, and its smallest step (gradients that land in the subnormals)
STORAGE = {torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 0.0), torch.float64: (0.0, 0.0), torch.float32: (0.0, 0.0)}


def _plumbing_problem(device, shape=PLUMBING_SHAPE, seed=31, elastic=True):
    geo = ar.on_device(_launch_geometry(shape, True, elastic, seed), device)
    g = torch.Generator().manual_seed(seed + 1)
    data, grad = torch.rand(shape, generator=g).to(device), torch.randn(shape, generator=g).to(device)
    fill = torch.linspace(0.4, -0.8, shape[1]).to(device)
    return geo, data, grad, fill


def _assert_is_the_explicit_launch(engine, geo, leaf_grad, grad, fill, what):
    """``leaf_grad`` (any float dtype) is the explicit launch's accumulator stored in that dtype: two launches of one scatter
    differ by the order of their additions (``order_tolerance``), the store rounds once (``|a| <= |b| + tol`` of the other)."""
    explicit = ar.adjoint(engine, grad.float(), geo, fill)
    relative, step = STORAGE[leaf_grad.dtype]
    tolerance = ar.order_tolerance(geo, grad.float())
    tolerance = tolerance * (1 + relative) + relative * explicit.double().abs() + step
    assert leaf_grad.shape == explicit.shape
    assert float(explicit.abs().max()) > 0
    return ar.assert_within(leaf_grad, explicit, tolerance, what)


def _leaf_dtype(engine, device, dtype):
    geo, data, grad, fill = _plumbing_problem(device)
    leaf = data.to(dtype).requires_grad_(True)
    out = ar.forward(engine, leaf, geo, fill)
    assert out.dtype == dtype and out.requires_grad
    incoming = grad.to(dtype)  # (what autograd hands the backward: a gradient of the output's dtype)
    out.backward(incoming)
    assert leaf.grad.dtype == dtype
    _assert_is_the_explicit_launch(engine, geo, leaf.grad, incoming, fill, str(dtype))


def _several_images(engine, device, count):
    """*count* float images of which every second one requires grad + an int16 label map resampled with "nearest"."""
    geo, data, grad, fill = _plumbing_problem(device, shape=(2, 2, 24, 20, 28))
    g = torch.Generator().manual_seed(count)
    images, fills = [], []
    for n in range(count):
        image = (data + 0.1 * n)[:, : 1 + n % 2].contiguous()
        images.append(image.requires_grad_(True) if n % 2 == 0 else image)
        fills.append(None if n % 3 == 2 else fill[: image.shape[1]] + 0.05 * n)
    labels = torch.randint(0, 5, (2, 1, 24, 20, 28), generator=g).to(torch.int16).to(device)
    outs = engine.resample3d(images + [labels], interps=["linear"] * count + ["nearest"], fills=fills + [None], **ar._launch_arguments(geo))
    assert len(outs) == count + 1 and outs[-1].dtype == torch.int16 and not outs[-1].requires_grad
    grads = [torch.randn(out.shape, generator=g).to(device) for out in outs[:count]]
    assert [out.requires_grad for out in outs[:count]] == [n % 2 == 0 for n in range(count)]
    torch.autograd.backward([outs[n] for n in range(0, count, 2)], [grads[n] for n in range(0, count, 2)])
    for n in range(0, count, 2):
        _assert_is_the_explicit_launch(engine, geo, images[n].grad, grads[n], fills[n], f"image {n} of {count}")
    # the outputs are what a call without autograd returns
    plain = engine.resample3d([t.detach() for t in images] + [labels], interps=["linear"] * count + ["nearest"], fills=fills + [None], **ar._launch_arguments(geo))
    for with_grad, without in zip(outs, plain, strict=True):
        assert torch.equal(with_grad.detach(), without)


def _refusals(engine, device):
    geo, data, grad, fill = _plumbing_problem(device, shape=(1, 1, 8, 8, 8), elastic=False)
    arguments = ar._launch_arguments(geo)
    with pytest.raises(ops.EngineError, match="differentiable"):
        engine.resample3d([data.clone().requires_grad_(True)], interps=["nearest"], fills=[None], **arguments)
    with pytest.raises(ops.EngineError, match="differentiable"):
        engine.resample3d([data.clone().requires_grad_(True)], interps=["label"], fills=[None], **arguments)
    with pytest.raises(ops.EngineError, match="differentiable"):  # one refused image refuses the call
        engine.resample3d([data.clone().requires_grad_(True), data.clone().requires_grad_(True)], interps=["linear", "nearest"], fills=[None, None], **arguments)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_oracle_leaf_dtypes(oracle, dtype):
    _leaf_dtype(oracle, "cpu", dtype)


def test_oracle_several_images_and_the_chunk_loop(oracle):
    from torchio_amd import _abi

    _several_images(oracle, "cpu", 3)
    _several_images(oracle, "cpu", _abi.MAX_IMAGES + 3)


def test_oracle_refuses_gradients_of_nearest_and_label_images(oracle):
    _refusals(oracle, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_hip_leaf_dtypes(hip, dtype):
    _leaf_dtype(hip, "cuda", dtype)


@pytest.mark.gpu
def test_hip_several_images_and_the_chunk_loop(hip):
    from torchio_amd import _abi

    _several_images(hip, "cuda", 3)
    _several_images(hip, "cuda", _abi.MAX_IMAGES + 3)


@pytest.mark.gpu
def test_hip_refuses_gradients_of_nearest_and_label_images(hip):
    _refusals(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["tight", "fast"])
def test_hip_backward_of_a_forward_in_another_precision(hip, precision):
    """The backward is the exact-coordinate adjoint whatever arithmetic the forward ran in."""
    import torchio_amd as tio

    geo, data, grad, fill = _plumbing_problem("cuda", shape=(2, 1, 64, 48, 64))
    previous, opted = tio.get_resample_precision(), ops._FAST_OPTED_IN
    try:
        if precision == "fast":
            with pytest.raises(ValueError, match="allow_out_of_tolerance"):
                ops._FAST_OPTED_IN = False
                tio.set_resample_precision("fast")
            tio.set_resample_precision("fast", allow_out_of_tolerance=True)
        else:
            tio.set_resample_precision(precision)
        leaf = data.clone().requires_grad_(True)
        out = ar.forward(hip, leaf, geo, fill)
        out.backward(grad)
    finally:
        ops._FAST_OPTED_IN = opted
        tio.set_resample_precision(previous)
    _assert_is_the_explicit_launch(hip, geo, leaf.grad, grad, fill, precision)
    # and through the per-call argument
    leaf = data.clone().requires_grad_(True)
    ar.forward(hip, leaf, geo, fill, precision=precision).backward(grad)
    _assert_is_the_explicit_launch(hip, geo, leaf.grad, grad, fill, precision)


@pytest.mark.gpu
def test_hip_backward_of_a_forward_that_was_handed_a_plan(hip):
    shape = (3, 1, 256, 256, 256)  # 12 288 bricks: the smallest launch that starts from a plan
    geo = ar.on_device(_launch_geometry(shape, True, False, 41), "cuda")
    generator = torch.Generator(device="cuda").manual_seed(42)
    data = torch.rand(shape, generator=generator, device="cuda")
    grad = torch.randn(shape, generator=generator, device="cuda")
    fill = torch.tensor([-0.25], device="cuda")
    plan = hip.resample_plan(batch=shape[0], in_shape=shape[2:], precision="exact", **ar._launch_arguments(geo))
    assert plan is not None
    plain = ar.forward(hip, data, geo, fill)
    leaf = data.clone().requires_grad_(True)
    out = ar.forward(hip, leaf, geo, fill, plan=plan)
    assert torch.equal(out.detach(), plain)
    del plain
    out.backward(grad)
    _assert_is_the_explicit_launch(hip, geo, leaf.grad, grad, fill, "plan made ahead")


OP_CASES = [name for name, case in DENSE_CASES.items() if case[0]["cp_skip"] is None and case[0]["norm_shape"] is None]  # (the op takes neither)


@pytest.mark.gpu
@pytest.mark.parametrize("name", OP_CASES)
def test_custom_op_adjoint_over_the_option_cross(hip, oracle, name):
    import torchio_amd.torch_ops  # noqa: F401

    geo, batch, channels, kind, matrix, grad = _dense_problem(name, oracle)
    dev = ar.on_device(geo, "cuda")
    fill = _fill(kind, channels, "cuda")
    result = torch.ops.tio_hip.resample3d_adjoint(grad.cuda(), list(geo["in_shape"]), dev["mapping"], dev["control_points"], [float(s) for s in geo["in_spacing"]],
                                                  [float(s) for s in geo["out_spacing"]], geo["affine_first"], fill, dev["passthrough"])
    figures = ar.check_against_dense(matrix, grad, result)  # the exact transpose ...
    explicit = ar.adjoint(hip, grad.cuda(), dev, fill)
    ar.assert_within(result, explicit, 2 * figures["bound"].cuda(), name)  # ... hence the explicit launch, up to the order (S_v <= G_v)
    # autograd through the forward op ends in the same launch
    data = torch.rand(batch, channels, *geo["in_shape"], generator=torch.Generator().manual_seed(3)).cuda().requires_grad_(True)
    (out,) = torch.ops.tio_hip.resample3d([data], [1], dev["mapping"], dev["control_points"], [float(s) for s in geo["in_spacing"]], [float(s) for s in geo["out_spacing"]],
                                          list(geo["out_shape"]), geo["affine_first"], [fill], dev["passthrough"], 0)
    out.backward(grad.cuda())
    ar.check_against_dense(matrix, grad, data.grad)
