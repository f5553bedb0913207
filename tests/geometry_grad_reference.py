"""Test-only reference, bounds and cases for ``tio_resample3d_geometry_grad`` (tests/test_geometry_grad_host.py,
tests/test_gpu_geometry_grad.py, tests/test_gpu_geometry_grad_guarded.py).  Nothing here is imported by the product.

The reference is float64 autograd: ``adjoint_reference.coordinates64`` - the coordinate chain without its float32 roundings,
differentiable in the mapping and the control points - fed with float64 leaves, normalised, ``F.grid_sample(align_corners=True,
padding_mode="zeros")`` in float64, the ones-mask ``torch.where`` for fills, ``torch.autograd.grad`` of ``<out, g>``.  It shares no
line with the kernel.

Next to it the module restates the gradient ANALYTICALLY in float64 (``analytic``): the per-voxel derivative ``D_a``, the chain to
the 12 + ``ni nj nk 3`` parameters.  The host test holds that restatement to the autograd reference; its only purpose is that its
absolute-value twin gives, per output component ``p``, the magnitude the kernel's roundings are relative to,

    A_p = sum over voxels of  |g| * sum_t |x_t| * |dv/dp|      (in-bounds taps, un-weighted; gated voxels left out)

and with it two allowances:

**Rounding bound** ``R_p = (60 c + k) u A_p + L_p``, ``u = 2^-24``.

* ``60 u c``, ``c`` the largest extent in the call: the project's figure for what a float32 sampling coordinate may do to a tap
  weight (``adjoint_reference.coordinate_rounding_bound``), reused as it stands.  ``D_a`` multiplies a tap by the weights of the two
  OTHER axes, each of which moves by the coordinate's error whatever its own size - which is why ``A_p`` carries no weights.
* ``k = 32 + C`` counts the kernel's own roundings, each relative to a partial sum that ``A_p`` bounds (``C`` the channels of the
  call: ``D`` is accumulated channel by channel, image by image).  Per voxel and channel: the weights ``c + 1 - x`` / ``x - c`` (1
  each, 2 in a product) and their product (1): 3; ``v1 - v0``: 1; times the weight product: 1; the sum of the four terms: 3; times
  ``g``: 1; the accumulation over the channels: ``C``; the ratio ``(S_own - 1) / max(S_norm - 1, 1)`` and the product with it: 2.
  That is ``11 + C``.  The chain: ``d * P``: 1, and where the displacement goes through the matrix, ``P = c + disp / spacing`` (3)
  and ``M^T d`` (5), the division by the spacing 1: at most 10.  The reduction: 8 additions per lane, 6 shuffle levels, the
  rounding of the float64 total to float32: 15 for the mapping; for a control value the wave sum (6), the product with the k weight
  (1), ``(w_i w_j) t`` (2) and the final rounding (1): 10.  Mapping: ``11 + C + 4 + 15 = 30 + C``; control points: ``11 + C + 10 + 10 =
  31 + C``; ``k = 32 + C`` covers both.
* ``L_p`` (control points only): the lerp weights.  ``lerp_index`` forms ``real = scale * o`` (2 roundings, of the size of ``real``)
  and ``l1 = real - i0``, ``l0 = 1 - l1``: an ABSOLUTE error of ``(2 real + 2) u`` on each of the two nodes of the voxel's cell,
  which no multiple of a small weight covers.  ``L_p`` is the trilinear sum of ``|dDisp|`` with one axis' weights replaced by that
  error, for each axis in turn.

**Kink allowance** ``K_p``.  The interpolant's derivative jumps where a coordinate crosses an integer, the gate where the in-bounds
weight crosses 1/2; a float32 chain may stand on the other side than float64.  A voxel is *ambiguous* when its float64 coordinate
lies within ``60 u max(|c|, 1)`` of an integer on an axis of extent > 1, or its in-bounds weight within ``1e-5`` of 1/2 (images with
a fill).  ``K_p`` is the sum over the ambiguous voxels of ``|g| |difference of the two one-sided derivatives| |dv/dp|`` (for a gate:
the whole term).  ``conditions`` states how few such voxels a case may have; the host test asserts it for every case.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from adjoint_reference import U
from adjoint_reference import coordinates64
from adjoint_reference import geometry
from adjoint_reference import scaled_mapping

GATE_WINDOW = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the reference: float64 autograd through grid_sample
# ---------------------------------------------------------------------------------------------------------------------
def _as64(image: torch.Tensor) -> torch.Tensor:
    """The values the kernel computes with: float64 images are rounded to float32 on load, the others are exact in it."""
    return image.detach().cpu().to(torch.float32).double()


def _sample64(volume: torch.Tensor, coords: torch.Tensor, in_shape) -> torch.Tensor:
    """``F.grid_sample`` of ``(B, C, I, J, K)`` float64 at voxel coordinates ``(B, Io, Jo, Ko, 3)``: zero padding, align_corners."""
    scale = torch.tensor([2.0 / (s - 1) if s > 1 else 0.0 for s in in_shape], dtype=torch.float64)
    offset = torch.tensor([1.0 if s > 1 else 0.0 for s in in_shape], dtype=torch.float64)
    grid = (coords * scale - offset).permute(0, 3, 2, 1, 4)  # x = i = ATen's W: the volume goes in as (B, C, K, J, I)
    out = F.grid_sample(volume.permute(0, 1, 4, 3, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.permute(0, 1, 4, 3, 2)


def autograd_reference(geo: dict, images, grads, fills) -> tuple[torch.Tensor, torch.Tensor | None]:
    """``d sum_n <resample(x_n), g_n> / d (mapping, control_points)`` in float64, in the shapes of the two tensors."""
    batch = images[0].shape[0]
    mapping = geo["mapping"].detach().cpu().double().requires_grad_(True)
    control = None if geo["control_points"] is None else geo["control_points"].detach().cpu().double().requires_grad_(True)
    with torch.enable_grad():
        coords = coordinates64({**_host(geo), "mapping": mapping, "control_points": control}, batch)
        total = torch.zeros((), dtype=torch.float64)
        for image, grad, fill in zip(images, grads, fills, strict=True):
            volume = _as64(image)
            out = _sample64(volume, coords, geo["in_shape"])
            if fill is not None:
                mask = _sample64(torch.ones_like(volume[:, :1]), coords, geo["in_shape"])
                out = torch.where(mask > 0.5, out, fill.detach().cpu().double().view(1, -1, 1, 1, 1))
            total = total + (out * grad.detach().cpu().double()).sum()
        leaves = [mapping] + ([] if control is None else [control])
        results = torch.autograd.grad(total, leaves, allow_unused=True)
    results = [torch.zeros_like(leaf) if r is None else r for r, leaf in zip(results, leaves, strict=True)]
    return results[0], (results[1] if control is not None else None)


def _host(geo: dict) -> dict:
    return {key: value.detach().cpu() if isinstance(value, torch.Tensor) else value for key, value in geo.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the analytic restatement and its absolute-value twins
# ---------------------------------------------------------------------------------------------------------------------
def lerp_matrix(n_nodes: int, n_out: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(W, E)``, both ``(n_out, n_nodes)`` float64: the align-corners lerp weights of every output index, and the absolute
    error a float32 ``lerp_index`` may have on them (on the nodes within one cell of the output's position)."""
    nodes = torch.arange(n_nodes, dtype=torch.float64)
    if n_out == n_nodes:
        return torch.eye(n_nodes, dtype=torch.float64), torch.zeros(n_nodes, n_nodes, dtype=torch.float64)
    scale = (n_nodes - 1) / (n_out - 1) if n_out > 1 else 0.0
    real = scale * torch.arange(n_out, dtype=torch.float64)
    weights = (1 - (real[:, None] - nodes[None, :]).abs()).clamp(min=0.0)
    near = (real[:, None] - nodes[None, :]).abs() < 1 + 1e-6
    return weights, near.double() * ((2 * real + 2) * U)[:, None]


def _derivative(volume, grad, coords, cell, keep):
    """``(D, T)``: ``D[b, i, j, k, a] = sum_c g * sum_t x_t s_a(t) w_other(t)`` and ``T[b, i, j, k] = sum_c |g| sum_t |x_t|`` over the
    in-bounds taps of *cell* ``(B, Io, Jo, Ko, 3)`` (int64), both zero where *keep* ``(B, Io, Jo, Ko)`` is False."""
    batch, channels, *in_shape = volume.shape
    upper = coords - cell.double()  # weight of the upper tap per axis; the lower tap's is 1 - upper
    flat = volume.reshape(batch, channels, -1)
    derivative = torch.zeros((*coords.shape[:-1], 3), dtype=torch.float64)
    magnitude = torch.zeros(coords.shape[:-1], dtype=torch.float64)
    for tap in range(8):
        bits = [(tap >> a) & 1 for a in range(3)]
        index = [cell[..., a] + bits[a] for a in range(3)]
        ok = torch.ones(coords.shape[:-1], dtype=torch.bool)
        for a in range(3):
            ok &= (index[a] >= 0) & (index[a] < in_shape[a])
        linear = (index[0].clamp(0, in_shape[0] - 1) * in_shape[1] + index[1].clamp(0, in_shape[1] - 1)) * in_shape[2] + index[2].clamp(0, in_shape[2] - 1)
        values = torch.gather(flat, 2, linear.reshape(batch, 1, -1).expand(batch, channels, -1)).reshape(batch, channels, *coords.shape[1:-1])
        values = values * ok[:, None]
        weight = [upper[..., a] if bits[a] else 1 - upper[..., a] for a in range(3)]
        weighted = (values * grad).sum(dim=1)
        magnitude += (values.abs() * grad.abs()).sum(dim=1)
        for a in range(3):
            others = weight[(a + 1) % 3] * weight[(a + 2) % 3]
            derivative[..., a] += (1 if bits[a] else -1) * weighted * others
    return derivative * keep[..., None], magnitude * keep


def _in_bounds_weight(coords, in_shape):
    cell = torch.floor(coords).to(torch.int64)
    upper = coords - cell.double()
    total = torch.zeros(coords.shape[:-1], dtype=torch.float64)
    for tap in range(8):
        weight = torch.ones_like(total)
        for a in range(3):
            bit = (tap >> a) & 1
            index = cell[..., a] + bit
            weight = weight * (upper[..., a] if bit else 1 - upper[..., a]) * ((index >= 0) & (index < in_shape[a]))
        total += weight
    return total


def analytic(geo: dict, images, grads, fills) -> dict:
    """The gradient restated analytically in float64, with ``A_p``, ``R_p``, ``K_p`` per component and the ambiguity census.

    Keys: ``mapping`` / ``control`` (the gradients, ``control`` None without control points), ``A_mapping`` / ``A_control``,
    ``R_mapping`` / ``R_control``, ``K_mapping`` / ``K_control``, ``ambiguous`` (voxels), ``voxels``, ``k``, ``c``."""
    geo = _host(geo)
    batch = images[0].shape[0]
    in_shape, out_shape = geo["in_shape"], geo["out_shape"]
    coords = coordinates64({**geo, "mapping": geo["mapping"].double(),
                            "control_points": None if geo["control_points"] is None else geo["control_points"].double()}, batch)
    live = torch.ones(batch, dtype=torch.bool) if geo["passthrough"] is None else ~geo["passthrough"].bool()
    live_voxels = live.view(-1, 1, 1, 1).expand(coords.shape[:-1])
    cell = torch.floor(coords).to(torch.int64)

    # ambiguity: a coordinate within 60 u max(|c|, 1) of an integer (axes of extent > 1), an in-bounds weight within 1e-5 of 1/2
    nearest = torch.round(coords)
    near_integer = (coords - nearest).abs() <= 60 * U * coords.abs().clamp(min=1.0)
    for a in range(3):
        if in_shape[a] == 1:
            near_integer[..., a] = False
    near_integer &= live_voxels[..., None]
    inside = _in_bounds_weight(coords, in_shape)
    near_gate = ((inside - 0.5).abs() <= GATE_WINDOW) & live_voxels

    derivative = torch.zeros((*coords.shape[:-1], 3), dtype=torch.float64)
    magnitude = torch.zeros(coords.shape[:-1], dtype=torch.float64)
    jump = torch.zeros_like(derivative)
    ambiguous = near_integer.any(dim=-1)
    channels = 0
    for image, grad, fill in zip(images, grads, fills, strict=True):
        volume, g = _as64(image), grad.detach().cpu().double()
        channels += volume.shape[1]
        keep = live_voxels & ((inside > 0.5) if fill is not None else torch.ones_like(live_voxels))
        d, t = _derivative(volume, g, coords, cell, keep)
        derivative += d
        magnitude += t
        for a in range(3):  # the two one-sided derivatives along an ambiguous axis: the cells on either side of the integer
            if not bool(near_integer[..., a].any()):
                continue
            above, below = cell.clone(), cell.clone()
            above[..., a] = nearest[..., a].to(torch.int64)
            below[..., a] = above[..., a] - 1
            d_above, _ = _derivative(volume, g, coords, above, keep)
            d_below, _ = _derivative(volume, g, coords, below, keep)
            jump[..., a] += (d_above[..., a] - d_below[..., a]).abs() * near_integer[..., a]
        if fill is not None:
            ambiguous = ambiguous | near_gate
            if bool(near_gate.any()):  # a gate that may fall either way: the whole term
                d_open, _ = _derivative(volume, g, coords, cell, live_voxels)
                jump += d_open.abs() * near_gate[..., None]

    norm = geo["norm_shape"] if geo["norm_shape"] is not None else in_shape
    ratio = torch.tensor([(s - 1) / max(n - 1, 1) for s, n in zip(in_shape, norm, strict=True)], dtype=torch.float64)
    mapping = geo["mapping"].double()
    control = None if geo["control_points"] is None else geo["control_points"].double()
    axes = [torch.arange(n, dtype=torch.float64) for n in out_shape]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    spacing = torch.tensor(geo["in_spacing"] if geo["affine_first"] else geo["out_spacing"], dtype=torch.float64)
    lerps = None if control is None else [lerp_matrix(control.shape[1 + a], out_shape[a]) for a in range(3)]

    def spread(field):  # (Io, Jo, Ko, 3) -> the control grid: the transpose of the trilinear upsampling
        return torch.einsum("ia,jb,kc,ijke->abce", lerps[0][0], lerps[1][0], lerps[2][0], field)

    def spread_error(field):
        (wi, ei), (wj, ej), (wk, ek) = lerps
        return (torch.einsum("ia,jb,kc,ijke->abce", ei, wj, wk, field) + torch.einsum("ia,jb,kc,ijke->abce", wi, ej, wk, field)
                + torch.einsum("ia,jb,kc,ijke->abce", wi, wj, ek, field))

    names = ("mapping", "A_mapping", "K_mapping")
    sums = {name: torch.zeros_like(mapping) for name in names}
    if control is not None:
        sums.update({name: torch.zeros_like(control) for name in ("control", "A_control", "K_control", "L_control")})
    for b in range(batch):
        if not bool(live[b]):
            continue
        m = mapping[b if mapping.shape[0] > 1 else 0]
        elastic = control is not None and not (geo["cp_skip"] is not None and bool(geo["cp_skip"][b]))
        chained = elastic and not geo["affine_first"]
        position = grid
        if chained:
            coarse = control[b if control.shape[0] > 1 else 0]
            position = grid + torch.einsum("ia,jb,kc,abce->ijke", lerps[0][0], lerps[1][0], lerps[2][0], coarse) / spacing
        position = torch.cat([position, torch.ones_like(position[..., :1])], dim=-1)
        fields = {"mapping": derivative[b] * ratio, "A_mapping": magnitude[b][..., None] * ratio, "K_mapping": jump[b] * ratio}
        slot = b if mapping.shape[0] > 1 else 0
        sums["mapping"][slot] += torch.einsum("ijkr,ijkc->rc", fields["mapping"], position)
        sums["A_mapping"][slot] += torch.einsum("ijkr,ijkc->rc", fields["A_mapping"], position.abs())
        sums["K_mapping"][slot] += torch.einsum("ijkr,ijkc->rc", fields["K_mapping"], position.abs())
        if elastic:
            jacobian = (m[:, :3] if chained else torch.eye(3, dtype=torch.float64)) / spacing  # [a][e] = d v_a / d disp_e (before the ratio)
            slot = b if control.shape[0] > 1 else 0
            sums["control"][slot] += spread(fields["mapping"] @ jacobian)
            absolute = fields["A_mapping"] @ jacobian.abs()
            sums["A_control"][slot] += spread(absolute)
            sums["L_control"][slot] += spread_error(absolute)
            sums["K_control"][slot] += spread(fields["K_mapping"] @ jacobian.abs())

    extent = float(max(*in_shape, *out_shape, *norm))
    k = 32 + channels
    result = {"mapping": sums["mapping"], "A_mapping": sums["A_mapping"], "K_mapping": sums["K_mapping"],
              "R_mapping": (60 * extent + k) * U * sums["A_mapping"], "control": None, "ambiguous": int(ambiguous.sum()),
              "voxels": int(live_voxels.sum()), "k": k, "c": extent}
    if control is not None:
        result.update(control=sums["control"], A_control=sums["A_control"], K_control=sums["K_control"],
                      R_control=(60 * extent + k) * U * sums["A_control"] + sums["L_control"])
    return result


def conditions(case: dict) -> None:
    """What a case must meet for its kink allowance to mean anything (asserted on the host for every case)."""
    ref, total = case["analytic"], case["analytic"]["voxels"]
    if total < 10_000:
        assert ref["ambiguous"] == 0, f"{case['name']}: {ref['ambiguous']} ambiguous voxels in a case of {total}: pick another seed"
    else:
        assert ref["ambiguous"] <= 1e-3 * total, f"{case['name']}: {ref['ambiguous']} ambiguous voxels of {total}"
    kinks = [ref["K_mapping"].max()] + ([] if ref["control"] is None else [ref["K_control"].max()])
    largest = [case["reference"][0].abs().max()] + ([] if ref["control"] is None else [case["reference"][1].abs().max()])
    assert max(kinks) <= 1e-3 * max(largest), f"{case['name']}: kink allowance {float(max(kinks)):.3g} against {float(max(largest)):.3g}"


def check(case: dict, d_mapping, d_control) -> float:
    """Every component of the kernel's result within ``R_p + K_p`` of the autograd reference; returns the largest error / bound."""
    ref = case["analytic"]
    worst = 0.0
    pairs = [("mapping", d_mapping, case["reference"][0])]
    if ref["control"] is not None:
        pairs.append(("control", d_control, case["reference"][1]))
    for name, actual, expected in pairs:
        assert actual is not None and actual.dtype == torch.float32 and tuple(actual.shape) == tuple(expected.shape), (case["name"], name)
        error = (actual.detach().cpu().double() - expected).abs()
        bound = ref[f"R_{name}"] + ref[f"K_{name}"]
        ratio = torch.where(bound > 0, error / bound, torch.where(error > 0, torch.full_like(error, float("inf")), torch.zeros_like(error)))
        print(f"{case['name']}: d_{name}: max |ref| {float(expected.abs().max()):.4g}, max error {float(error.max()):.3g}, "
              f"max error / (R + K) {float(ratio.max()):.3g}, max K / max |ref| {float(ref[f'K_{name}'].max() / expected.abs().max().clamp(min=1e-300)):.3g}")
        bad = int((error > bound).sum())
        assert bad == 0, f"{case['name']}: {bad} components of d_{name} beyond R + K; worst error / bound {float(ratio.max()):.3g}"
        worst = max(worst, float(ratio.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def rough_image(generator, batch, channels, shape, dtype=torch.float32) -> torch.Tensor:
    """A smooth part (products of sines, per channel its own phase) plus uniform noise of a third of its amplitude."""
    axes = [torch.arange(s, dtype=torch.float64) for s in shape]
    i, j, k = torch.meshgrid(*axes, indexing="ij")
    out = torch.empty(batch, channels, *shape, dtype=torch.float64)
    for b in range(batch):
        for c in range(channels):
            phase = 0.7 * b + 1.3 * c
            out[b, c] = torch.sin(0.55 * i + phase) * torch.cos(0.41 * j - phase) + 0.5 * torch.sin(0.33 * k + 0.2 * j + phase)
    out += (torch.rand(out.shape, generator=generator, dtype=torch.float64) - 0.5) * 0.6
    return out.to(dtype)


def smooth_control(generator, batch, nodes, amplitude=1.5) -> torch.Tensor:
    return ((torch.rand(batch, *nodes, 3, generator=generator, dtype=torch.float64) - 0.5) * 2 * amplitude).to(torch.float32)


def coherent_gradient(generator, geo, image, fill) -> torch.Tensor:
    """An incoming gradient as a registration loss makes it: the difference between the image sampled 0.37 voxels further along
    every axis and the image sampled where the geometry says, plus uniform noise - so that the sums do not cancel to nothing."""
    batch = image.shape[0]
    coords = coordinates64({**_host(geo), "mapping": geo["mapping"].double(),
                            "control_points": None if geo["control_points"] is None else geo["control_points"].double()}, batch)
    volume = _as64(image)
    moved = _sample64(volume, coords + 0.37, geo["in_shape"]) - _sample64(volume, coords, geo["in_shape"])
    return (moved + (torch.rand(moved.shape, generator=generator, dtype=torch.float64) - 0.5) * 0.2).to(torch.float32).contiguous()


def _case(name, seed, *, in_shape, out_shape, batch, channels=(2,), dtypes=None, nodes=(4, 4, 4), shared_mapping=False, shared_control=False,
          fills=False, zoom=0.93, shift=(0.31, -0.27, 0.43), skew=0.06, **extra) -> dict:
    generator = torch.Generator().manual_seed(seed)
    norm_shape = extra.get("norm_shape")
    rows = []
    for b in range(1 if shared_mapping else batch):
        jitter = (torch.rand(3, generator=generator, dtype=torch.float64) - 0.5) * 0.4
        rows.append(scaled_mapping(in_shape, out_shape, zoom=zoom * (1 + 0.03 * b), shift=tuple(float(s + t) for s, t in zip(shift, jitter, strict=True)),
                                   skew=skew, norm_shape=norm_shape))
    control = None if nodes is None else smooth_control(generator, 1 if shared_control else batch, nodes)
    geo = geometry(in_shape=in_shape, out_shape=out_shape, mapping=torch.stack(rows), control_points=control, **extra)
    dtypes = dtypes or [torch.float32] * len(channels)
    images = [rough_image(generator, batch, c, in_shape, dtype) for c, dtype in zip(channels, dtypes, strict=True)]
    fill_values = [torch.linspace(-0.5, 0.8, c) if fills else None for c in channels]
    grads = [coherent_gradient(generator, geo, image, fill) for image, fill in zip(images, fill_values, strict=True)]
    return {"name": name, "geo": geo, "images": images, "grads": grads, "fills": fill_values}


_BUILDERS = {
    "1-batched": lambda: _case("1-batched", 1, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2),
    "2-chained-spacing": lambda: _case("2-chained-spacing", 2, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, affine_first=False,
                                       in_spacing=(1.5, 0.8, 2.0), out_spacing=(1.2, 1.0, 0.7)),
    "3-shared": lambda: _case("3-shared", 3, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=3, nodes=(4, 5, 6), shared_mapping=True, shared_control=True),
    "4-flags": lambda: _case("4-flags", 4, in_shape=(6, 7, 8), out_shape=(6, 7, 8), batch=3, cp_skip=torch.tensor([0, 1, 0], dtype=torch.uint8),
                             passthrough=torch.tensor([0, 0, 1], dtype=torch.uint8)),
    "5-out-of-bounds": lambda: _case("5-out-of-bounds", 5, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, zoom=1.4, shift=(1.3, -0.9, 1.1)),
    "5-out-of-bounds-fill": lambda: _case("5-out-of-bounds-fill", 5, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, zoom=1.4, shift=(1.3, -0.9, 1.1),
                                          fills=True),
    "6-norm-shape": lambda: _case("6-norm-shape", 6, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, norm_shape=(9, 8, 11)),
    "7-two-dimensional": lambda: _case("7-two-dimensional", 7, in_shape=(1, 9, 11), out_shape=(1, 9, 11), batch=2, nodes=(2, 4, 4)),
    "8-ko70": lambda: _case("8-ko70", 20, in_shape=(6, 5, 8), out_shape=(9, 5, 70), batch=1, channels=(1,)),
    "8-ko3": lambda: _case("8-ko3", 9, in_shape=(6, 5, 8), out_shape=(9, 5, 3), batch=2, channels=(1,)),
    "9-two-images": lambda: _case("9-two-images", 10, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, channels=(1, 3)),
    "9-dtypes": lambda: _case("9-dtypes", 11, in_shape=(6, 5, 8), out_shape=(5, 7, 6), batch=2, channels=(1, 1, 2),
                              dtypes=[torch.float16, torch.bfloat16, torch.float64]),
    "10-many-blocks": lambda: _case("10-many-blocks", 12, in_shape=(12, 10, 16), out_shape=(32, 32, 128), batch=2, channels=(1,), nodes=(7, 7, 7)),
}
CASE_NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """The inputs of a case with its two references, computed once per process and shared (treat as read-only)."""
    built = _BUILDERS[name]()
    built["reference"] = autograd_reference(built["geo"], built["images"], built["grads"], built["fills"])
    built["analytic"] = analytic(built["geo"], built["images"], built["grads"], built["fills"])
    return built
