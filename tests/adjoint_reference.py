"""Test-only helpers of tests/test_gpu_adjoint.py and tests/test_gpu_backward.py: references and per-voxel bounds for the
trilinear adjoint scatter (``TIO_LINEAR_ADJOINT``).  Nothing here is imported by the product.

Three references, from the tightest to the most independent:

* ``dense_matrix``: at small shapes the forward of the one-hot volumes IS the matrix ``A`` of the resampling, in exactly the
  float32 weights the kernels use (``0 + 1 * w = w``; the forward is pinned bit for bit elsewhere).  ``A^T g`` in float64 is
  then the exact answer and the only freedom an implementation has is the order in which it adds its rounded products.
* ``coordinates64`` / ``scatter_bound``: at launch sizes ``A`` is too large; the sampling coordinates restated in float64
  give, per input voxel, an upper bound of the number of contributions and of their magnitudes.
* ``aten_reference_adjoint``: what autograd derives through ``F.grid_sample`` (+ the ones-mask ``torch.where``) in float64,
  from the float32 grid of ``tests/aten_pipeline._grid``: it shares no line with the engines.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from aten_pipeline import _grid

U = 2.0 ** -24  # unit roundoff of float32 (round to nearest)


# ---------------------------------------------------------------------------------------------------------------------
# geometry of one launch: a plain dict of what Engine.resample3d takes besides the images
# ---------------------------------------------------------------------------------------------------------------------
def geometry(*, in_shape, out_shape, mapping, control_points=None, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True,
             cp_skip=None, passthrough=None, norm_shape=None) -> dict:
    return dict(in_shape=tuple(in_shape), out_shape=tuple(out_shape), mapping=mapping, control_points=control_points,
                in_spacing=tuple(in_spacing), out_spacing=tuple(out_spacing), affine_first=affine_first, cp_skip=cp_skip,
                passthrough=passthrough, norm_shape=norm_shape)


def on_device(geo: dict, device) -> dict:
    return {key: value.to(device) if isinstance(value, torch.Tensor) else value for key, value in geo.items()}


def _launch_arguments(geo: dict) -> dict:
    return {key: value for key, value in geo.items() if key != "in_shape"}


def forward(engine, data: torch.Tensor, geo: dict, fill, **extra) -> torch.Tensor:
    (out,) = engine.resample3d([data], interps=["linear"], fills=[fill], **_launch_arguments(geo), **extra)
    return out


def adjoint(engine, grad: torch.Tensor, geo: dict, fill) -> torch.Tensor:
    """The explicit ``linear_adjoint`` launch: dL/d(input) (float32) of the incoming gradient *grad* ``(B, C, *out_shape)``."""
    accumulator = torch.zeros((*grad.shape[:2], *geo["in_shape"]), dtype=torch.float32, device=grad.device)
    engine.resample3d([accumulator], interps=["linear_adjoint"], fills=[fill], _adjoint_of=[grad], **_launch_arguments(geo))
    return accumulator


def scaled_mapping(in_shape, out_shape, *, zoom=1.0, shift=(0.0, 0.0, 0.0), skew=0.0, norm_shape=None) -> torch.Tensor:
    """A ``(3, 4)`` output-voxel -> input-voxel mapping that carries the centre of the output grid to the centre of the input
    grid (+ *shift*, in input voxels) with the ratio of the two extents times *zoom* on the diagonal — a mapping that is not
    scaled with the shape ratio leaves the bulk of a larger output grid out of view — and *skew* off the diagonal."""
    reach = norm_shape if norm_shape is not None else in_shape
    rows = torch.zeros(3, 4, dtype=torch.float64)
    for d in range(3):
        ratio = (reach[d] - 1) / max(out_shape[d] - 1, 1) if reach[d] > 1 else 0.0
        rows[d, d] = ratio * zoom
        for e in range(3):
            if e != d:
                rows[d, e] = skew * (1 if (d + e) % 2 else -1) * (0.5 + 0.25 * d)
    centre_out = torch.tensor([(s - 1) / 2 for s in out_shape], dtype=torch.float64)
    centre_in = torch.tensor([(s - 1) / 2 for s in reach], dtype=torch.float64)
    rows[:, 3] = centre_in + torch.tensor(shift, dtype=torch.float64) - rows[:, :3] @ centre_out
    return rows.to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the dense matrix
# ---------------------------------------------------------------------------------------------------------------------
def dense_matrix(engine, geo: dict, batch: int, has_fill: bool, device="cpu") -> torch.Tensor:
    """``A`` as ``(B, n_in, n_out)`` float32: ``A[b, v, o]`` is what output voxel ``o`` of element ``b`` takes from input voxel
    ``v``.  The ``n_in`` one-hot volumes ride as CHANNELS, so that every element meets its own mapping / control points /
    flags.  With a fill rule the forward of the zero volume is subtracted: what is left is ``gate * w`` — the fill gate is part
    of ``A`` (and ``f - f`` is exactly zero where the fill was taken)."""
    i, j, k = geo["in_shape"]
    n = i * j * k
    one_hots = torch.eye(n, dtype=torch.float32, device=device).reshape(1, n, i, j, k).repeat(batch, 1, 1, 1, 1)
    fill = torch.linspace(-3.0, 5.0, n, device=device) if has_fill else None  # (any values: they cancel)
    matrix = forward(engine, one_hots, geo, fill)
    if has_fill:
        matrix = matrix - forward(engine, torch.zeros_like(one_hots), geo, fill)
    return matrix.reshape(batch, n, -1)


def check_against_dense(matrix: torch.Tensor, grad: torch.Tensor, result: torch.Tensor) -> dict:
    """``|acc_v - (A^T g)_v| <= (N_v + 1) u S_v`` at EVERY input voxel, ``S = |A|^T |g|`` and ``N_v`` the non-zeros of
    column ``v``: the a-priori bound of a float32 sum of ``N_v`` rounded products taken in any order (each product errs by at
    most ``u |g w|``, each of the ``N_v - 1`` additions by ``u`` times a partial sum that ``S_v (1 + N_v u)`` bounds; ``N_v + 1``
    absorbs the second-order terms for every ``N_v`` a test can reach).  Returns the figures for the caller's own assertions."""
    batch, channels = grad.shape[:2]
    a64 = matrix.double().cpu()
    g64 = grad.double().cpu().reshape(batch, channels, -1)
    reference = torch.einsum("bvo,bco->bcv", a64, g64)
    magnitude = torch.einsum("bvo,bco->bcv", a64.abs(), g64.abs())
    counts = (a64 != 0).sum(dim=2).double()[:, None, :]
    bound = (counts + 1) * U * magnitude
    error = (result.double().cpu().reshape(batch, channels, -1) - reference).abs()
    worst = torch.where(bound > 0, error / bound, torch.where(error > 0, torch.full_like(error, math.inf), torch.zeros_like(error)))
    bad = int((error > bound).sum())
    assert bad == 0, f"{bad} voxels beyond the summation bound; worst error / bound = {float(worst.max()):.3g}"
    return {"worst_ratio": float(worst.max()), "max_count": int(counts.max()), "reference": reference.reshape(result.shape),
            "bound": bound.reshape(result.shape), "empty_columns": (counts[:, 0, :] == 0).double().mean(dim=1)}


# ---------------------------------------------------------------------------------------------------------------------
# 2. float64 coordinates: how many output voxels can add into an input voxel, and how much
# ---------------------------------------------------------------------------------------------------------------------
def coordinates64(geo: dict, batch: int, device="cpu") -> torch.Tensor:
    """The sampling coordinates ``(B, Io, Jo, Ko, 3)`` in input voxels, float64: the operations of the engines' coordinate
    chain (include/tio_hip.h) without their float32 roundings.  Gated-out elements (``passthrough``) sample their own voxel."""
    io, jo, ko = geo["out_shape"]
    axes = [torch.arange(n, dtype=torch.float64, device=device) for n in (io, jo, ko)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)  # (Io, Jo, Ko, 3)
    mapping = geo["mapping"].to(device=device, dtype=torch.float64)
    control = geo["control_points"]
    spacing = torch.tensor(geo["in_spacing"] if geo["affine_first"] else geo["out_spacing"], dtype=torch.float64, device=device)
    out = []
    for b in range(batch):
        m = mapping[b if mapping.shape[0] > 1 else 0]
        elastic = control is not None and not (geo["cp_skip"] is not None and bool(geo["cp_skip"][b]))
        if geo["passthrough"] is not None and bool(geo["passthrough"][b]):
            out.append(grid.clone())
            continue
        displacement = None
        if elastic:
            coarse = control[b if control.shape[0] > 1 else 0].to(device=device, dtype=torch.float64)
            field = F.interpolate(coarse.permute(3, 0, 1, 2)[None], size=(io, jo, ko), mode="trilinear", align_corners=True)
            displacement = field[0].permute(1, 2, 3, 0) / spacing
        if displacement is not None and not geo["affine_first"]:
            source = grid + displacement
            voxels = source @ m[:, :3].T + m[:, 3]
        else:
            voxels = grid @ m[:, :3].T + m[:, 3]
            if displacement is not None:
                voxels = voxels + displacement
        if geo["norm_shape"] is not None:  # normalised with another shape than the one it is un-normalised with
            scale = [(s - 1) / max(n - 1, 1) for s, n in zip(geo["in_shape"], geo["norm_shape"], strict=True)]
            voxels = voxels * torch.tensor(scale, dtype=torch.float64, device=device)
        for d in range(3):  # an axis of one voxel: every coordinate lands on it ((g + 1) / 2 * 0)
            if geo["in_shape"][d] == 1:
                voxels[..., d] = 0.0
        out.append(voxels)
    return torch.stack(out)


def reach(geo: dict, per_output: torch.Tensor, taps_only: bool = False) -> torch.Tensor:
    """``(B, C, I, J, K)`` float64: per input voxel, the sum of *per_output* ``(B, C, Io, Jo, Ko)`` over the output voxels that
    can reach it.  The float64 coordinates are binned per input cell and the 3 x 3 x 3 box sum credits every cell to the voxels
    around it.  The cell is the NEAREST voxel ``r``, not the floor: a coordinate ``x`` has its taps at ``floor(x)`` and
    ``floor(x) + 1``, both within ``r - 1 .. r + 1``, and they stay there when a float32 chain puts ``x`` on the other side of an
    integer (binned by the floor ``c``, a float32 coordinate just past ``c + 1`` has a tap at ``c + 2``, outside the box: seen
    as a contribution of 5e-9 at a voxel that "nothing can reach").  *taps_only*: the eight taps of the float64 coordinate
    itself (cells ``floor(x)`` and ``floor(x) + 1``) instead — where a contribution of some weight goes, not an upper bound."""
    batch, channels = per_output.shape[:2]
    i, j, k = geo["in_shape"]
    device = per_output.device
    cells = torch.floor(coordinates64(geo, batch, device) + (0.0 if taps_only else 0.5)).to(torch.int64)  # (B, Io, Jo, Ko, 3)
    sums = torch.zeros(batch, channels, i, j, k, dtype=torch.float64, device=device)
    padded = (i + 2) * (j + 2) * (k + 2)

    def box(histogram):  # 3 x 3 x 3 sums of the padded histogram, one axis at a time (taps only: voxel v collects cells v - 1 and v)
        histogram = histogram.reshape(i + 2, j + 2, k + 2)
        histogram = histogram[:-2] + histogram[1:-1] + (0 if taps_only else histogram[2:])
        histogram = histogram[:, :-2] + histogram[:, 1:-1] + (0 if taps_only else histogram[:, 2:])
        return histogram[:, :, :-2] + histogram[:, :, 1:-1] + (0 if taps_only else histogram[:, :, 2:])

    for b in range(batch):
        ci, cj, ck = cells[b, ..., 0].reshape(-1), cells[b, ..., 1].reshape(-1), cells[b, ..., 2].reshape(-1)
        inside = (ci >= -1) & (ci <= i) & (cj >= -1) & (cj <= j) & (ck >= -1) & (ck <= k)
        index = (((ci + 1) * (j + 2) + (cj + 1)) * (k + 2) + (ck + 1))[inside]
        for c in range(channels):
            sums[b, c] = box(torch.bincount(index, weights=per_output[b, c].reshape(-1).double()[inside], minlength=padded))
    return sums


def scatter_bound(geo: dict, grad: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(N, G)``, both ``(B, C, I, J, K)`` float64 on the gradient's device: upper bounds of the number of output voxels that add
    into an input voxel and of the sum of the magnitudes they add (``reach`` of ones and of ``|g|``).  Weights are taken as 1,
    gated-out voxels as present: upper bounds both."""
    counts = reach(geo, torch.ones_like(grad[:, :1]))
    return counts.expand(grad.shape[0], grad.shape[1], *geo["in_shape"]), reach(geo, grad.abs())


def order_tolerance(geo: dict, grad: torch.Tensor) -> torch.Tensor:
    """``2 (N_v + 1) u G_v``: two float32 sums of the same ``<= N_v`` rounded products, each within ``(N_v + 1) u G_v`` of the
    exact sum of those products (see ``check_against_dense``), differ by at most twice that."""
    counts, sums = scatter_bound(geo, grad)
    return 2 * (counts + 1) * U * sums


def assert_within(actual: torch.Tensor, expected: torch.Tensor, tolerance: torch.Tensor, what: str) -> float:
    """Every voxel within its tolerance; returns the largest error / tolerance seen (0 where both are 0)."""
    error = (actual.double() - expected.double()).abs()
    tolerance = tolerance.to(error.device)
    bad = int((error > tolerance).sum())
    ratio = torch.where(tolerance > 0, error / tolerance, torch.zeros_like(error))
    assert bad == 0, f"{what}: {bad} of {error.numel()} voxels beyond their tolerance, the largest error among them {float(error[error > tolerance].max()):.3g}"
    return float(ratio.max())


def dot_product_gap(geo: dict, data: torch.Tensor, grad: torch.Tensor, forward_linear: torch.Tensor, result: torch.Tensor) -> tuple[float, float]:
    """``|<A x, g> - <x, A^T g>|`` in float64 and its rounding bound.  *forward_linear* is the linear part of the forward (with a
    non-zero fill: minus the forward of the zero volume).  Each output voxel is a float32 sum of 8 rounded products of weights
    that add up to at most ``1 + 3u``: within ``9 u max|x|``; each input voxel of the adjoint within ``(N_v + 1) u G_v``."""
    lhs = (forward_linear.double() * grad.double()).sum()
    rhs = (data.double() * result.double()).sum()
    counts, sums = scatter_bound(geo, grad)
    bound = 9 * U * float(data.abs().max()) * grad.double().abs().sum() + (data.double().abs() * (counts + 1) * U * sums).sum()
    return float((lhs - rhs).abs()), float(bound)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the independent reference: float64 autograd through grid_sample
# ---------------------------------------------------------------------------------------------------------------------
def aten_reference_adjoint(geo: dict, grad: torch.Tensor, fill, device) -> tuple[torch.Tensor, torch.Tensor | None]:
    """``d <resample(x), grad> / dx`` as the reference's autograd computes it, in float64: the float32 grid of
    ``aten_pipeline._grid`` (built on the host, like the reference builds it for a host subject) cast to float64,
    ``F.grid_sample`` + the ones-mask ``torch.where`` (``aten_pipeline.resample``), ``torch.autograd.grad``.  Covers what
    ``_grid`` covers: equal shapes, unit spacing, the affine composed first.  Second result: with a fill, the output voxels
    ``(B, 1, I, J, K)`` that kept their value (``mask > 0.5`` in float64)."""
    assert geo["in_shape"] == geo["out_shape"] and geo["affine_first"] and geo["norm_shape"] is None
    assert tuple(geo["in_spacing"]) == (1, 1, 1) and geo["cp_skip"] is None and geo["passthrough"] is None
    batch, channels = grad.shape[:2]
    mapping, control = geo["mapping"].cpu(), geo["control_points"]
    grids = torch.stack([
        _grid(geo["in_shape"], mapping[b if mapping.shape[0] > 1 else 0], None if control is None else control[b if control.shape[0] > 1 else 0].cpu(), "cpu")
        for b in range(batch)
    ]).to(device=device, dtype=torch.float64).permute(0, 3, 2, 1, 4)
    kept = None
    with torch.enable_grad():
        leaf = torch.zeros((batch, channels, *geo["in_shape"]), dtype=torch.float64, device=device).requires_grad_(True)
        volume = leaf.permute(0, 1, 4, 3, 2)
        out = F.grid_sample(volume, grids, mode="bilinear", padding_mode="zeros", align_corners=True)
        if fill is not None:
            mask = F.grid_sample(torch.ones_like(volume[:, :1]).detach(), grids, mode="bilinear", padding_mode="zeros", align_corners=True)
            out = torch.where(mask > 0.5, out, fill.to(device=device, dtype=torch.float64).view(1, -1, 1, 1, 1))
            kept = (mask > 0.5).permute(0, 1, 4, 3, 2)
        out = out.permute(0, 1, 4, 3, 2)
        (result,) = torch.autograd.grad(out, leaf, grad.to(device=device, dtype=torch.float64))
    return result, kept


def flipped_gates(engine, geo: dict, batch: int, kept64: torch.Tensor) -> torch.Tensor:
    """Input voxels ``(B, 1, I, J, K)`` (bool, on ``kept64``'s device) that are taps of an output voxel whose fill gate fell
    differently in the float32 chain than in float64 (an in-bounds weight within coordinate rounding of 1/2).  The float32
    decision is read off *engine*'s FORWARD — the zero volume with fill 1 comes out 1 exactly where the fill was taken —,
    never off an adjoint under test.  At such voxels a float32 adjoint and the float64 reference differ by a whole
    contribution ``g w``: they are left out of the comparison with that reference (and of no other).  (A tap that the float32
    chain has on the other side of a cell border carries a weight of the size of the coordinate's rounding: that stays within
    ``coordinate_rounding_bound``.)"""
    device = geo["mapping"].device
    taken = forward(engine, torch.zeros((batch, 1, *geo["in_shape"]), device=device), geo, torch.ones(1, device=device)) == 1
    flipped = taken.to(kept64.device) == kept64
    return reach(on_device(geo, kept64.device), flipped.double(), taps_only=True) > 0


def coordinate_rounding_bound(geo: dict, grad: torch.Tensor) -> torch.Tensor:
    """How far a float32 adjoint may be from the float64 reference at an input voxel whose gates agree: ``60 u c G_v + (N_v + 1)
    u G_v`` with ``c`` the largest coordinate magnitude (the extent).  A float32 sampling coordinate is the end of about ten
    roundings of intermediates no larger than ``c`` (affine row: 4, displacement: 1 + the control grid's blend at a much smaller
    magnitude, normalise and un-normalise: 4), the reference's own float32 grid of as many: the two differ by ``d <= 20 u c``.
    A tap weight is a product of three factors that each move by ``d``: ``|dw| <= 3 d``; a voxel collects ``sum |g| |dw| <= 3 d
    G_v``; the order of the additions adds ``(N_v + 1) u G_v``."""
    counts, sums = scatter_bound(geo, grad)
    return (60 * U * float(max(geo["in_shape"])) + (counts + 1) * U) * sums


def deviation(candidate: torch.Tensor, reference: torch.Tensor, leave_out: torch.Tensor | None = None) -> float:
    """max |candidate - reference| / max |reference|, the maximum over the voxels that are not in *leave_out*"""
    error = (candidate.double().to(reference.device) - reference).abs()
    if leave_out is not None:
        error = error.masked_fill(leave_out.expand_as(error), 0.0)
    return float(error.max() / reference.abs().max())
