"""Cases and the float64 numpy reference of the annotation tests (``test_points_reference_host.py``, ``test_gpu_points_warp.py``,
``test_gpu_annotations_transforms.py``, ``test_gpu_points_guarded.py``).

The reference restates the sampling map of the reference implementation (spatial.py:1570-1577, 2171-2189) and the solver
``include/tio_hip.h`` specifies for ``tio_points_warp``, independently of the kernel, in plain numpy:

    affine_first:  s(o) = M o + d(o) / spacing_in          otherwise:  s(o) = M (o + d(o) / spacing_out)

``d`` the trilinear interpolation of the ``(n_i, n_j, n_k, 3)`` control points at ``o_a (n_a - 1) / max(S_a - 1, 1)``, the index
clamped to ``[0, n_a - 1]``; Newton from the affine-only answer, the step halved while ``max|s(o) - p|`` does not decrease,
until that residual is at most ``TOLERANCE`` or ``MAX_ITERATIONS`` steps were taken; a converged point then takes one more
full step, kept when it lowers the residual (the stop alone leaves anything up to ``TOLERANCE``).
"""
from __future__ import annotations

import numpy as np
import torch

TOLERANCE = 1.0e-7
MAX_ITERATIONS = 50
MAX_HALVINGS = 30
BLOCK_DOUBLES = 40

# the smallest shapes at which axis or spacing mix-ups show: nothing cubic, nothing isotropic
OUT_SHAPE = (11, 24, 17)
IN_SHAPE = (13, 19, 23)
GRID = (5, 7, 6)
IN_SPACING = (0.8, 1.0, 2.5)
OUT_SPACING = (1.2, 0.9, 2.0)
COUNTS = (0, 1, 257)  # an empty element, one point, one point more than a block


class Map:
    """One element's sampling map."""

    def __init__(self, matrix, out_shape=(1, 1, 1), in_spacing=(1.0, 1.0, 1.0), out_spacing=(1.0, 1.0, 1.0), affine_first=True, field=None):
        self.matrix = np.asarray(matrix, dtype=np.float64)
        if self.matrix.shape == (3, 4):
            self.matrix = np.vstack([self.matrix, [0.0, 0.0, 0.0, 1.0]])
        self.inverse = np.linalg.inv(self.matrix)
        self.out_shape = tuple(int(s) for s in out_shape)
        self.in_spacing = np.asarray(in_spacing, dtype=np.float64)
        self.out_spacing = np.asarray(out_spacing, dtype=np.float64)
        self.affine_first = bool(affine_first)
        self.field = None if field is None else np.asarray(field, dtype=np.float32)

    def block(self, cp_offset: int = -1) -> np.ndarray:
        """The element's parameter block as ``include/tio_hip.h`` lays it out."""
        block = np.zeros(BLOCK_DOUBLES)
        block[0:12] = self.matrix[:3].reshape(-1)
        block[12:24] = self.inverse[:3].reshape(-1)
        block[24:27] = self.out_shape
        block[27:30] = self.in_spacing
        block[30:33] = self.out_spacing
        block[33] = 1.0 if self.affine_first else 0.0
        if self.field is not None:
            block[34:37] = self.field.shape[:3]
        block[37] = cp_offset if self.field is not None else -1
        return block


def apply34(matrix: np.ndarray, v: np.ndarray) -> np.ndarray:
    return v @ matrix[:3, :3].T + matrix[:3, 3]


def displacement(m: Map, o: np.ndarray):
    """``d(o)`` in mm, ``(N, 3)``, and ``D[n, c, a] = d d_c / d o_a``."""
    field = m.field.astype(np.float64)
    n = np.asarray(field.shape[:3])
    scale = (n - 1) / np.maximum(np.asarray(m.out_shape, dtype=np.float64) - 1.0, 1.0)
    raw = o * scale
    inside = (raw >= 0.0) & (raw <= n - 1)
    u = np.clip(np.where(np.isnan(raw), 0.0, raw), 0.0, n - 1)
    lo = np.clip(np.floor(u).astype(np.int64), 0, np.maximum(n - 2, 0))
    hi = np.minimum(lo + 1, n - 1)
    t = u - lo
    slope = np.where(inside, scale, 0.0)
    corner = {}
    for x in (0, 1):
        for y in (0, 1):
            for z in (0, 1):
                corner[x, y, z] = field[(hi if x else lo)[:, 0], (hi if y else lo)[:, 1], (hi if z else lo)[:, 2]]  # (N, 3)
    w = [np.stack([1.0 - t[:, a], t[:, a]])[:, :, None] for a in range(3)]  # w[a][side]: (N, 1)
    vk = {(x, y): corner[x, y, 0] * w[2][0] + corner[x, y, 1] * w[2][1] for x in (0, 1) for y in (0, 1)}
    dk = {(x, y): corner[x, y, 1] - corner[x, y, 0] for x in (0, 1) for y in (0, 1)}
    vj = {x: vk[x, 0] * w[1][0] + vk[x, 1] * w[1][1] for x in (0, 1)}
    dj = {x: vk[x, 1] - vk[x, 0] for x in (0, 1)}
    dkj = {x: dk[x, 0] * w[1][0] + dk[x, 1] * w[1][1] for x in (0, 1)}
    d = vj[0] * w[0][0] + vj[1] * w[0][1]
    derivative = np.stack([vj[1] - vj[0], dj[0] * w[0][0] + dj[1] * w[0][1], dkj[0] * w[0][0] + dkj[1] * w[0][1]], axis=2)  # (N, c, a)
    return d, derivative * slope[:, None, :]


def s_ref(m: Map, o: np.ndarray):
    """``s(o)`` ``(N, 3)`` and its Jacobian ``(N, 3, 3)`` in float64."""
    o = np.asarray(o, dtype=np.float64)
    linear = m.matrix[:3, :3]
    if m.field is None:
        return apply34(m.matrix, o), np.broadcast_to(linear, (o.shape[0], 3, 3)).copy()
    d, derivative = displacement(m, o)
    if m.affine_first:
        return apply34(m.matrix, o) + d / m.in_spacing, linear + derivative / m.in_spacing[:, None]
    inner = np.eye(3) + derivative / m.out_spacing[:, None]
    return apply34(m.matrix, o + d / m.out_spacing), linear @ inner


def solve_ref(m: Map, p: np.ndarray):
    """``o`` with ``s(o) = p`` ``(N, 3)`` float64 and the status ``(N,)``: 0 converged, 1 not."""
    p = np.asarray(p, dtype=np.float64)
    o = apply34(m.inverse, p)
    status = np.zeros(p.shape[0], dtype=np.int8)
    if m.field is None or p.shape[0] == 0:
        return o, status
    s, jacobian = s_ref(m, o)
    err = np.abs(s - p).max(axis=1)
    active = ~(err <= TOLERANCE)
    for _ in range(MAX_ITERATIONS):
        if not active.any():
            break
        rows = np.flatnonzero(active)
        with np.errstate(all="ignore"):
            try:
                step = np.linalg.solve(jacobian[rows], (s[rows] - p[rows])[:, :, None])[:, :, 0]
            except np.linalg.LinAlgError:
                break
        step_scale = np.ones(rows.shape[0])
        pending = np.ones(rows.shape[0], dtype=bool)
        for _ in range(MAX_HALVINGS):
            if not pending.any():
                break
            sub = rows[pending]
            trial = o[sub] - step_scale[pending, None] * step[pending]
            st, jt = s_ref(m, trial)
            et = np.abs(st - p[sub]).max(axis=1)
            better = et < err[sub]
            accepted = sub[better]
            o[accepted], s[accepted], jacobian[accepted], err[accepted] = trial[better], st[better], jt[better], et[better]
            where = np.flatnonzero(pending)
            pending[where[better]] = False
            step_scale[pending] *= 0.5
        active[rows[pending]] = False  # stalled: the best iterate stays, status 1
        status[rows[pending]] = 1
        active &= ~(err <= TOLERANCE)
    status[active] = 1
    status[err <= TOLERANCE] = 0
    # the stop decides the status; one more full step from a converged iterate, kept where it lowers the residual
    rows = np.flatnonzero((status == 0) & (err > 0.0))
    if rows.size:
        with np.errstate(all="ignore"):
            try:
                step = np.linalg.solve(jacobian[rows], (s[rows] - p[rows])[:, :, None])[:, :, 0]
            except np.linalg.LinAlgError:
                return o, status
        trial = o[rows] - step
        better = np.abs(s_ref(m, trial)[0] - p[rows]).max(axis=1) < err[rows]
        o[rows[better]] = trial[better]
    return o, status


def jacobian_bound(m: Map) -> float:
    """An upper bound on the infinity norm of the Jacobian of ``s`` anywhere: ``M`` and the control field's finite differences
    (the trilinear cell's partial derivatives are convex combinations of its edges' differences)."""
    linear = np.abs(m.matrix[:3, :3])
    if m.field is None:
        return float(linear.sum(axis=1).max())
    field = m.field.astype(np.float64)
    n = np.asarray(field.shape[:3])
    scale = (n - 1) / np.maximum(np.asarray(m.out_shape, dtype=np.float64) - 1.0, 1.0)
    growth = np.zeros((3, 3))  # growth[c, a] >= |d d_c / d o_a|
    for axis in range(3):
        if n[axis] > 1:
            growth[:, axis] = np.abs(np.diff(field, axis=axis)).reshape(-1, 3).max(axis=0) * scale[axis]
    if m.affine_first:
        return float((linear + growth / m.in_spacing[:, None]).sum(axis=1).max())
    return float((linear @ (np.eye(3) + growth / m.out_spacing[:, None])).sum(axis=1).max())


# -- the maps of recorded Spatial parameters ----------------------------------------------------------------------------------
def spatial_maps(params, in_affine, out_shape, out_affine, batch):
    """One ``Map`` (or ``None``: element left alone) per batch element from a recorded params dict."""
    batched = "affine_matrix" in (params.get("_batched_keys") or [])
    matrices = params["affine_matrix"] if batched else [params["affine_matrix"]] * batch
    fields = params["control_points"] if batched else [params["control_points"]] * batch
    maps = []
    for matrix, field in zip(matrices, fields, strict=True):
        if batched and params["target"] is None and matrix is None and field is None:
            maps.append(None)
            continue
        world = np.eye(4) if matrix is None else np.linalg.inv(np.asarray(matrix, dtype=np.float64))
        voxel = np.linalg.inv(in_affine.numpy()) @ world @ out_affine.numpy()
        maps.append(Map(voxel, out_shape, in_affine.spacing, out_affine.spacing, params["affine_first"],
                              None if field is None else np.asarray(field, dtype=np.float32)))
    return maps


# -- cases ----------------------------------------------------------------------------------------------------------------
def rotation(degrees) -> np.ndarray:
    a, b, c = np.radians(degrees)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def oblique_affine(spacing, degrees, origin) -> np.ndarray:
    matrix = np.eye(4)
    matrix[:3, :3] = rotation(degrees) * np.asarray(spacing, dtype=np.float64)
    matrix[:3, 3] = origin
    return matrix


IN_AFFINE = oblique_affine(IN_SPACING, (7.0, -11.0, 4.0), (-9.0, 5.0, 12.0))
OUT_AFFINE = oblique_affine(OUT_SPACING, (-5.0, 3.0, 9.0), (-7.0, 6.5, 10.0))


def world_transform(seed: int) -> np.ndarray:
    """A world-space affine as ``Affine`` would draw it: rotation, anisotropic scale, translation about a centre."""
    rng = np.random.default_rng(seed)
    matrix = np.eye(4)
    matrix[:3, :3] = rotation(rng.uniform(-15, 15, 3)) @ np.diag(rng.uniform(0.85, 1.2, 3))
    matrix[:3, 3] = rng.uniform(-3, 3, 3)
    return matrix


def voxel_matrix(seed: int | None) -> np.ndarray:
    """``inv(A_in) inv(T) A_out`` of the oblique grids above."""
    world = np.eye(4) if seed is None else np.linalg.inv(world_transform(seed))
    return np.linalg.inv(IN_AFFINE) @ world @ OUT_AFFINE


def folding_bound() -> np.ndarray:
    """The displacement per axis (mm) beyond which the reference warns of folding (spatial.py:2192-2225): half the spacing of
    the control grid's interior, ``extent / (n - 3)``."""
    extent = np.asarray(OUT_SHAPE, dtype=np.float64) * np.asarray(OUT_SPACING)
    return extent / (np.asarray(GRID) - 3.0) / 2.0


def control_field(seed: int, limit_mm) -> np.ndarray:
    """``GRID`` control points uniform in ``[-limit, limit]`` mm per axis, float32."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (*GRID, 3)) * np.asarray(limit_mm, dtype=np.float64)).astype(np.float32)


def gentle_limit() -> np.ndarray:
    """Regime (a): at most 1/8 of a coarse cell per axis, in mm of the space the displacement is divided by.  A cell spans
    ``(S - 1) / (n - 1)`` output voxels; in voxel units ``|d d_c / d o_a| <= 2 * limit_c / cell_a``, so each row of ``grad d``
    sums to at most ``3 * 2 / 8 < 1``: ``I + grad d`` is strictly diagonally dominant and the map injective."""
    cell = (np.asarray(OUT_SHAPE) - 1.0) / (np.asarray(GRID) - 1.0)
    return cell.min() / 8.0 * np.minimum(np.asarray(IN_SPACING), np.asarray(OUT_SPACING))


def elastic_map(regime: str, affine_first: bool, seed: int) -> Map:
    limit = gentle_limit() if regime == "gentle" else folding_bound() / 2.0
    return Map(voxel_matrix(seed), OUT_SHAPE, IN_SPACING, OUT_SPACING, affine_first, control_field(seed, limit))


def points_for(m: Map, count: int, seed: int) -> np.ndarray:
    """*count* float32 input-voxel points whose pre-images spread over the output grid, every third one outside the field of
    view (by up to half the grid's extent)."""
    rng = np.random.default_rng(seed)
    shape = np.asarray(m.out_shape, dtype=np.float64)
    o = rng.uniform(0.0, 1.0, (count, 3)) * (shape - 1.0)
    outside = np.arange(count) % 3 == 2
    push = np.where(rng.uniform(size=(count, 3)) < 0.5, -1.0, 1.0) * rng.uniform(0.05, 0.5, (count, 3)) * shape
    axis = rng.integers(0, 3, count)
    mask = np.zeros((count, 3), dtype=bool)
    mask[np.arange(count), axis] = True
    o = np.where(outside[:, None] & mask, np.where(push < 0, push, shape - 1.0 + push), o)
    return s_ref(m, o)[0].astype(np.float32)


def ragged(maps, counts=COUNTS, seed: int = 0):
    """``(points (N, 3) float32, offsets (B + 1,) int32, blocks (B, 40) float64, control points float32 or None)``."""
    pieces, blocks, fields, used = [], [], [], 0
    for index, (m, count) in enumerate(zip(maps, counts, strict=True)):
        pieces.append(points_for(m, count, seed + index))
        blocks.append(m.block(used))
        if m.field is not None:
            fields.append(m.field.reshape(-1))
            used += m.field.size
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    control = np.concatenate(fields) if fields else None
    return np.concatenate(pieces), offsets, np.stack(blocks), control


def warp_on_gpu(engine, points, offsets, blocks, control, return_status=True):
    out = engine.warp_points(
        torch.from_numpy(points).cuda(), torch.from_numpy(offsets), torch.from_numpy(blocks),
        None if control is None else torch.from_numpy(control), return_status=return_status,
    )
    if return_status:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def elastic_bar(m: Map, o_gpu: np.ndarray) -> float:
    """``1e-6 + 4 spacing(float32(max|coord|)) Jn``: the rounding of the float32 output carried through ``s``, over the
    solver's stop."""
    largest = np.float32(np.abs(o_gpu).max()) if o_gpu.size else np.float32(1.0)
    return 1e-6 + 4.0 * float(np.spacing(largest)) * jacobian_bound(m)
