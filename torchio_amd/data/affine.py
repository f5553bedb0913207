"""Voxel-to-world affine (mirror of reference ``src/torchio/data/affine.py:20-248``).

Only what the augmentation hot path touches: a float64 4x4 on the host side,
``spacing`` / ``origin`` / ``direction`` and conversion helpers.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor


class AffineMatrix:
    """4x4 float64 matrix mapping voxel indices to world (mm) coordinates."""

    __slots__ = ("_matrix", "_spacing_cache", "_bytes_cache", "_inverse_cache")

    def __init__(self, matrix=None) -> None:
        if matrix is None:
            value = torch.eye(4, dtype=torch.float64)
        elif isinstance(matrix, AffineMatrix):
            value = matrix._matrix.clone()
        elif isinstance(matrix, Tensor):
            value = matrix.detach().to(torch.float64).clone()
        else:
            value = torch.from_numpy(np.array(matrix, dtype=np.float64, copy=True))
        if tuple(value.shape) != (4, 4):
            raise ValueError(f"AffineMatrix must be 4x4, got {tuple(value.shape)}")
        self._matrix = value
        self._spacing_cache = None  # (tensor version, spacing): the 4x4 may be edited in place through .data
        self._bytes_cache = None    # (tensor version, the 128 bytes of the matrix): `same_values`
        self._inverse_cache = None  # (tensor version, np.linalg.inv of the matrix): `inverse_numpy`

    @classmethod
    def from_spacing(cls, spacing, *, origin=(0.0, 0.0, 0.0), direction=None) -> "AffineMatrix":
        matrix = torch.eye(4, dtype=torch.float64)
        if direction is not None:
            matrix[:3, :3] = torch.as_tensor(np.asarray(direction, dtype=np.float64))
        matrix[:3, :3] *= torch.as_tensor(spacing, dtype=torch.float64)
        matrix[:3, 3] = torch.as_tensor(origin, dtype=torch.float64)
        return cls(matrix)

    @property
    def data(self) -> Tensor:
        return self._matrix

    @property
    def device(self) -> torch.device:
        return self._matrix.device

    def _column_norms(self) -> Tensor:
        return torch.sqrt(torch.sum(self._matrix[:3, :3] ** 2, dim=0))

    @property
    def spacing(self) -> tuple[float, float, float]:
        version = self._matrix._version
        cached = self._spacing_cache
        if cached is not None and cached[0] == version:
            return cached[1]
        norms = self._column_norms().tolist()  # (ATen's float64 reduction: numpy adds the three squares in another order)
        value = (float(norms[0]), float(norms[1]), float(norms[2]))
        self._spacing_cache = (version, value)
        return value

    @property
    def origin(self) -> tuple[float, float, float]:
        o = self._matrix[:3, 3]
        return (float(o[0]), float(o[1]), float(o[2]))

    @property
    def direction(self) -> Tensor:
        return self._matrix[:3, :3] / self._column_norms()

    @property
    def orientation(self) -> tuple[str, str, str]:
        """Anatomical orientation codes such as ``('R', 'A', 'S')`` (reference affine.py:124-128).

        The reference asks nibabel (``aff2axcodes``); this is the same published algorithm: the
        closest orthogonal matrix to the zoom-normalised direction block (SVD), then every voxel
        axis claims the world axis on which it has the largest absolute component, each world
        axis being claimed at most once.
        """
        block = self._matrix[:3, :3].cpu().numpy().astype(np.float64)
        zooms = np.sqrt(np.sum(block * block, axis=0))
        zooms[zooms == 0] = 1.0
        left, singular, right = np.linalg.svd(block / zooms)
        keep = singular > singular.max() * 3 * np.finfo(singular.dtype).eps
        rotation = left[:, keep] @ right[keep]
        labels = (("L", "R"), ("P", "A"), ("I", "S"))
        codes: list[str] = []
        for axis in range(3):
            column = rotation[:, axis]
            if np.allclose(column, 0):
                codes.append(None)  # type: ignore[arg-type]
                continue
            world = int(np.argmax(np.abs(column)))
            codes.append(labels[world][0 if column[world] < 0 else 1])
            rotation[world, :] = 0  # a world axis is assigned once
        return (codes[0], codes[1], codes[2])

    def _value_bytes(self) -> bytes:
        version = self._matrix._version
        cached = self._bytes_cache
        if cached is not None and cached[0] == version:
            return cached[1]
        value = self._matrix.numpy().tobytes()
        self._bytes_cache = (version, value)
        return value

    def same_values(self, other: "AffineMatrix") -> bool:
        """``torch.equal(self.data, other.data)`` for host matrices (NaN-free grids: byte equality, except that +0.0 and
        -0.0 compare unequal here — callers fall back to the tensor comparison on ``False``); cached per tensor version."""
        return self is other or self._value_bytes() == other._value_bytes()

    def inverse_numpy(self) -> np.ndarray:
        """``np.linalg.inv(self.numpy())`` (read-only; cached per tensor version: the same grid is inverted by every
        spatial transform of a pipeline)."""
        version = self._matrix._version
        cached = self._inverse_cache
        if cached is not None and cached[0] == version:
            return cached[1]
        value = np.linalg.inv(self._matrix.numpy())
        value.setflags(write=False)
        self._inverse_cache = (version, value)
        return value

    def to(self, *args, **kwargs) -> "AffineMatrix":
        """Affines stay float64 and — unlike image data — on the host.

        The reference moves the 4x4 along with the data (affine.py ``to``); every
        consumer on the hot path immediately reads it back with ``float()`` /
        ``.numpy()`` (spatial.py:1594, affine.py:104-109), i.e. one device sync
        per access.  Keeping it on the CPU removes those syncs and changes no
        value.
        """
        return self

    def clone(self) -> "AffineMatrix":
        new = AffineMatrix.__new__(AffineMatrix)
        new._matrix = self._matrix.clone()
        # The copy inherits what is cached for these values.  The spacing is worked out HERE if nobody asked the source yet:
        # a pipeline copies its input batch every step and asks the COPIES (four tensor ops per element and step, for ever);
        # asked once of the source, every later copy starts with the answer.
        if self._spacing_cache is None or self._spacing_cache[0] != self._matrix._version:
            self.spacing  # noqa: B018 - fills the cache
        cached = self._spacing_cache
        # the copy starts at tensor version 0 with the same values: the spacing carries over
        version = self._matrix._version
        new._spacing_cache = (0, cached[1]) if cached is not None and cached[0] == version else None
        cached = self._bytes_cache
        new._bytes_cache = (0, cached[1]) if cached is not None and cached[0] == version else None
        cached = self._inverse_cache
        new._inverse_cache = (0, cached[1]) if cached is not None and cached[0] == version else None
        return new

    def inverse(self) -> "AffineMatrix":
        return AffineMatrix(torch.linalg.inv(self._matrix))

    def compose(self, other: "AffineMatrix") -> "AffineMatrix":
        """``self @ other`` as a new ``AffineMatrix`` (reference affine.py:178-183)."""
        return AffineMatrix(self._matrix @ other._matrix)

    def apply(self, points) -> Tensor:
        """Map an ``(N, 3)`` set of points through the affine, in float64 (reference affine.py:185-205)."""
        if not isinstance(points, Tensor):
            pts = torch.as_tensor(np.asarray(points, dtype=np.float64), dtype=torch.float64)
        else:
            pts = points.to(torch.float64)
        pts = pts.to(self._matrix.device)
        homogeneous = torch.cat([pts, torch.ones(pts.shape[0], 1, dtype=torch.float64, device=pts.device)], dim=1)
        return (self._matrix @ homogeneous.T).T[:, :3]

    def numpy(self) -> np.ndarray:
        return self._matrix.cpu().numpy()

    def __matmul__(self, other):
        if not isinstance(other, AffineMatrix):
            return NotImplemented
        return AffineMatrix(self._matrix @ other._matrix)

    def __array__(self, dtype=None, copy=None):
        array = self.numpy()
        return array.astype(dtype) if dtype is not None else (array.copy() if copy else array)

    def __eq__(self, other) -> bool:
        if not isinstance(other, AffineMatrix):
            return NotImplemented
        return torch.equal(self._matrix, other._matrix)

    def __hash__(self):  # pragma: no cover - identity hash like the reference's default
        return id(self)

    def __copy__(self):
        return self.clone()

    def __deepcopy__(self, memo):
        new = self.clone()
        memo[id(self)] = new
        return new

    def __repr__(self) -> str:
        sp = ", ".join(f"{s:.2f}" for s in self.spacing)
        o = ", ".join(f"{v:.2f}" for v in self.origin)
        return f"AffineMatrix(spacing=({sp}), origin=({o}))"


# -- orientation algebra ------------------------------------------------------------------------------------------------
# The four nibabel functions ``Reorient`` calls (reference transforms/spatial/reorient.py:48-60, :161), restated from the
# published algorithms like ``AffineMatrix.orientation`` above.  An "ornt" is a (3, 2) float array: row = voxel axis,
# column 0 = the world (or output) axis it is closest to, column 1 = +1 / -1 for the direction along it.
_AXIS_LABELS = (("L", "R"), ("P", "A"), ("I", "S"))


def io_orientation(affine) -> np.ndarray:
    """Orientation of the voxel axes of *affine* relative to world RAS+ (``nibabel.orientations.io_orientation``)."""
    block = np.asarray(affine, dtype=np.float64)[:3, :3]
    zooms = np.sqrt(np.sum(block * block, axis=0))
    zooms[zooms == 0] = 1.0
    left, singular, right = np.linalg.svd(block / zooms, full_matrices=False)
    keep = singular > singular.max() * 3 * np.finfo(singular.dtype).eps
    rotation = left[:, keep] @ right[keep]
    ornt = np.full((3, 2), np.nan)
    for axis in range(3):
        column = rotation[:, axis]
        if np.allclose(column, 0):
            continue
        world = int(np.argmax(np.abs(column)))
        ornt[axis] = (world, -1.0 if column[world] < 0 else 1.0)
        rotation[world, :] = 0  # a world axis is assigned once
    return ornt


def axcodes2ornt(axcodes) -> np.ndarray:
    """Orientation array of axis codes such as ``('L', 'P', 'S')`` (``nibabel.orientations.axcodes2ornt``)."""
    allowed = {code for pair in _AXIS_LABELS for code in pair} | {None}
    if not set(axcodes).issubset(allowed):
        raise ValueError(f"Not all axis codes {list(axcodes)} in label set {sorted(c for c in allowed if c)}")
    ornt = np.full((len(axcodes), 2), np.nan)
    for index, code in enumerate(axcodes):
        for world, pair in enumerate(_AXIS_LABELS):
            if code is not None and code in pair:
                ornt[index] = (world, -1.0 if code == pair[0] else 1.0)
                break
    return ornt


def ornt_transform(start_ornt, end_ornt) -> np.ndarray:
    """The orientation that takes an array in *start_ornt* to *end_ornt* (``nibabel.orientations.ornt_transform``):
    row = axis of the start array, column 0 = the axis of the end array it becomes, column 1 = -1 when it is reversed."""
    start_ornt, end_ornt = np.asarray(start_ornt), np.asarray(end_ornt)
    if start_ornt.shape != end_ornt.shape:
        raise ValueError("The orientations must have the same shape")
    if start_ornt.shape[1] != 2:
        raise ValueError(f"Invalid shape for an orientation: {start_ornt.shape}")
    result = np.empty_like(start_ornt)
    for end_axis, (end_world, end_flip) in enumerate(end_ornt):
        for start_axis, (start_world, start_flip) in enumerate(start_ornt):
            if end_world == start_world:
                result[start_axis] = (end_axis, 1 if start_flip == end_flip else -1)
                break
        else:
            raise ValueError(f"Unable to find out axis {end_world} in start_ornt")
    return result


def inv_ornt_aff(ornt, shape) -> np.ndarray:
    """The 4x4 that maps voxel indices of the REORIENTED array to indices of the array of *shape* it was made from
    (``nibabel.orientations.inv_ornt_aff``): undo the axis order, then undo the flips about the array centre."""
    ornt = np.asarray(ornt, dtype=np.float64)
    if np.any(np.isnan(ornt)):
        raise ValueError("We cannot invert orientation transformations that drop axes")
    size = ornt.shape[0]
    extent = np.array(shape, dtype=np.float64)[:size]
    undo_reorder = np.eye(size + 1)[[*ornt[:, 0].astype(int), size], :]
    undo_flip = np.diag([*ornt[:, 1], 1.0])
    centre = -(extent - 1) / 2.0
    undo_flip[:size, size] = ornt[:, 1] * centre - centre
    return undo_flip @ undo_reorder
