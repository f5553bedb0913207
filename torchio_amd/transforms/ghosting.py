"""``Ghosting`` on the HIP engine (mirror of reference ``transforms/intensity/ghosting.py``).

The reference transforms the whole volume to k-space, scales every ``step``-th plane along one axis by ``1 - intensity``,
restores a central window and transforms back: two complex 3-D FFTs, two shifts and a mask product per image.  Only planes
along ONE axis are touched, so the other two axes' transforms cancel and each line along the axis loses a handful of its
Fourier components: ``tio_kspace_ghost_lines`` does that with one reduction and one update per line
(``csrc/kspace_artefacts.hip``).  Same constructor, draw order, parameter dictionary and warning; ``make_params`` reads
nothing of the data.
"""
from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .. import ops
from ..data.batch import SubjectsBatch
from .parameter_range import to_nonneg_range
from .transform import IntensityTransform


class Ghosting(IntensityTransform):
    """Ghost replicas of the anatomy along one axis (ghosting.py:16-146).

    ``num_ghosts``: the number of replicas or a ``(a, b)`` range of it; ``axes``: the axes one is drawn from; ``intensity``:
    the artefact's strength or a range (the default 0 does nothing, and warns); ``restore``: the fraction of central k-space
    left alone.  Unlike the reference's, the cost grows with the number of scaled planes.  Not invertible.
    """

    def __init__(
        self,
        *,
        num_ghosts: int | tuple[int, int] = 4,
        axes: tuple[int, ...] = (0, 1, 2),
        intensity: float | tuple[float, float] = 0.0,
        restore: float | None = None,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        self.num_ghosts = to_nonneg_range(num_ghosts)
        self.axes = axes
        self.intensity = to_nonneg_range(intensity)
        self.restore = restore
        self._warn_if_noop(is_noop=self.intensity.is_constant(0.0) or self.num_ghosts.is_constant(0.0), hint="intensity=(0.5, 1)")

    @property
    def supports_per_instance_params(self) -> bool:
        return True

    @property
    def supports_per_instance_p(self) -> bool:
        return True

    def _draw_one(self) -> tuple[int, int, float]:
        """The count, the axis, the strength — in this order (ghosting.py:77-82, :95-97)."""
        num_ghosts = max(1, round(self.num_ghosts.sample_1d()))
        axis = self.axes[int(torch.randint(len(self.axes), (1,)).item())]
        return num_ghosts, axis, self.intensity.sample_1d()

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        restore = self.restore if self.restore is not None else 0.0
        n = self._resolve_n(batch)
        if n is None:
            num_ghosts, axis, intensity = self._draw_one()
            return {"num_ghosts": num_ghosts, "axis": axis, "intensity": intensity, "restore": restore}
        keep = self._keep_mask(batch, n)
        drawn = [(0, self.axes[0], 0.0) if keep is not None and not keep[index] else self._draw_one() for index in range(n)]
        params = {
            "num_ghosts": [d[0] for d in drawn],
            "axis": [d[1] for d in drawn],
            "intensity": [d[2] for d in drawn],
            "restore": restore,
        }
        self._tag_batched(params, batch, n, keep, ["num_ghosts", "axis", "intensity"])
        return params

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        restore = params["restore"]
        if self._is_per_instance_params(params):
            elements = list(zip(params["num_ghosts"], params["axis"], params["intensity"], strict=True))
        else:
            elements = [(params["num_ghosts"], params["axis"], params["intensity"])]
        if not any(ghosts and strength != 0 for ghosts, _, strength in elements):
            return batch  # nothing active: every image stays the object it was
        for img_batch in self._get_images(batch).values():
            data = img_batch.data  # (pending lazy work is carried out here)
            shape = data.shape[2:]
            entries = elements if len(elements) > 1 or data.shape[0] == 1 else elements * data.shape[0]
            axes, strengths, lists = [], [], []
            for ghosts, axis, strength in entries:
                on = bool(ghosts) and strength != 0
                axes.append(axis)
                strengths.append(_mask_strength(strength) if on else 0.0)
                lists.append(ghost_frequencies(int(shape[axis]), ghosts, restore) if on else [])
            img_batch.data = ops.engine().ghost_lines(data, axes, strengths, lists)
        return batch


def _mask_strength(strength: float) -> float:
    """The reference stores ``1 - strength`` in a float32 mask; what the planes lose is one minus THAT."""
    return 1.0 - float(np.float32(1.0 - strength))


def ghost_line_mask(size: int, num_ghosts: int, restore: float) -> np.ndarray:
    """True where the reference's line mask differs from 1 (ghosting.py:189-197, :250-271), by SHIFTED index: every
    ``step``-th plane from 0, minus the window ``[mid - half, mid + half)`` — a Python slice, so a start below zero counts
    from the end, as it does in the reference."""
    scaled = np.zeros(size, dtype=bool)
    step = max(size // num_ghosts, 1)
    scaled[::step] = True
    if restore > 0:
        mid = size // 2
        half_restore = max(int(size * restore / 2), 1)
        scaled[mid - half_restore : mid + half_restore] = False
    return scaled


def ghost_frequencies(size: int, num_ghosts: int, restore: float) -> list[int]:
    """The scaled planes as UNSHIFTED frequencies: shifted index ``u`` is frequency ``(u - size // 2) mod size``."""
    shifted = np.nonzero(ghost_line_mask(size, num_ghosts, restore))[0]
    return [int(f) for f in (shifted - size // 2) % size]
