"""``Spike`` on the HIP engine (mirror of reference ``transforms/intensity/spike.py``).

The reference adds ``peak * intensity`` to a few points of the shifted spectrum and transforms back: two complex 3-D FFTs,
two shifts and an ``abs`` temporary per image.  A point of k-space is a plane wave in image space, so the result is the
image plus a sum of cosines: ``tio_kspace_add_spikes`` adds them in one pass (``csrc/kspace_artefacts.hip``).  Only the peak
of the spectrum needs a transform — ``Engine.spectrum_peak``, a half-spectrum FFT reduced on the device; the peak is
never read back.  Same constructor, draw order, parameter dictionary and warning; ``make_params`` reads nothing of the data.
"""
from __future__ import annotations

from typing import Any

import torch

from .. import ops
from ..data.batch import SubjectsBatch
from .parameter_range import to_nonneg_range
from .parameter_range import to_range
from .transform import IntensityTransform


class Spike(IntensityTransform):
    """Stripes from spikes in k-space, the herringbone artefact (spike.py:17-121).

    ``num_spikes``: the number of spikes or a ``(a, b)`` range of it; ``intensity``: the spike's amplitude over the
    spectrum's maximum, or a range (the default 0 does nothing, and warns).  Not invertible.
    """

    def __init__(self, *, num_spikes: int | tuple[int, int] = 1, intensity: float | tuple[float, float] = 0.0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.num_spikes = to_nonneg_range(num_spikes)
        self.intensity = to_range(intensity)
        self._warn_if_noop(is_noop=self.intensity.is_constant(0.0) or self.num_spikes.is_constant(0.0), hint="intensity=(1, 3)")

    @property
    def supports_per_instance_params(self) -> bool:
        return True

    @property
    def supports_per_instance_p(self) -> bool:
        return True

    def _draw_one(self) -> tuple[list[list[float]], float]:
        """The count, the positions, the intensity — in this order (spike.py:67-69, :83-85)."""
        num_spikes = max(1, round(self.num_spikes.sample_1d()))
        positions = torch.rand(num_spikes, 3).tolist()
        return positions, self.intensity.sample_1d()

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        n = self._resolve_n(batch)
        if n is None:
            positions, intensity = self._draw_one()
            return {"positions": positions, "intensity": intensity}
        keep = self._keep_mask(batch, n)
        keep_values = [True] * n if keep is None else keep.tolist()
        drawn = [self._draw_one() if should_keep else ([], 0.0) for should_keep in keep_values]
        params = {"positions": [d[0] for d in drawn], "intensity": [d[1] for d in drawn]}
        self._tag_batched(params, batch, n, keep, ["positions", "intensity"])
        return params

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        if self._is_per_instance_params(params):
            elements = list(zip(params["positions"], params["intensity"], strict=True))
        else:
            elements = [(params["positions"], params["intensity"])]
        if not any(positions and intensity != 0 for positions, intensity in elements):
            return batch  # nothing active: every image stays the object it was
        engine = ops.engine()
        for img_batch in self._get_images(batch).values():
            data = img_batch.data  # (pending lazy work is carried out here)
            shape = tuple(int(s) for s in data.shape[2:])
            entries = elements if len(elements) > 1 or data.shape[0] == 1 else elements * data.shape[0]
            lists = [spike_frequencies(positions, shape) if positions and intensity != 0 else [] for positions, intensity in entries]
            intensities = [intensity for _, intensity in entries]
            img_batch.data = engine.add_spikes(data, lists, intensities, engine.spectrum_peak(data))
        return batch


def spike_frequencies(positions, shape) -> list[tuple[int, int, int]]:
    """Positions in [0, 1) -> indices of the SHIFTED spectrum, ``int(p * s) % s`` (spike.py:155, :213) -> unshifted
    frequencies ``(index - s // 2) mod s``."""
    triples = []
    for position in positions:
        indices = [int(p * s) % s for p, s in zip(position, shape, strict=True)]
        triples.append(tuple((index - s // 2) % s for index, s in zip(indices, shape, strict=True)))
    return triples
