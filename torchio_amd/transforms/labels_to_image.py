"""``LabelsToImage`` on the HIP engine (mirror of reference ``transforms/intensity/labels_to_image.py``).

The reference loops over the labels and runs, per label, a full-volume ``randn_like``, a multiply, an add, a ``==`` mask,
a cast, another multiply and an accumulate.  The masks are disjoint, so every voxel receives exactly one Gaussian draw with
the mean and the deviation of its own label: ``tio_labels_to_image`` (``csrc/labels_to_image.hip``) reads the label, looks
the pair up and writes the float32 voxel in one pass.  Same constructor, draw order, parameter dictionary, errors and
history as the reference.

Two sources for the standard-normal draws, selected by :func:`~torchio_amd.transforms.noise.set_noise_rng`:

``"philox"``
    one seed is drawn from the global generator at the start of ``apply_transform`` and the whole image is one launch with
    in-kernel draws (Philox4x32-10 + Box-Muller, the stream of ``Engine.philox_normal``).  Same distribution, another
    stream: NOT reference-identical.
``"reference"`` (default)
    exactly the reference's run on the CPU: for every label, in the reference's loop order, ``torch.randn((B, 1, I, J, K))``
    from the global CPU generator, uploaded and applied by one launch in one-label mode.  Bit-identical under
    ``torch.manual_seed``, at the cost of one host draw and one upload of the whole volume PER LABEL.

The generated image lives on the device it was computed on.  One deliberate difference in structure: the new ``ImagesBatch``
gets CLONES of the label map's affines (the reference hands over the list object itself), so that a later spatial transform
of one image cannot move the other's affine.
"""
from __future__ import annotations

from collections.abc import Sequence
from typing import Any

import torch
from torch import Tensor

from .. import ops
from ..data.batch import ImagesBatch
from ..data.batch import SubjectsBatch
from ..data.image import LabelMap
from ..data.image import ScalarImage
from . import noise
from .parameter_range import to_range
from .transform import Transform


class LabelsToImage(Transform):
    """Generate a synthetic ``ScalarImage`` from a label map (labels_to_image.py:19-179): per label a Gaussian tissue with a
    sampled mean and deviation, SynthSeg style.  Compose with ``Blur`` and ``BiasField``.

    ``label_key``: the label map to read (``None``: the first ``LabelMap``); ``image_key``: the name of the new image.
    ``mean`` / ``std``: per-label ranges, by position in the sorted labels of the first batch element; labels beyond the
    lists draw from ``default_mean`` / ``default_std``.  ``ignore_background``: label 0 stays zero.  Existing images are not
    modified.  Not invertible.
    """

    def __init__(
        self,
        label_key: str | None = None,
        *,
        image_key: str = "image_from_labels",
        mean: Sequence[float | tuple[float, float]] | None = None,
        std: Sequence[float | tuple[float, float]] | None = None,
        default_mean: float | tuple[float, float] = (0.1, 0.9),
        default_std: float | tuple[float, float] = (0.01, 0.1),
        ignore_background: bool = False,
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        self.label_key = label_key
        self.image_key = image_key
        self.mean_ranges = [to_range(m) for m in mean] if mean is not None else None
        self.std_ranges = [to_range(s) for s in std] if std is not None else None
        self.default_mean = to_range(default_mean)
        self.default_std = to_range(default_std)
        self.ignore_background = ignore_background

    @property
    def supports_per_instance_params(self) -> bool:
        return True

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        label_batch = self._find_label_batch(batch)
        # the labels of the FIRST element (labels_to_image.py:86); int() folds 1.2 and 1.7 into two entries of key 1
        unique = sorted(int(v) for v in ops.engine().unique_labels(label_batch.data[0]).tolist())
        n = self._resolve_n(batch)
        if n is None:
            means, stds = self._sample_label_values(unique)
            return {"means": means, "stds": stds}
        means_list: list[dict[int, float]] = []
        stds_list: list[dict[int, float]] = []
        for _ in range(n):
            means, stds = self._sample_label_values(unique)
            means_list.append(means)
            stds_list.append(stds)
        params = {"means": means_list, "stds": stds_list}
        self._tag_batched(params, batch, n, None, ["means", "stds"])
        return params

    def _sample_label_values(self, unique: list[int]) -> tuple[dict[int, float], dict[int, float]]:
        """One mean and one deviation per label, in the reference's draw order (labels_to_image.py:105-132)."""
        means: dict[int, float] = {}
        stds: dict[int, float] = {}
        for idx, label in enumerate(unique):
            if self.ignore_background and label == 0:
                means[label] = 0.0
                stds[label] = 0.0
                continue
            if self.mean_ranges is not None and idx < len(self.mean_ranges):
                means[label] = self.mean_ranges[idx].sample_1d()
            else:
                means[label] = self.default_mean.sample_1d()
            if self.std_ranges is not None and idx < len(self.std_ranges):
                stds[label] = self.std_ranges[idx].sample_1d()
            else:
                stds[label] = abs(self.default_std.sample_1d())
        return means, stds

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        label_batch = self._find_label_batch(batch)
        data = label_batch.data
        per_element = self._is_per_instance_params(params)
        # the reference's loop order: the dictionary's own for shared parameters, the sorted union for per-element ones
        if per_element:
            order = sorted(set().union(*(values.keys() for values in params["means"])))
            means = [[values.get(label, 0.0) for label in order] for values in params["means"]]
            stds = [[values.get(label, 0.0) for label in order] for values in params["stds"]]
            # (the reference counts the non-zeros of the float32 tensors, labels_to_image.py:249-260)
            zero = (torch.tensor(means, dtype=torch.float32) == 0) & (torch.tensor(stds, dtype=torch.float32) == 0)
            skipped = zero.reshape(len(means), len(order)).all(dim=0).tolist()
        else:
            order = list(params["means"])
            means = [params["means"][label] for label in order]
            stds = [params["stds"].get(label, 0.0) for label in order]
            skipped = [m == 0.0 and s == 0.0 for m, s in zip(means, stds, strict=True)]
        # the engine takes its keys in ascending order
        by_key = sorted(range(len(order)), key=lambda j: order[j])
        keys = [order[j] for j in by_key]
        if per_element:
            means, stds = [[row[j] for j in by_key] for row in means], [[row[j] for j in by_key] for row in stds]
        else:
            means, stds = [means[j] for j in by_key], [stds[j] for j in by_key]
        engine = ops.engine()
        if noise.get_noise_rng() == "philox":
            seed = int(torch.randint(0, 2**31, (1,)).item())
            generated = engine.labels_to_image(data, keys, means, stds, seed=seed)
        else:
            shape = (data.shape[0], 1, *data.shape[2:])
            generated = torch.zeros(shape, dtype=torch.float32, device=data.device)
            position = {j: at for at, j in enumerate(by_key)}
            for j in range(len(order)):
                if skipped[j]:
                    continue  # (labels_to_image.py:212, :284: no draw for a label whose mean and deviation are all zero)
                base = ops.h2d(torch.randn(shape), data.device)
                engine.labels_to_image(data, keys, means, stds, base=base, base_key=position[j], out=generated)
        batch.images[self.image_key] = ImagesBatch(generated, [a.clone() for a in label_batch.affines], image_class=ScalarImage)
        return batch

    def _find_label_batch(self, batch: SubjectsBatch) -> ImagesBatch:
        if self.label_key is not None:
            if self.label_key not in batch.images:
                raise KeyError(f"Label key '{self.label_key}' not found. Available: {list(batch.images.keys())}")
            return batch.images[self.label_key]
        for img_batch in batch.images.values():
            if issubclass(img_batch._image_class, LabelMap):
                return img_batch
        raise KeyError("No LabelMap found in the subject")
