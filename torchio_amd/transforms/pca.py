"""``PCA`` on the HIP engine (mirror of reference ``transforms/intensity/pca.py``).

The reference centres the ``(voxels, C)`` matrix of every element and hands it to ``torch.pca_lowrank``, a randomised
sketch.  Here the whole batch is read twice: ``tio_channel_scatter`` makes the channel means and the ``C x C`` scatter
matrix in float64, ``torch.linalg.eigh`` of that small matrix gives the exact principal axes, and ``tio_channel_project``
centres, projects, whitens, normalises, maps ``values_range`` onto ``[0, 1]`` and clips in one pass.  Nothing is read back.

Sign convention (this package's own; the reference's sign is whatever its random sketch gives): each loading vector is
signed so that its entry of largest magnitude is positive, the lowest index on ties.

The reference draws ``torch.randn(C, num_components)`` from the global CPU generator once per element and image, inside
``pca_lowrank``; the same numbers are drawn and discarded here, so a seeded pipeline stays in step with the reference.
"""
from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from .. import ops
from ..data.batch import SubjectsBatch
from .transform import IntensityTransform


def projection_parameters(mean: Tensor, scatter: Tensor, voxels: int, num_components: int, *, whiten: bool, normalize: bool,
                          values_range: tuple[float, float]) -> tuple[Tensor, Tensor, Tensor]:
    """``(center, weights, offset)`` for ``Engine.channel_project`` from the float64 ``(B, C)`` means and ``(B, C, C)``
    scatter matrices of ``Engine.channel_scatter``: float32 ``(B, C)``, ``(B, q, C)`` and ``(B, q)``, on their device.
    Everything is formed in float64 and rounded once."""
    eigenvalues, eigenvectors = torch.linalg.eigh(scatter)  # ascending
    eigenvalues = eigenvalues[:, -num_components:].flip(-1).clamp(min=0.0)  # (B, q), descending
    loadings = eigenvectors[:, :, -num_components:].flip(-1).transpose(1, 2)  # (B, q, C)
    largest = loadings.abs().argmax(dim=2, keepdim=True)  # (the first of equal maxima)
    sign = torch.where(loadings.gather(2, largest) < 0, -1.0, 1.0)
    loadings = loadings * sign
    deviation = (eigenvalues / (voxels - 1 if voxels > 1 else 1)).sqrt()  # of each projected component, unbiased
    scale = torch.ones_like(deviation)
    first = deviation[:, :1]
    if whiten:
        std = deviation.clamp(min=1e-8)
        scale = scale / std
        first = first / std[:, :1]
    if normalize:
        # (`.std()` of one value is NaN in the reference too)
        first_std = first.clamp(min=1e-8) if voxels > 1 else torch.full_like(first, float("nan"))
        scale = scale / first_std
    low, high = (float(v) for v in values_range)
    weights = loadings * (scale / (high - low)).unsqueeze(2)
    offset = torch.full_like(deviation, -low / (high - low))
    return mean.to(torch.float32), weights.to(torch.float32), offset.to(torch.float32)


class PCA(IntensityTransform):
    """Reduce the channel axis to its first ``num_components`` principal components (pca.py:15-140): a ``(C, I, J, K)``
    image becomes ``(num_components, I, J, K)`` float32, e.g. a feature map as an RGB image.

    ``whiten``: each component to unit variance.  ``normalize``: all components divided by the standard deviation of the
    first.  ``values_range``: mapped linearly onto ``[0, 1]`` (the default covers 99 % of a standard normal).  ``clip``: the
    result clamped to ``[0, 1]``.  The components are exact (an eigendecomposition of the covariance, not the reference's
    randomised sketch) and signed as the module's docstring says.
    """

    def __init__(self, num_components: int = 3, *, whiten: bool = True, normalize: bool = True,
                 values_range: tuple[float, float] = (-2.3, 2.3), clip: bool = True, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if num_components < 1:
            raise ValueError(f"num_components must be >= 1, got {num_components}")
        self.num_components = num_components
        self.whiten = whiten
        self.normalize = normalize
        self.values_range = values_range
        self.clip = clip

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for img_batch in self._get_images(batch).values():
            data = img_batch.data
            channels = int(data.shape[1])
            if channels < self.num_components:
                raise ValueError(f"Image has {channels} channels but num_components={self.num_components}. Need at least as many "
                                 "channels as components.")
            if data.dtype != torch.float32:
                data = data.float()
            engine = ops.engine()
            mean, scatter = engine.channel_scatter(data)
            for _ in range(int(data.shape[0])):  # pca_lowrank's sketch matrix, per element: drawn to keep the generator in step
                torch.randn(channels, self.num_components)
            voxels = int(data.shape[2]) * int(data.shape[3]) * int(data.shape[4])
            center, weights, offset = projection_parameters(mean, scatter, voxels, self.num_components, whiten=self.whiten,
                                                            normalize=self.normalize, values_range=self.values_range)
            img_batch.data = engine.channel_project(data, center, weights, offset, clip=self.clip)
        return batch
