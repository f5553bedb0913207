"""Inputs and the float64 reference of the PCA tests (``test_pca_host.py``, ``test_gpu_pca.py``, ``golden/make_golden_pca.py``).

Inputs are ``Q diag(0.5^k) z`` plus a per-channel offset: ``Q`` a random orthogonal ``C x C`` matrix, ``z`` standard normal
``(latent, voxels)``.  The deviations of neighbouring components differ by 2 x, their eigenvalues by 4 x, so no case has
near-ties and every principal axis is well conditioned.  The offsets are of the size of the first component's deviation (one):
a mean far above the deviation is the subject of the scatter tests, not of the projection tests, whose bound prices the
float32 rounding of a centred dot product and leaves, of its ``C + 4`` units, two for the float32 rounding of the mean.

``exact_pca`` is a float64 numpy PCA with the package's sign convention (the entry of largest magnitude of each loading
vector is positive, the lowest index on ties); it never touches the engine.
"""
from __future__ import annotations

import numpy as np
import torch

GOLDEN_SEED = 20240
DEFAULT_RANGE = (-2.3, 2.3)

#: fixture cases: rank <= q inputs, where the reference's randomised sketch is exact.  name -> (builder arguments, PCA arguments)
GOLDEN_CASES = {
    "c3_q3": (dict(channels=3, shape=(6, 5, 7), seed=1), dict(num_components=3)),
    "c3_q3_noclip": (dict(channels=3, shape=(6, 5, 7), seed=2), dict(num_components=3, clip=False)),
    "c40_latent3": (dict(channels=40, shape=(9, 8, 7), seed=3, latent=3), dict(num_components=3)),
    "c40_latent3_noclip": (dict(channels=40, shape=(9, 8, 7), seed=4, latent=3), dict(num_components=3, clip=False)),
    "c40_latent3_raw": (dict(channels=40, shape=(9, 8, 7), seed=5, latent=3), dict(num_components=3, whiten=False, normalize=False, clip=False)),
    "c3_q3_raw_clip": (dict(channels=3, shape=(6, 5, 7), seed=6), dict(num_components=3, whiten=False, normalize=False)),
    "batch2_c40_latent3": (dict(channels=40, shape=(9, 8, 7), seed=7, latent=3, batch=2), dict(num_components=3)),
}


def make_input(channels: int, shape, seed: int, *, batch: int = 1, latent: int | None = None, offset: float = 1.0) -> torch.Tensor:
    """float32 ``(batch, channels, *shape)``; the batch elements differ in ``Q``, ``z`` and the offsets."""
    generator = torch.Generator().manual_seed(1000 + seed)
    latent = channels if latent is None else latent
    voxels = int(np.prod(shape))
    elements = []
    for _ in range(batch):
        q, _ = torch.linalg.qr(torch.randn(channels, channels, dtype=torch.float64, generator=generator))
        z = torch.randn(latent, voxels, dtype=torch.float64, generator=generator)
        scale = 0.5 ** torch.arange(latent, dtype=torch.float64)
        x = q[:, :latent] @ (scale[:, None] * z) + offset * torch.randn(channels, 1, dtype=torch.float64, generator=generator)
        elements.append(x.reshape(channels, *shape))
    return torch.stack(elements).to(torch.float32)


def batch_of(tio, data: torch.Tensor, device: str = "cpu", name: str = "emb"):
    """A ``SubjectsBatch`` of ``tio`` (the reference or this package) with one scalar image ``name`` per element of ``data``."""
    batch = tio.SubjectsBatch.from_subjects([tio.Subject(**{name: tio.ScalarImage(element.clone())}) for element in data])
    return batch if device == "cpu" else batch.to(device)


def run_case(tio, name: str, data: torch.Tensor | None = None, device: str = "cpu"):
    """A fixture case through ``tio`` under the fixture's seed: ``(output (B, q, I, J, K), the next torch.rand(1))``."""
    builder, arguments = GOLDEN_CASES[name]
    data = make_input(**builder) if data is None else data
    batch = batch_of(tio, data, device)
    torch.manual_seed(GOLDEN_SEED)
    out = tio.PCA(**arguments)(batch)
    return out.images["emb"].data, torch.rand(1)


def scatter_reference(x: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """float64 ``(mean (B, C), scatter (B, C, C))`` of a ``(B, C, ...)`` tensor, centred before the products."""
    flat = x.reshape(x.shape[0], x.shape[1], -1).to(torch.float64).numpy()
    mean = flat.mean(axis=2)
    centred = flat - mean[:, :, None]
    return mean, np.einsum("bcv,bdv->bcd", centred, centred)


def exact_pca(x: torch.Tensor, num_components: int = 3, *, whiten: bool = True, normalize: bool = True, values_range=DEFAULT_RANGE,
              clip: bool = True) -> dict:
    """The transform on ONE ``(C, I, J, K)`` element in float64, from the float32 values the reference's ``.float()`` makes.

    Returns ``out`` ``(q, I, J, K)`` and, for the error bound, ``weights`` ``(q, C)``, ``mean`` ``(C,)``, ``offset`` ``(q,)``
    and ``centred`` ``(C, voxels)``.
    """
    channels = x.shape[0]
    flat = x.to(torch.float32).to(torch.float64).reshape(channels, -1).numpy()
    n = flat.shape[1]
    mean = flat.mean(axis=1)
    centred = flat - mean[:, None]
    eigenvalues, eigenvectors = np.linalg.eigh(centred @ centred.T)
    order = np.argsort(eigenvalues)[::-1][:num_components]
    eigenvalues = np.clip(eigenvalues[order], 0.0, None)
    loadings = eigenvectors[:, order].T  # (q, C)
    for k in range(num_components):
        if loadings[k, np.argmax(np.abs(loadings[k]))] < 0:
            loadings[k] = -loadings[k]
    deviation = np.sqrt(eigenvalues / (n - 1 if n > 1 else 1))
    scale = np.ones(num_components)
    first = deviation[0]
    if whiten:
        std = np.maximum(deviation, 1e-8)
        scale = scale / std
        first = first / std[0]
    if normalize:
        scale = scale / (max(first, 1e-8) if n > 1 else float("nan"))
    low, high = values_range
    weights = loadings * (scale / (high - low))[:, None]
    offset = np.full(num_components, -low / (high - low))
    out = weights @ centred + offset[:, None]
    if clip:
        out = np.where(np.isnan(out), out, np.clip(out, 0.0, 1.0))
    return {"out": out.reshape(num_components, *x.shape[1:]), "weights": weights, "mean": mean, "offset": offset, "centred": centred}


def rounding_bound(exact: dict) -> np.ndarray:
    """``(C + 4) 2^-24 (sum_c |W_kc| |x_c - mean_c| + |o_k|)`` per component and voxel, in float64, shaped like ``out``: the
    float32 rounding of a ``C``-term centred dot product."""
    channels = exact["weights"].shape[1]
    magnitude = np.abs(exact["weights"]) @ np.abs(exact["centred"]) + np.abs(exact["offset"])[:, None]
    return ((channels + 4) * 2.0**-24 * magnitude).reshape(exact["out"].shape)


def flip_excess(values: np.ndarray, expected: np.ndarray, allowed) -> np.ndarray:
    """Per component, how far ``|values - expected| - allowed`` rises above zero at worst, taking for each component the better
    of ``expected`` and its mirror image ``1 - expected`` (a principal axis of the other sign, under the default range)."""
    values, expected = np.asarray(values, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    allowed = np.broadcast_to(np.asarray(allowed, dtype=np.float64), expected.shape)
    components = expected.shape[0]
    straight = (np.abs(values - expected) - allowed).reshape(components, -1).max(axis=1)
    mirrored = (np.abs(values - (1.0 - expected)) - allowed).reshape(components, -1).max(axis=1)
    return np.minimum(straight, mirrored)
