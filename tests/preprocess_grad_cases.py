"""The pre-processing pipelines whose input gradient ``tests/golden/make_golden_preprocess_grad.py`` records from the reference
and ``tests/test_gpu_preprocess_backward.py`` replays on the HIP engine: ``CropOrPad(reflect)``, ``Resize``, ``Anisotropy``,
``Ghosting`` and ``Motion`` in front of ``sum(out^2)``.  One module for both sides, so that they cannot drift apart.

``stated``: the Compose with every transform at the arguments the fixture was asked for (``Ghosting()`` is the reference's
default, which scales no plane: it takes part in the draw order and the history only).  ``ghosting``: the same with
``Ghosting(intensity=(0.5, 1.0))``, so that the ghost lines carry a gradient too.  Each runs on one subject (shared parameters)
and on a batch of three (per-instance parameters; the seed makes ``Anisotropy`` draw more than one axis).
"""
from __future__ import annotations

import warnings

import torch

SEED = 7
SHAPE = (18, 14, 16)
VARIANTS = {"stated": {}, "ghosting": {"intensity": (0.5, 1.0)}}
CASES = [(variant, batch) for variant in VARIANTS for batch in (1, 3)]


def case_name(variant: str, batch: int) -> str:
    return f"{variant}-{'shared' if batch == 1 else 'per_instance'}"


def pipeline(tio, variant: str, copy: bool = True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # Ghosting() says that it does nothing
        return tio.Compose([
            tio.CropOrPad((20, 12, 16), padding_mode="reflect"), tio.Resize((15, 18, 12)), tio.Anisotropy(downsampling=2.5),
            tio.Ghosting(**VARIANTS[variant]), tio.Motion(),
        ], copy=copy)


def leaf(batch: int) -> torch.Tensor:
    return torch.randn((batch, 1, *SHAPE), generator=torch.Generator().manual_seed(100 + batch)) * 20.0 + 50.0


def run(tio, variant: str, batch: int, device: str = "cpu"):
    """``(d sum(out^2) / d input, the recorded parameter dictionaries, the output)`` of the case through *tio*."""
    data = leaf(batch).to(device).requires_grad_(True)
    # (a batch stacked from slices of the leaf is no leaf itself, and Compose's deepcopy takes leaves only: no copy there)
    pipe = pipeline(tio, variant, copy=batch == 1)
    torch.manual_seed(SEED)
    if batch == 1:
        single = data.detach()[0].clone().requires_grad_(True)  # Compose copies a subject, and a copy needs a leaf
        out = pipe(tio.Subject(t1=tio.ScalarImage(single)))
        result = out.t1.data
    else:
        out = pipe(tio.SubjectsBatch.from_subjects([tio.Subject(t1=tio.ScalarImage(data[b])) for b in range(batch)]))
        result = out.images["t1"].data
    (result ** 2).sum().backward()
    if batch == 1:
        return single.grad[None], [(record.name, record.params) for record in out.applied_transforms], result.detach()
    return data.grad, [(record.name, record.params) for record in out.applied_transforms], result.detach()
