"""GPU: the gradient through ``Compose([CropOrPad(reflect), Resize, Anisotropy, Ghosting, Motion])`` on the HIP engine against
the gradient autograd derived through the UNMODIFIED reference (``tests/golden/preprocess_grad_golden.pt``, recorded by
``tests/golden/make_golden_preprocess_grad.py`` from the cases of ``tests/preprocess_grad_cases.py``).

The same seed replays the same draws: the recorded parameter dictionaries must match first, so that a draw-order slip cannot pass
as a gradient error.  The gradient is held to ``1e-4`` of its scale, the bar ``tests/test_autograd.py`` uses for the six-transform
Compose.
"""
from __future__ import annotations

import os

import pytest
import torch

import preprocess_grad_cases as cases
import torchio_amd as tio
from parity_harness import use_engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess_grad_golden.pt")


def _plain(value):
    """Parameter dictionaries as nested lists / dicts of numbers: the two packages may differ in tuple against list."""
    if isinstance(value, dict):
        return {key: _plain(item) for key, item in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(item) for item in value]
    if isinstance(value, torch.Tensor):
        return _plain(value.tolist())
    return pytest.approx(value, rel=1e-6, abs=1e-9) if isinstance(value, float) else value


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=True)


@pytest.mark.parametrize(("variant", "batch"), cases.CASES, ids=[cases.case_name(v, b) for v, b in cases.CASES])
def test_the_gradient_equals_the_one_autograd_derived_through_the_reference(hip, golden, variant, batch):
    entry = golden["cases"][cases.case_name(variant, batch)]
    assert golden["seed"] == cases.SEED and torch.equal(entry["input"], cases.leaf(batch))
    with use_engine(hip):
        grad, records, out = cases.run(tio, variant, batch, device="cuda")
    assert tuple(out.shape) == tuple(entry["out_shape"])
    assert [name for name, _ in records] == [name for name, _ in entry["records"]]
    for (name, params), (_, expected) in zip(records, entry["records"], strict=True):
        assert _plain(params) == _plain(expected), name
    expected = entry["grad"]
    assert grad.shape == expected.shape and grad.dtype == expected.dtype
    scale = float(expected.abs().max())
    worst = float((grad.cpu() - expected).abs().max())
    print(f"[preprocess backward] {cases.case_name(variant, batch)}: max|d| = {worst:.3e} = {worst / scale:.3e} of the scale")
    assert worst <= 1e-4 * scale
