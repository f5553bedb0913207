"""GPU: every guarded case (``guarded_cases.py``) on the HIP engine — inputs, outputs and scratch between ``0xFF`` guards
(``guarded_memory.py``), the volumes 16-byte aligned (skew 0) and one element off (skew 1).  After every call: the guards,
then unwritten elements, then the values against the oracle at the bar of the op's own parity test; at skew 1, wherever
both roads are documented as bit-identical, also bit for bit against the aligned HIP result."""
from __future__ import annotations

import pytest
import torch

import guarded_cases
from guarded_cases import CASES
from guarded_cases import run_case

pytestmark = pytest.mark.gpu

_ALIGNED: dict = {}  # case id -> the HIP engine's outputs at skew 0


def _aligned(case, hip, oracle, monkeypatch):
    if case.id not in _ALIGNED:
        _ALIGNED[case.id] = run_case(case, hip, "cuda", 0, monkeypatch, oracle, hip)
    return _ALIGNED[case.id]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[case.id for case in CASES])
def test_case_on_hip(hip, oracle, monkeypatch, case, skew):
    guarded_cases._DEVICE[0] = "cuda"
    if skew == 0:
        _ALIGNED.pop(case.id, None)
        assert _aligned(case, hip, oracle, monkeypatch) is not None
        return
    got = run_case(case, hip, "cuda", 1, monkeypatch, oracle, hip)
    if case.at_skew1 == "none":
        assert got is None
    elif case.bits_at_skew:
        for n, (aligned, shifted) in enumerate(zip(_aligned(case, hip, oracle, monkeypatch), got, strict=True)):
            assert torch.equal(aligned.view(torch.uint8), shifted.view(torch.uint8)), f"{case.id}: output {n} depends on the alignment of its inputs"
