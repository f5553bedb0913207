"""Golden fixture for the data gradients through the pre-processing transforms.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_preprocess_grad.py

Build container only.  Every case of ``tests/preprocess_grad_cases.py`` runs through the UNMODIFIED reference on the CPU (imported
through ref_import.py): ``Compose([CropOrPad(reflect), Resize, Anisotropy, Ghosting, Motion])`` on a leaf that requires a
gradient, then ``sum(out^2).backward()``.  Writes ``tests/golden/preprocess_grad_golden.pt``: per case the input, the recorded
parameter dictionaries of every transform and ``d sum(out^2) / d input`` as autograd derived it through the reference's torch ops.

Before anything is written: the gradient is finite and non-zero, and the per-instance cases drew more than one Anisotropy axis.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import preprocess_grad_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()


def main():
    golden = {"seed": cases.SEED, "cases": {}}
    for variant, batch in cases.CASES:
        grad, records, out = cases.run(tio, variant, batch)
        assert grad.shape == (batch, 1, *cases.SHAPE) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        assert [name for name, _ in records] == ["Pad", "Crop", "CropOrPad", "Resize", "Anisotropy", "Ghosting", "Motion"], [name for name, _ in records]
        if batch > 1:
            anisotropy = dict(records)["Anisotropy"]
            assert len(set(anisotropy["axis"])) > 1, f"seed {cases.SEED}: every element drew axis {anisotropy['axis']}"
        golden["cases"][cases.case_name(variant, batch)] = {"input": cases.leaf(batch), "records": records, "grad": grad.clone(), "out_shape": tuple(out.shape)}
    path = os.path.join(HERE, "preprocess_grad_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")
    for name, entry in golden["cases"].items():
        print(name, entry["out_shape"], float(entry["grad"].abs().max()), entry["records"])


if __name__ == "__main__":
    main()
