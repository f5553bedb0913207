"""Recorded results of the UNMODIFIED reference for the tests that used to import it at run time.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_reference.py

Build container only (imports the reference through ref_import.py).  Writes ``tests/golden/reference_recorded.pt``
(plain tensors / strings / dicts, loads with ``torch.load(weights_only=True)``):

* ``autograd``: the gradient autograd derives through the reference's Compose (``tests/test_autograd.py``);
* ``compose96`` / ``spatial96``: the reference's outputs at 96^3 (``tests/test_reference_large.py``) — the SHA-256 of every
  output that must match bit for bit, and for the float images of the Compose (held to a relative tolerance) every
  ``SAMPLE_STRIDE``-th voxel of the flattened volume plus the float64 sum and sum of squares of the whole volume; for those
  float images also the SHA-256 of the CPU oracle's output, after checking it against the reference's at every voxel.
"""
from __future__ import annotations

import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

from oracle.oracle import oracle_engine  # noqa: E402
from ref_import import import_reference  # noqa: E402

import test_autograd  # noqa: E402
import test_reference_large  # noqa: E402
import torchio_amd  # noqa: E402

tio = import_reference()
warnings.simplefilter("ignore")


def main() -> None:
    record = {"torch": str(torch.__version__), "torchio": str(tio.__version__)}
    record["autograd"] = {"grad": test_autograd.reference_pipeline_grad(tio, None)}
    expected = test_reference_large.run_compose(tio, None)
    record["compose96"] = test_reference_large.record(expected, floats=("t1", "t2"))
    checked = test_reference_large.run_compose(torchio_amd, oracle_engine())
    worst = test_reference_large.check_every_voxel(expected, checked)  # (raises unless every voxel is within the bound)
    for name in ("t1", "t2"):
        record["compose96"][name]["checked_oracle_sha256"] = test_reference_large.record(checked, floats=())[name]["sha256"]
        record["compose96"][name]["checked_max_rel"] = worst[name]
    print("compose96: oracle vs reference, largest relative error per voxel", worst)
    record["spatial96"] = test_reference_large.record(test_reference_large.run_spatial(tio, None), floats=())
    path = os.path.join(HERE, "reference_recorded.pt")
    torch.save(record, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
