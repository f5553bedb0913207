"""Golden fixtures for PCA.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pca.py

Build container only.  Every case of ``tests/pca_cases.py: GOLDEN_CASES`` runs through the UNMODIFIED reference ``tio.PCA`` on
the CPU (imported through ref_import.py) under ``torch.manual_seed``.  The inputs have rank <= ``num_components``: there the
reference's randomised sketch spans the whole signal and its answer is the exact one, up to the sign of each component.
Writes ``tests/golden/pca_golden.pt``: per case the input, the reference's output, the next ``torch.rand(1)`` and ``dev_ref``,
the largest ``|reference - exact_pca|`` up to a per-component flip ``y <-> 1 - y``.  ``dev_ref <= 2e-6`` is asserted before
writing (measured: 1.1e-7 .. 4.2e-7; the cap leaves about 5 x for another BLAS): a condition on the inputs, not a bar on the engine.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pca_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()
DEV_REF_CAP = 2e-6


def main():
    golden = {"seed": cases.GOLDEN_SEED, "cases": {}}
    for name, (builder, arguments) in cases.GOLDEN_CASES.items():
        data = cases.make_input(**builder)
        out, next_rand = cases.run_case(tio, name, data)
        assert out.dtype == torch.float32 and out.shape == (data.shape[0], arguments["num_components"], *data.shape[2:])
        dev_ref = 0.0
        for b in range(data.shape[0]):
            exact = cases.exact_pca(data[b], **arguments)
            dev_ref = max(dev_ref, float(cases.flip_excess(out[b].numpy(), exact["out"], 0.0).max()))
        assert dev_ref <= DEV_REF_CAP, (name, dev_ref)
        golden["cases"][name] = {"input": data, "out": out.clone(), "next_rand": next_rand, "dev_ref": dev_ref}
        print(name, tuple(data.shape), "->", tuple(out.shape), "dev_ref", dev_ref, "next rand", float(next_rand))
    path = os.path.join(HERE, "pca_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
