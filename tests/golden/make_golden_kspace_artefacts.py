"""Golden fixtures for Ghosting and Spike.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kspace_artefacts.py

Build container only.  Every case of ``tests/kspace_artefact_cases.py`` runs through the UNMODIFIED reference on the CPU
(imported through ref_import.py): the whole call — constructor, gate draw, ``make_params``, ``apply_transform``, history.
Writes ``tests/golden/kspace_artefacts_golden.pt``: per case the recorded parameters, the history name, the warnings and the
output (the inputs are the cases module's seeded tensors and are not stored).

Before anything is written, every output is held against the float64 FFT-route restatement of the cases module with the
bars of the GPU tests (``cases.check``): the fixtures alone satisfy the conditions the engine is tested under, the integer
cases' share cap included.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import kspace_artefact_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()


def main():
    golden = {"seed": cases.GOLDEN_SEED, "cases": {}}
    for name in cases.CASES:
        out, params, history_name, built, messages = cases.run_case(tio, name)
        image = cases.case_input(name)
        assert out.dtype == image.dtype and out.shape == image.shape
        cases.check(out, cases.expected_for(name, params), name)
        if name.endswith("_noop"):
            assert torch.equal(out, image) and len(built) == 1, "the default does nothing, and says so"
        elif name.endswith("_gated"):
            assert 0 < sum(params["_keep"]) < len(params["_keep"])
            for b, keep in enumerate(params["_keep"]):
                assert keep or torch.equal(out[b], image[b]), "a gated-out element passes through"
        else:
            assert not torch.equal(out, image), "the case changes its input"
        golden["cases"][name] = {"params": params, "name": history_name, "built": built, "warnings": messages, "out": out.clone()}
    path = os.path.join(HERE, "kspace_artefacts_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")
    for name, entry in golden["cases"].items():
        print(name, {k: v for k, v in entry["params"].items() if k != "positions"}, entry["built"], entry["warnings"])


if __name__ == "__main__":
    main()
