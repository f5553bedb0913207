"""Golden fixtures for Swap and HistogramStandardization.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_swap_histogram.py

Build container only.  Every case of ``tests/swap_histogram_cases.py`` runs through the UNMODIFIED reference on the CPU
(imported through ref_import.py): the whole call — gate draw, ``make_params``, ``apply_transform``, history.  Writes
``tests/golden/swap_histogram_golden.pt``: per case the recorded parameters, the history name, the warnings and the output
(the inputs are the cases module's seeded tensors and are not stored); for the landmark training the landmarks and the
``np.percentile`` rows they were averaged from.
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

import swap_histogram_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()


def main():
    golden = {"seed": cases.GOLDEN_SEED, "cases": {}}
    for name in [*cases.SWAP_CASES, *cases.HISTOGRAM_CASES]:
        out, params, history_name, messages = cases.run_case(tio, name)
        entry = {"params": params, "name": history_name, "warnings": messages, "out": {key: image.data.clone() for key, image in out.images.items()}}
        if name in cases.SWAP_CASES and cases.swap_inputs(name)[2] is not None:
            assert torch.equal(out.images["seg"].data, cases.swap_inputs(name)[2]), "the label map passes through"
            assert len(messages) == 1
        if name == "swap_all_pairs_overlap":
            patch = cases.SWAP_CASES[name][0]["patch_size"]
            assert all(all(abs(a[d] - b[d]) < patch[d] for d in range(3)) for a, b in params["locations"]), "every pair overlaps"
        if name == "swap_gated":
            assert any(entry == [] for entry in params["locations"]) and any(params["locations"])
        golden["cases"][name] = entry
    for name, mask_fn in cases.LANDMARK_CASES.items():
        rows = [cases.percentiles(cases.inside_values(image, None if mask_fn is None else mask_fn(image)), cases.DEFAULT_QUANTILES)
                for image in cases.training_images()]
        golden["cases"][name] = {"landmarks": cases.run_case(tio, name), "database": torch.as_tensor(np.vstack(rows))}
    path = os.path.join(HERE, "swap_histogram_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")
    for name, entry in golden["cases"].items():
        print(name, {k: (tuple(v.shape) if hasattr(v, "shape") else (len(v["locations"]) if isinstance(v, dict) and "locations" in v else v)) for k, v in entry.items() if k != "out"})


if __name__ == "__main__":
    main()
