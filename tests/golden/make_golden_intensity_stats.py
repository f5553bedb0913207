"""Golden fixtures for Normalize / Standardize / Clamp / Mask.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_intensity_stats.py

Build container only.  Every case of ``tests/intensity_stats_cases.py`` runs through the UNMODIFIED reference on the CPU
(imported through ref_import.py): the whole call — gate draw, ``make_params``, ``apply_transform``, history — and, for
the listed cases, ``apply_inverse_transform`` on the result.  Writes ``tests/golden/intensity_stats_golden.pt``: per case the
recorded parameters, the history name and the output (the inputs are the cases module's seeded tensors, kept as well).
"""
from __future__ import annotations

import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import intensity_stats_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()
warnings.simplefilter("ignore")


def main():
    golden = {"shape": cases.GOLDEN_SHAPE, "seed": cases.GOLDEN_SEED, "image": cases.golden_image(), "labels": cases.golden_labels(), "cases": {}}
    for name in cases.CASES:
        out, params, history_name = cases.run_case(tio, name)
        entry = {"params": params, "name": history_name, "out": out.images["t1"].data.clone()}
        assert torch.equal(out.images["seg"].data, cases.golden_labels()), "the label map passes through"
        if name in cases.INVERSES:
            entry["restored"] = tio.apply_inverse_transform(out).images["t1"].data.clone()
        golden["cases"][name] = entry
    subjects = [tio.Subject(t1=tio.ScalarImage(cases.golden_image()[b].clone())) for b in range(cases.GOLDEN_SHAPE[0])]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    batch.applied_transforms.append(tio.AppliedTransform("Normalize", dict(cases.ZERO_RANGE_INVERSE)))
    golden["zero_range_restored"] = tio.apply_inverse_transform(batch).images["t1"].data.clone()
    path = os.path.join(HERE, "intensity_stats_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
