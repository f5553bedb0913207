"""Golden fixtures for LabelsToImage.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labels_to_image.py

Build container only.  Every case of ``tests/labels_to_image_cases.py`` runs through the UNMODIFIED reference on the CPU
(imported through ref_import.py): the whole call under ``torch.manual_seed(seed)`` — constructor, gate draw,
``make_params``, ``apply_transform``, history.  Writes ``tests/golden/labels_to_image_golden.pt``: per case the seed, the
label map, the recorded parameters, the history name, the generated image and the next ``torch.rand(1)`` of the global
generator (where the reference's stream stands afterwards), and the next draw after the gate and ``make_params`` alone.

Before anything is written, the properties the one-pass kernel relies on are held against the reference's own outputs: a
voxel whose label has no key, a non-integer voxel and the ignored background are +0.0, every other voxel is non-zero, and
the label map and the other images pass through.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import labels_to_image_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()


def main():
    golden = {"cases": {}}
    for name, (seed, elements, keywords) in cases.CASES.items():
        out, params, history_name, after = cases.run_case(tio, name)
        labels = torch.stack(elements())
        image = out.images[cases.IMAGE_KEY].data
        assert torch.equal(out.images["seg"].data, labels) and image.dtype == torch.float32
        assert image.shape == (labels.shape[0], 1, *labels.shape[2:])
        means = params["means"] if isinstance(params["means"], list) else [params["means"]] * labels.shape[0]
        for b, element_means in enumerate(means):
            drawn = [key for key, mean in element_means.items() if not (keywords.get("ignore_background") and key == 0)]
            with_key = torch.isin(labels[b, 0].double(), torch.tensor(drawn, dtype=torch.float64))
            assert bool((image[b, 0][with_key] != 0).all()), name
            rest = image[b, 0][~with_key]
            assert bool((rest.view(torch.int32) == 0).all()), name  # +0.0, bit for bit
            if "absent" in name or "non_integer" in name or keywords.get("ignore_background"):
                assert rest.numel() > 0 or b == 0, name
        drawn_params, after_params = cases.draw_case(tio, name)
        assert drawn_params == params, name
        golden["cases"][name] = {"seed": seed, "labels": labels, "params": params, "name": history_name, "out": image.clone(), "after": float(after),
                                 "after_params": after_params}
    path = os.path.join(HERE, "labels_to_image_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
