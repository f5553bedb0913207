"""Golden fixtures for the label-map transforms.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labels.py

Build container only.  ``RemapLabels``, ``RemoveLabels``, ``SequentialLabels``, ``OneHot`` and ``Contour`` run the
UNMODIFIED reference's ``apply_transform`` (imported through ref_import.py); ``KeepLargestComponent`` needs SimpleITK,
which is absent, so its expectation comes from ``scipy.ndimage.label`` (full / cross structuring element) with the rule of
keep_largest.py:108-125 — on fields without two equally large largest components, so that no tie rule enters.
Writes ``tests/golden/labels_golden.pt``: plain tensors / dicts (binary outputs as uint8).
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import scipy.ndimage
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from label_cases import label_field  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()
warnings.simplefilter("ignore")

SHAPE, SEED = (2, 1, 12, 10, 17), 1


def run(transform, data):
    batch = tio.SubjectsBatch.from_subjects([tio.Subject(seg=tio.LabelMap(element.clone())) for element in data])
    params = transform.make_params(batch)
    return transform.apply_transform(batch, params).images["seg"].data, params


def keep_largest_scipy(data, labels, background, fully_connected):
    structure = np.ones((3, 3, 3)) if fully_connected else scipy.ndimage.generate_binary_structure(3, 1)
    out = data.clone()
    for b in range(data.shape[0]):
        volume = data[b, 0].numpy()
        for value in labels:
            numbered, count = scipy.ndimage.label(volume == value, structure=structure)
            if count == 0:
                continue
            sizes = np.bincount(numbered.reshape(-1))[1:]
            assert (sizes == sizes.max()).sum() == 1, "two largest components tie: pick another field"
            out[b, 0][torch.from_numpy((numbered > 0) & (numbered != 1 + int(sizes.argmax())))] = background
    return out


def main():
    field = label_field(SHAPE, SEED).to(torch.int16)
    sparse = torch.tensor([0, 5, 10, 40], dtype=torch.int16)[field.long()]
    golden = {"shape": SHAPE, "seed": SEED, "field": field, "sparse": sparse}
    golden["remap"], params = run(tio.RemapLabels({1: 2, 2: 1, 3: 7, 9: 4}), field)
    golden["remap_params"] = params
    golden["remove"], _ = run(tio.RemoveLabels([2, 3], background_label=6), field)
    golden["sequential"], params = run(tio.SequentialLabels(), sparse)
    golden["sequential_params"] = params
    one_hot, _ = run(tio.OneHot(), field)
    golden["one_hot"] = one_hot.to(torch.uint8)
    one_hot, _ = run(tio.OneHot(num_classes=6), field)
    golden["one_hot_6"] = one_hot.to(torch.uint8)
    contour, _ = run(tio.Contour(), field)
    golden["contour"] = contour.to(torch.uint8)
    for fully_connected in (True, False):
        golden[f"keep_largest_{int(fully_connected)}"] = keep_largest_scipy(field, [1, 2, 3], 0, fully_connected)
    golden["keep_largest_label2_background5"] = keep_largest_scipy(field, [2], 5, True)
    path = os.path.join(HERE, "labels_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
