"""Golden fixtures for Reorient, Transpose, CropOrPad, EnsureShapeMultiple, ToReferenceSpace and CopyAffine.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_orientation.py

Build container only.  Every case of ``tests/orientation_cases.py`` runs through the UNMODIFIED reference on the CPU
(imported through ref_import.py): the whole call under ``torch.manual_seed(seed)``.  Writes
``tests/golden/orientation_golden.pt``: per case the output tensors, the output affines, the names and parameter
dictionaries of the history, and the next ``torch.rand(1)`` of the global generator.

``Reorient`` asks nibabel for four functions of ``nibabel.orientations`` that the stub module of ref_import.py does not
have.  They are installed here, after the import, written from nibabel's published algorithms and on their own: nothing
of ``torchio_amd`` is imported, so the fixture and the package's restatement (``torchio_amd/data/affine.py``) are two
independent readings.  Neither is trusted for the affine: ``tests/test_orientation_host.py`` holds every output affine
against the voxel correspondence worked out from ``perm`` / ``flip`` alone, and the same property is asserted here
before anything is written.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import orientation_cases as cases  # noqa: E402
from ref_import import import_reference  # noqa: E402

tio = import_reference()


# -- nibabel.orientations, the four functions reorient.py calls ----------------------------------------------------------
def io_orientation(affine, tol=None):
    affine = np.asarray(affine)
    q, p = affine.shape[0] - 1, affine.shape[1] - 1
    rzs = affine[:q, :p]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    left, s, right = np.linalg.svd(rs, full_matrices=False)
    if tol is None:
        tol = s.max() * max(rs.shape) * np.finfo(s.dtype).eps
    keep = s > tol
    r = np.dot(left[:, keep], right[keep])
    ornt = np.ones((p, 2), dtype=np.int8) * np.nan
    for in_ax in range(p):
        col = r[:, in_ax]
        if not np.allclose(col, 0):
            out_ax = np.argmax(np.abs(col))
            ornt[in_ax, 0] = out_ax
            ornt[in_ax, 1] = -1 if col[out_ax] < 0 else 1
            r[out_ax, :] = 0
    return ornt


def axcodes2ornt(axcodes, labels=None):
    labels = list(zip("LPI", "RAS", strict=True)) if labels is None else labels
    ornt = np.ones((len(axcodes), 2), dtype=np.int8) * np.nan
    for code_idx, code in enumerate(axcodes):
        for label_idx, codes in enumerate(labels):
            if code is None:
                continue
            if code in codes:
                ornt[code_idx, :] = [label_idx, -1 if code == codes[0] else 1]
                break
    return ornt


def ornt_transform(start_ornt, end_ornt):
    start_ornt, end_ornt = np.asarray(start_ornt), np.asarray(end_ornt)
    result = np.empty_like(start_ornt)
    for end_in_idx, (end_out_idx, end_flip) in enumerate(end_ornt):
        for start_in_idx, (start_out_idx, start_flip) in enumerate(start_ornt):
            if end_out_idx == start_out_idx:
                result[start_in_idx, :] = [end_in_idx, 1 if start_flip == end_flip else -1]
                break
        else:
            raise ValueError(f"Unable to find out axis {end_out_idx} in start_ornt")
    return result


def inv_ornt_aff(ornt, shape):
    ornt = np.asarray(ornt)
    p = ornt.shape[0]
    shape = np.array(shape)[:p]
    undo_reorder = np.eye(p + 1)[list(ornt[:, 0].astype(int)) + [p], :]
    undo_flip = np.diag(list(ornt[:, 1]) + [1.0])
    center_trans = -(shape - 1) / 2.0
    undo_flip[:p, p] = (ornt[:, 1] * center_trans) - center_trans
    return np.dot(undo_flip, undo_reorder)


orientations = sys.modules["nibabel.orientations"]
for function in (io_orientation, axcodes2ornt, ornt_transform, inv_ornt_aff):
    setattr(orientations, function.__name__, function)


def check_reorient(name: str, entry: dict) -> None:
    """World positions are kept: the output affine at an output corner is the input affine at the voxel it came from."""
    source, code = name.split("_to_")
    affine_in = cases.SOURCE_AFFINES[source]
    ornt = np.asarray(entry["params"][-1]["ornt"]) if entry["params"] else None
    for image in entry["images"].values():
        affine_out = image["affines"][0].numpy()
        out_shape = tuple(image["data"].shape[-3:])
        assert tuple(tio.AffineMatrix(affine_out).orientation) == tuple(code), name
        perm = [0, 1, 2] if ornt is None else [int(p) for p in np.argsort(ornt[:, 0])]
        flips = [] if ornt is None else [a for a in range(3) if ornt[a, 1] == -1]
        for corner in cases.corner_indices(out_shape):
            index_in = cases.input_index(corner, perm, flips, cases.REORIENT_SHAPE)
            np.testing.assert_allclose(affine_out @ [*corner, 1.0], affine_in @ [*index_in, 1.0], rtol=0, atol=1e-9, err_msg=name)


def main():
    golden = {"reorient": cases.run_moves(tio, cases.reorient_cases()), "transpose": cases.run_moves(tio, cases.transpose_cases())}
    for name, entry in golden["reorient"].items():
        if "_to_" in name:
            check_reorient(name, entry)
    for group in cases.GROUPS:
        golden[group] = cases.run_group(tio, group)
    golden["from_tensor"] = cases.from_tensor_case(tio)
    path = os.path.join(HERE, "orientation_golden.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes", {key: len(value) for key, value in golden.items()})


if __name__ == "__main__":
    main()
