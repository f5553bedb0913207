"""Cases of ``Reorient``, ``Transpose``, ``CropOrPad``, ``EnsureShapeMultiple``, ``ToReferenceSpace`` and ``CopyAffine``
shared by the fixture generator (``tests/golden/make_golden_orientation.py``, which runs them through the unmodified
reference on the CPU) and the tests (which run them through this package), plus the launch shapes of the
``permute3d`` tests.

Every case is one whole call ``transform(input)`` under ``torch.manual_seed(seed)``; ``record`` turns the result into
plain tensors, lists and strings.  The volumes are ``arange``-based: every element is distinct, so a misplaced one shows.
A plain module: nothing in the product imports it.
"""
from __future__ import annotations

import itertools
import math
import warnings

import numpy as np
import torch

# -- permute3d launches --------------------------------------------------------------------------------------------------
PERMUTATIONS = tuple(itertools.permutations(range(3)))
#: spatial shapes that put tile edges on every axis for a tile of 32, 64 or 128
PERMUTE_SHAPES = ((1, 1, 1), (2, 3, 1), (1, 33, 2), (31, 32, 33), (63, 2, 65), (64, 64, 3), (65, 1, 64), (3, 129, 31), (128, 2, 130))
PERMUTE_SHAPE_ONE_ELEMENT = (96, 80, 72)  # at (B, C) = (1, 1)
PERMUTE_DTYPES = (torch.uint8, torch.int16, torch.float32, torch.float64)  # element sizes 1 / 2 / 4 / 8


def distinct(shape, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    """``arange`` over *shape*; 1- and 2-byte types wrap, with a prime period that is no multiple of any extent in use.
    Never 255, -1 or NaN: the guarded tests read those as "not written"."""
    count = math.prod(shape)
    values = torch.arange(count, dtype=torch.int64, device=device)
    if dtype == torch.uint8:
        values = values % 251
    elif dtype == torch.int16:
        values = values % 32749 + 1
    return values.to(dtype).reshape(shape)


def aten_permute(data: torch.Tensor, perm, mask: int) -> torch.Tensor:
    """What the reference runs: the flips, then ``permute``, then ``contiguous`` (reorient.py:63-91)."""
    for axis in range(3):
        if mask & (1 << axis):
            data = torch.flip(data, [2 + axis])
    return data.permute(0, 1, 2 + perm[0], 2 + perm[1], 2 + perm[2]).contiguous()


# -- affines -------------------------------------------------------------------------------------------------------------
def _rotation_z(degrees: float) -> np.ndarray:
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _affine(direction, spacing, origin) -> np.ndarray:
    matrix = np.eye(4)
    matrix[:3, :3] = np.asarray(direction, dtype=np.float64) * np.asarray(spacing, dtype=np.float64)
    matrix[:3, 3] = origin
    return matrix


SOURCE_AFFINES = {
    "ras_anisotropic": _affine(np.eye(3), (0.8, 1.5, 2.0), (-10.0, 20.0, 5.5)),
    "lps": _affine(np.diag([-1.0, -1.0, 1.0]), (1.0, 1.0, 1.25), (90.0, 110.0, -30.0)),
    "oblique": _affine(_rotation_z(10.0) @ np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), (1.1, 0.9, 3.0), (4.0, -7.0, 12.0)),
}
ORIENTATIONS = tuple(
    "".join(code)
    for order in itertools.permutations(("LR", "PA", "IS"))
    for code in itertools.product(*order)
)
assert len(ORIENTATIONS) == 48 and len(set(ORIENTATIONS)) == 48

REORIENT_SHAPE = (3, 5, 4)
SHAPE = (6, 9, 7)


def subject(tio, shape=SHAPE, affine="ras_anisotropic", shift: int = 0, names=("t1", "seg")):
    """A float32 scalar image and an int16 label map of two channels each, every voxel distinct."""
    matrix = SOURCE_AFFINES[affine] if isinstance(affine, str) else affine
    entries = {}
    if "t1" in names:
        entries["t1"] = tio.ScalarImage(distinct((2, *shape), torch.float32) * 0.5 + shift, affine=matrix.copy())
    if "seg" in names:
        entries["seg"] = tio.LabelMap(distinct((2, *shape), torch.int16) + shift, affine=matrix.copy())
    return tio.Subject(**entries)


def on(data, device="cpu"):
    return data.to(device) if device != "cpu" else data


def batch_of(tio, subjects, device="cpu"):
    return on(tio.SubjectsBatch.from_subjects(subjects), device)


def _params(value):
    """Parameter dictionaries as plain python (tuples stay tuples)."""
    if isinstance(value, dict):
        return {key: _params(entry) for key, entry in value.items()}
    if isinstance(value, (list, tuple)):
        return type(value)(_params(entry) for entry in value)
    if isinstance(value, (np.ndarray, torch.Tensor)):
        return value.tolist()
    return value


def record(tio, out) -> dict:
    """Data, affines and history of a result, whatever its container."""
    if isinstance(out, tio.Image):
        images = {"image": {"data": out.data.cpu().clone(), "affines": [out.affine.data.cpu().clone()]}}
    elif isinstance(out, tio.Subject):
        images = {name: {"data": image.data.cpu().clone(), "affines": [image.affine.data.cpu().clone()]} for name, image in out.images.items()}
    else:
        images = {name: {"data": image.data.cpu().clone(), "affines": [a.data.cpu().clone() for a in image.affines]} for name, image in out.images.items()}
    history = list(getattr(out, "applied_transforms", []))
    return {
        "images": images,
        "history": [trace.name for trace in history],
        "params": [_params(trace.params) for trace in history],
    }


def run(tio, build, make_input, seed: int = 0) -> dict:
    """One whole call under the seed, and where the global generator stands afterwards."""
    transform = build(tio)
    data = make_input(tio)
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the statistic padding modes warn about integer inputs
        out = transform(data)
    after = float(torch.rand(1))
    entry = record(tio, out)
    entry["after"] = after
    return entry


# -- Reorient / Transpose ------------------------------------------------------------------------------------------------
def reorient_cases(device="cpu") -> dict:
    cases = {}
    for source in SOURCE_AFFINES:
        for code in ORIENTATIONS:
            cases[f"{source}_to_{code}"] = (
                lambda tio, code=code: tio.Reorient(code),
                lambda tio, source=source: batch_of(tio, [subject(tio, REORIENT_SHAPE, source)], device),
            )
    # the orientation of the FIRST element decides for the whole batch
    cases["batch2_first_decides"] = (
        lambda tio: tio.Reorient("LPS"),
        lambda tio: batch_of(tio, [subject(tio, REORIENT_SHAPE, "oblique"), subject(tio, REORIENT_SHAPE, "ras_anisotropic", 1)], device),
    )
    cases["include_t1_only"] = (
        lambda tio: tio.Reorient("SAL", include=["t1"]),
        lambda tio: batch_of(tio, [subject(tio, REORIENT_SHAPE, "lps")], device),
    )
    return cases


def transpose_cases(device="cpu") -> dict:
    return {
        "single_image": (lambda tio: tio.Transpose(), lambda tio: on(subject(tio, SHAPE, "oblique", names=("t1",)), device)),
        "batch2": (
            lambda tio: tio.Transpose(),
            lambda tio: batch_of(tio, [subject(tio, SHAPE, "ras_anisotropic"), subject(tio, SHAPE, "lps", 3)], device),
        ),
    }


# -- CropOrPad / EnsureShapeMultiple -------------------------------------------------------------------------------------
def _one(device, **kwargs):
    return lambda tio: batch_of(tio, [subject(tio, **kwargs)], device)


def crop_or_pad_cases(device="cpu") -> dict:
    """name -> (build, input, seed); shape (6, 9, 7) on spacing (0.8, 1.5, 2.0) unless the case says otherwise."""
    cases = {
        "pad_only_odd": (lambda tio: tio.CropOrPad((9, 12, 8)), _one(device), 0),
        "crop_only_odd": (lambda tio: tio.CropOrPad((3, 4, 6)), _one(device), 0),
        "mixed_per_axis": (lambda tio: tio.CropOrPad((8, 4, 7)), _one(device), 0),
        "none_axis": (lambda tio: tio.CropOrPad((8, None, 5)), _one(device), 0),
        "scalar_target": (lambda tio: tio.CropOrPad(7), _one(device), 0),
        "already_there": (lambda tio: tio.CropOrPad((6, 9, 7)), _one(device), 0),
        "millimetres": (lambda tio: tio.CropOrPad((8.0, 9.0, 10.0), units="mm"), _one(device), 0),
        "centimetres": (lambda tio: tio.CropOrPad((0.6, 1.2, 1.0), units="cm"), _one(device), 0),
        "only_crop": (lambda tio: tio.CropOrPad((8, 4, 7), only_crop=True), _one(device), 0),
        "only_pad": (lambda tio: tio.CropOrPad((8, 4, 7), only_pad=True), _one(device), 0),
        "include_seg": (lambda tio: tio.CropOrPad((8, 4, 7), include=["seg"]), _one(device), 0),
        "batch2_oblique": (
            lambda tio: tio.CropOrPad((5, 11, 7), fill=-2),
            lambda tio: batch_of(tio, [subject(tio, affine="oblique"), subject(tio, affine="lps", shift=2)], device), 0),
        "subject_mixed": (lambda tio: tio.CropOrPad((8, 4, 7)), lambda tio: on(subject(tio), device), 0),
        "subject_crop_only": (lambda tio: tio.CropOrPad((3, 4, 6), include=["t1"]), lambda tio: on(subject(tio), device), 0),
        "image_pad": (lambda tio: tio.CropOrPad((9, 12, 8), fill=1.5), lambda tio: on(subject(tio), device).images["t1"], 0),
    }
    for seed in (1, 2, 3):
        cases[f"random_seed{seed}"] = (lambda tio: tio.CropOrPad((3, 4, 9), location="random"), _one(device), seed)
    cases["random_subject"] = (lambda tio: tio.CropOrPad((2, 9, 3), location="random"), lambda tio: on(subject(tio), device), 5)
    for mode in ("constant", "reflect", "replicate", "circular", "mean", "median", "minimum"):
        fill = 3.5 if mode == "constant" else 0
        cases[f"mode_{mode}"] = (lambda tio, mode=mode, fill=fill: tio.CropOrPad((9, 12, 8), padding_mode=mode, fill=fill), _one(device), 0)
    return cases


def ensure_shape_multiple_cases(device="cpu") -> dict:
    return {
        "pad_scalar": (lambda tio: tio.EnsureShapeMultiple(4), _one(device), 0),
        "crop_scalar": (lambda tio: tio.EnsureShapeMultiple(4, method="crop"), _one(device), 0),
        "pad_tuple_two_axes_fit": (lambda tio: tio.EnsureShapeMultiple((3, 4, 7)), _one(device), 0),
        "crop_below_the_multiple": (lambda tio: tio.EnsureShapeMultiple(8, method="crop"), _one(device), 0),
        "pad_replicate": (lambda tio: tio.EnsureShapeMultiple((4, 5, 2), padding_mode="replicate"), _one(device), 0),
        "subject_pad": (lambda tio: tio.EnsureShapeMultiple(4, fill=7), lambda tio: on(subject(tio), device), 0),
        "subject_crop": (lambda tio: tio.EnsureShapeMultiple((4, 2, 3), method="crop"), lambda tio: on(subject(tio), device), 0),
    }


# -- ToReferenceSpace / CopyAffine ---------------------------------------------------------------------------------------
def reference_image(tio, affine="oblique", shape=(8, 10, 12)):
    return tio.ScalarImage(torch.zeros(1, *shape), affine=SOURCE_AFFINES[affine].copy())


def to_reference_space_cases(device="cpu") -> dict:
    return {
        "oblique_reference": (lambda tio: tio.ToReferenceSpace(reference_image(tio)), _one(device, shape=(4, 5, 6)), 0),
        "other_shape_batch2": (
            lambda tio: tio.ToReferenceSpace(reference_image(tio, "ras_anisotropic", (16, 9, 7))),
            lambda tio: batch_of(tio, [subject(tio, (3, 7, 5), "lps"), subject(tio, (3, 7, 5), "oblique", 1)], device), 0),
        "include_t1": (lambda tio: tio.ToReferenceSpace(reference_image(tio), include=["t1"]), _one(device, shape=(4, 5, 6)), 0),
    }


def from_tensor_case(tio) -> dict:
    image = tio.ToReferenceSpace.from_tensor(distinct((3, 2, 5, 3), torch.float32), reference_image(tio))
    return {"class": type(image).__name__, "data": image.data.clone(), "affine": image.affine.data.clone()}


def copy_affine_cases(device="cpu") -> dict:
    def two_grids(tio):
        nearby = SOURCE_AFFINES["oblique"].copy()
        nearby[:3] += 1e-6  # what a round trip through single precision does to an affine
        first = subject(tio, affine="oblique", names=("t1",)).images["t1"]
        second = subject(tio, affine=nearby, names=("seg",)).images["seg"]
        third = subject(tio, affine="lps", names=("t1",)).images["t1"]
        return batch_of(tio, [tio.Subject(t1=first, seg=second, t2=third)], device)

    return {"from_t1": (lambda tio: tio.CopyAffine("t1"), two_grids, 0)}


GROUPS = {
    "crop_or_pad": crop_or_pad_cases,
    "ensure_shape_multiple": ensure_shape_multiple_cases,
    "to_reference_space": to_reference_space_cases,
    "copy_affine": copy_affine_cases,
}


def run_group(tio, group: str, device="cpu") -> dict:
    return {name: run(tio, build, make_input, seed) for name, (build, make_input, seed) in GROUPS[group](device).items()}


def run_moves(tio, cases: dict) -> dict:
    """Reorient / Transpose cases: ``(build, input)`` pairs, seed 0."""
    return {name: run(tio, build, make_input) for name, (build, make_input) in cases.items()}


#: float64 products of a handful of terms of magnitude <= 1e3: the margin covers the summation order only
AFFINE_BAR = 1e-12


def assert_same(ours: dict, expected: dict, name: str, affine_bar: float = 0.0) -> None:
    assert ours["history"] == expected["history"], name
    assert ours["params"] == expected["params"], name
    assert ours["after"] == expected["after"], name  # the global generator stands where the reference's stood
    assert list(ours["images"]) == list(expected["images"]), name
    for key, image in expected["images"].items():
        got = ours["images"][key]
        assert got["data"].dtype == image["data"].dtype and torch.equal(got["data"], image["data"]), (name, key)
        assert len(got["affines"]) == len(image["affines"])
        for mine, theirs in zip(got["affines"], image["affines"], strict=True):
            assert mine.dtype == torch.float64
            assert float((mine - theirs).abs().max()) <= affine_bar, (name, key)


# -- the property the affine algebra must have, worked out from perm / flip alone ----------------------------------------
def corner_indices(shape) -> np.ndarray:
    return np.array(list(itertools.product(*[(0, s - 1) for s in shape])), dtype=np.float64)


def input_index(output_index, perm, flips, in_shape) -> np.ndarray:
    """The input voxel an output voxel was taken from: ``i[perm[d]] = o_d``, mirrored where the input axis is flipped."""
    index = np.zeros(3)
    for d in range(3):
        axis = perm[d]
        index[axis] = in_shape[axis] - 1 - output_index[d] if axis in flips else output_index[d]
    return index
