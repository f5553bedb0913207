"""Cases of ``LabelsToImage`` shared by the fixture generator (``tests/golden/make_golden_labels_to_image.py``, which runs
them through the unmodified reference on the CPU) and the tests (which run them through this package).

Every case is one whole call ``transform(batch)`` under ``torch.manual_seed(seed)``: gate draw, ``make_params``,
``apply_transform``, history.  The label maps are small and deterministic (no generator involved), so the fixture stores
them only as a check.  A plain module: nothing in the product imports it.
"""
from __future__ import annotations

import torch

SHAPE_ODD = (7, 5, 9)   # 315 voxels: no multiple of 4, so the rows of elements 1 and later start off a quad
SHAPE_EVEN = (4, 4, 4)
IMAGE_KEY = "image_from_labels"


def label_volume(shape: tuple, values: list, shift: int = 0) -> torch.Tensor:
    """``(1, I, J, K)`` float64: blocks of ``values`` in an order that depends on the position and on ``shift``."""
    i, j, k = torch.meshgrid(*(torch.arange(s) for s in shape), indexing="ij")
    index = (i * 3 + j * 5 + k // 2 + (i * j) % 3 + shift) % len(values)
    return torch.tensor(values, dtype=torch.float64)[index][None]


def _elements(shape, values, dtype, count):
    return [label_volume(shape, values, shift).to(dtype) for shift in range(count)]


def _absent_label(shape, dtype):
    """Element 0 holds 0, 1, 2; element 1 holds 0, 1, 2 and 7 — a label the keys (taken from element 0) do not list."""
    return [label_volume(shape, [0, 1, 2]).to(dtype), label_volume(shape, [0, 1, 2, 7], 1).to(dtype)]


#: name -> (seed, label-map elements, constructor keywords)
CASES = {
    "single_int16": (11, lambda: _elements(SHAPE_ODD, [0, 1, 2, 3], torch.int16, 1), {}),
    "batch3_per_instance_uint8": (12, lambda: _elements(SHAPE_ODD, [0, 1, 2, 5], torch.uint8, 3), {}),
    "batch2_shared_int32": (13, lambda: _elements(SHAPE_EVEN, [-3, 0, 4, 100000], torch.int32, 2), {"per_instance": False}),
    "ignore_background_int16": (14, lambda: _elements(SHAPE_ODD, [0, 1, 2], torch.int16, 2), {"ignore_background": True}),
    "ignore_background_shared_float32": (
        15, lambda: _elements(SHAPE_EVEN, [0, 1, 2], torch.float32, 2), {"ignore_background": True, "per_instance": False}),
    "short_lists_uint8": (
        16, lambda: _elements(SHAPE_ODD, [0, 1, 2, 3, 4], torch.uint8, 2),
        {"mean": [(0.8, 1.0), 0.5, (-0.2, 0.2)], "std": [(0.01, 0.05), (0.02, 0.08)], "default_std": (-0.1, -0.01)}),
    "non_integer_float32": (17, lambda: _elements(SHAPE_ODD, [0.0, 1.2, 1.7, 2.0, 3.0], torch.float32, 2), {}),
    "absent_label_int16": (18, lambda: _absent_label(SHAPE_ODD, torch.int16), {}),
    "absent_label_shared_int32": (19, lambda: _absent_label(SHAPE_EVEN, torch.int32), {"per_instance": False}),
    "two_channels_float32": (
        20, lambda: [torch.cat([label_volume(SHAPE_EVEN, [0, 1, 2], s), label_volume(SHAPE_EVEN, [3, 4], s)]).float() for s in range(2)], {}),
}


def make_batch(tio, name: str, device: str = "cpu"):
    """A subject with a scalar image in front of the label map (the label map is found by class, or by its key)."""
    elements = CASES[name][1]()
    subjects = [tio.Subject(t1=tio.ScalarImage(torch.zeros(1, *e.shape[1:])), seg=tio.LabelMap(e.clone())) for e in elements]
    batch = tio.SubjectsBatch.from_subjects(subjects)
    return batch.to(device) if device != "cpu" else batch


def construct(tio, name: str):
    return tio.LabelsToImage(label_key="seg" if "shared" in name else None, **CASES[name][2])


def draw_case(tio, name: str):
    """The global-generator half of the call alone — the gate draw, then ``make_params`` — and the generator's next draw."""
    transform = construct(tio, name)
    batch = make_batch(tio, name)
    torch.manual_seed(CASES[name][0])
    torch.rand(1)  # the p-gate (transform.py:227)
    params = transform.make_params(batch)
    return params, float(torch.rand(1))


def run_case(tio, name: str, device: str = "cpu"):
    """The case through ``tio`` (the reference or this package): ``(output batch, recorded params, history name, the next
    draw of the global generator)``."""
    seed = CASES[name][0]
    transform = construct(tio, name)
    batch = make_batch(tio, name, device)
    torch.manual_seed(seed)
    out = transform(batch)
    after = torch.rand(1)
    record = out.applied_transforms[-1]
    return out, record.params, record.name, after
