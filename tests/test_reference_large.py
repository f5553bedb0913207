"""The UNMODIFIED reference against ``torchio_amd`` + the CPU oracle well above the 24-voxel golden fixtures (VERDICT r1,
item 1c) — a six-transform Compose on a three-image subject at 96^3, where bricks, multi-pass boxes and the 256-wide blur
windows of the kernels' CPU restatement are all exercised.

The reference's side is recorded (``tests/golden/reference_recorded.pt``, written by
``tests/golden/make_golden_reference.py`` from the same inputs and seeds): the SHA-256 of every output that must match
bit for bit, and for the Compose's float images a fixed sample of voxels plus the sums over the whole volume.  Every voxel
of those float images is held to the bound through the oracle: the recorder compares the oracle's output with the
reference's at EVERY voxel and stores the SHA-256 of that checked output, which the test then requires.  CPU only.
"""
from __future__ import annotations

import contextlib
import hashlib
import os

import torch

from parity_harness import nested_spheres
from parity_harness import use_engine

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_recorded.pt")
SAMPLE_STRIDE = 13  # every 13th voxel of the flattened 96^3 volume (13 is prime to 96: every row and plane is visited)
SPATIAL_KWARGS = dict(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5), max_displacement=7.5, label_interpolation="label")


def _make(tio_module, size: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return tio_module.Subject(
        t1=tio_module.ScalarImage(torch.rand(1, size, size, size, generator=g)),
        t2=tio_module.ScalarImage(torch.rand(1, size, size, size, generator=g) + 1),
        seg=tio_module.LabelMap(nested_spheres(size)),
    )


def _compose(tio_module):
    return tio_module.Compose(
        [
            tio_module.Affine(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5)),
            tio_module.ElasticDeformation(),
            tio_module.BiasField(),
            tio_module.Blur(std=(0.5, 2)),
            tio_module.Noise(),
            tio_module.Gamma(log_gamma=(-0.3, 0.3)),
        ]
    )


def _engine(engine):
    return contextlib.nullcontext() if engine is None else use_engine(engine)


def run_compose(tio_module, engine):
    """The six-transform Compose at 96^3 (*engine* None: the module's own code, as for the reference)."""
    torch.manual_seed(4)
    with _engine(engine):
        return _compose(tio_module)(_make(tio_module, 96, 7))


def run_spatial(tio_module, engine):
    """The fused ``Spatial`` with ``label_interpolation="label"`` at 96^3."""
    torch.manual_seed(8)
    with _engine(engine):
        return tio_module.Spatial(**SPATIAL_KWARGS)(_make(tio_module, 96, 9))


def _sha256(tensor: torch.Tensor) -> str:
    return hashlib.sha256(tensor.detach().contiguous().numpy().tobytes()).hexdigest()


def record(subject, floats) -> dict:
    """What the tests keep of a result: per image its shape, dtype and SHA-256; for the images in *floats* also every
    ``SAMPLE_STRIDE``-th voxel, the float64 sum and sum of squares, and the bounds those sums may move by when every voxel
    stays within 5e-6 relative (to max(1, |value|))."""
    out = {}
    for name in ("t1", "t2", "seg"):
        data = subject[name].data
        entry = {"shape": list(data.shape), "dtype": str(data.dtype), "sha256": _sha256(data)}
        if name in floats:
            want = data.double().reshape(-1)
            scale = want.abs().clamp_min(1.0)
            entry.update({
                "sample": data.reshape(-1)[::SAMPLE_STRIDE].clone(),
                "sum": want.sum().item(), "sum_sq": (want * want).sum().item(),
                "sum_bound": scale.sum().item(), "sum_sq_bound": ((2 * want.abs() + 5e-6 * scale) * scale).sum().item(),
            })
        out[name] = entry
    return out


def check_every_voxel(reference, oracle_result, names=("t1", "t2")) -> dict:
    """The per-voxel bound over whole volumes (the recorder runs it on the reference's and the oracle's results): the largest
    relative error per image, which must be within 5e-6 (to max(1, |value|))."""
    worst = {}
    for name in names:
        want, got = reference[name].data.double(), oracle_result[name].data.double()
        assert want.shape == got.shape, (name, want.shape, got.shape)
        worst[name] = ((want - got).abs() / want.abs().clamp_min(1.0)).max().item()
        assert worst[name] <= 5e-6, (name, worst[name])
    return worst


def _recorded() -> dict:
    return torch.load(RECORDED, weights_only=True)


def _assert_same_layout(name, got, want):
    assert list(got.shape) == want["shape"] and str(got.dtype) == want["dtype"], (name, got.shape, got.dtype, want["shape"], want["dtype"])


def test_six_transform_compose_96_reference_vs_oracle(oracle):
    import torchio_amd as ours  # noqa: PLC0415

    expected = _recorded()["compose96"]
    actual = run_compose(ours, oracle)
    _assert_same_layout("seg", actual["seg"].data, expected["seg"])
    assert _sha256(actual["seg"].data) == expected["seg"]["sha256"], "label map differs from the reference"
    for name in ("t1", "t2"):
        want_entry, got = expected[name], actual[name].data
        _assert_same_layout(name, got, want_entry)
        want = want_entry["sample"].double()
        sample = got.reshape(-1)[::SAMPLE_STRIDE].double()
        rel = ((want - sample).abs() / want.abs().clamp_min(1.0)).max().item()
        assert rel <= 1e-4, (name, rel)   # north_star
        assert rel <= 5e-6, (name, rel)   # what the oracle delivers (libm exp / pow vs ATen's vectorised ones)
        # the whole volume: its sum and sum of squares move no further than 5e-6 relative per voxel allows
        whole = got.double().reshape(-1)
        slack = 1e-12 * whole.numel()  # (float64 summation order)
        assert abs(whole.sum().item() - want_entry["sum"]) <= 5e-6 * want_entry["sum_bound"] + slack, name
        assert abs((whole * whole).sum().item() - want_entry["sum_sq"]) <= 5e-6 * want_entry["sum_sq_bound"] + slack, name
        # every voxel: this output is the one the recorder checked against the reference's at every voxel
        assert _sha256(got) == want_entry["checked_oracle_sha256"], (
            f"{name}: the oracle's output is no longer the one checked voxel by voxel against the reference "
            "(tests/golden/make_golden_reference.py checks the new one and records it)")


def test_fused_spatial_with_label_mode_96_is_bit_exact(oracle):
    import torchio_amd as ours  # noqa: PLC0415

    expected = _recorded()["spatial96"]
    actual = run_spatial(ours, oracle)
    for name in ("t1", "t2", "seg"):
        _assert_same_layout(name, actual[name].data, expected[name])
        assert _sha256(actual[name].data) == expected[name]["sha256"], name
