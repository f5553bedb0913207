"""Ghosting / Spike without a GPU: argument checks of the three new entry points (nothing is launched), the draw order of
``make_params`` against the reference's recorded parameters, constructors / warnings / history, the host-side frequency
lists against a brute-force mask, and the golden file (the reference's own outputs,
``tests/golden/make_golden_kspace_artefacts.py``) against the float64 FFT-route restatements of ``kspace_artefact_cases.py``
that the GPU tests compare the engine with — and those against the closed forms the kernels compute."""
from __future__ import annotations

import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import kspace_artefact_cases as cases
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib
from torchio_amd.transforms import ghosting
from torchio_amd.transforms import spike

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kspace_artefacts_golden.pt")
SOME = ctypes.c_void_p(4096)  # non-null, 16-byte aligned pointers no check dereferences
OTHER = ctypes.c_void_p(1 << 30)
NEW = ("kspace_ghost_lines", "complex_abs_max", "kspace_add_spikes")


@pytest.fixture(scope="module")
def fn():
    return _lib.load()[1]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)["cases"]


def _i3(*values):
    return (ctypes.c_int32 * 3)(*values)


# -- the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_hip_only_and_the_abi_number_stays(fn):
    assert _abi.ABI_VERSION >= 17 and fn["abi_version"]() == _abi.ABI_VERSION  # (these entry points: since 17)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "tio_hip.h")).read()
    for name in NEW:
        assert name in _abi.HIP_ONLY_PROTOTYPES and name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
        assert f"tio_{name}(" in header
    for where in ("ghosting.py:218-277", ":149-215 _add_ghosting_per_element", "spike.py:152", "spike.py:124-162", ":165-223 _add_spikes_per_instance"):
        assert where in header  # each entry names the reference lines it replaces
    assert "CONTRACT: finite input" in header


def test_ghost_lines_refuses_bad_arguments(fn):
    call = fn["kspace_ghost_lines"]

    def run(x=SOME, y=OTHER, dtype=_abi.F32, batch=2, channels=1, shape=(5, 6, 7), mask=1, params=SOME, words=20, max_count=4, tables=SOME,
            active=None):
        return call(x, y, dtype, batch, channels, _i3(*shape), mask, params, words, max_count, tables, active, None)

    assert run(x=None) == -1 and b"null data" in fn["last_error"]()
    assert run(y=None) == -1
    assert run(params=None) == -1 and b"null parameters or tables" in fn["last_error"]()
    assert run(tables=None) == -1
    assert run(dtype=9) == -2 and b"dtype" in fn["last_error"]()
    assert run(batch=-1) == -1 and run(shape=(5, -6, 7)) == -1 and run(max_count=-1) == -1 and b"negative" in fn["last_error"]()
    assert run(mask=0) == -1 and b"names no axis" in fn["last_error"]()
    assert run(mask=8) == -1 and b"bits 0 to 2" in fn["last_error"]()
    assert run(words=7) == -1 and b"parameter words" in fn["last_error"]()
    assert run(y=SOME) == -1 and b"overlaps" in fn["last_error"]()
    assert run(x=ctypes.c_void_p(4098)) == -1 and b"aligned" in fn["last_error"]()
    assert run(tables=ctypes.c_void_p(4100)) == -1 and b"not aligned" in fn["last_error"]()
    assert run(shape=(5, 40000, 7)) == -5 and b"at most 32768" in fn["last_error"]()
    assert run(shape=(2048, 2048, 2048)) == -5 and b"2^31" in fn["last_error"]()
    assert run(batch=70000) == -5 and b"65535" in fn["last_error"]()
    assert run(x=None, y=None, batch=0) == 0 and run(x=None, y=None, shape=(0, 6, 7)) == 0  # nothing to do


def test_complex_abs_max_refuses_bad_arguments(fn):
    call = fn["complex_abs_max"]
    assert call(None, 2, 8, OTHER, None) == -1 and b"null input" in fn["last_error"]()
    assert call(SOME, 2, 8, None, None) == -1 and b"null output" in fn["last_error"]()
    assert call(SOME, -1, 8, OTHER, None) == -1 and call(SOME, 2, -8, OTHER, None) == -1 and b"negative" in fn["last_error"]()
    assert call(ctypes.c_void_p(4100), 2, 8, OTHER, None) == -1 and b"complex64" in fn["last_error"]()
    assert call(SOME, 2, 8, ctypes.c_void_p(4098), None) == -1 and b"not aligned" in fn["last_error"]()
    assert call(SOME, 70000, 8, OTHER, None) == -5 and b"65535" in fn["last_error"]()
    assert call(SOME, 4, 1 << 39, OTHER, None) == -5 and b"2^40" in fn["last_error"]()
    assert call(None, 0, 8, None, None) == 0


def test_add_spikes_refuses_bad_arguments(fn):
    call = fn["kspace_add_spikes"]

    def run(x=SOME, y=OTHER, dtype=_abi.I16, batch=2, channels=1, shape=(5, 6, 7), params=SOME, words=20, max_count=4, tables=SOME, peaks=SOME,
            active=None):
        return call(x, y, dtype, batch, channels, _i3(*shape), params, words, max_count, tables, peaks, active, None)

    for name in ("params", "tables", "peaks"):
        assert run(**{name: None}) == -1 and b"null parameters, tables or peaks" in fn["last_error"]()
    assert run(x=None) == -1 and run(y=None) == -1 and b"null data" in fn["last_error"]()
    assert run(dtype=12) == -2
    assert run(channels=-1) == -1 and run(max_count=-1) == -1 and b"negative" in fn["last_error"]()
    assert run(words=3) == -1 and b"parameter words" in fn["last_error"]()
    assert run(peaks=ctypes.c_void_p(4098)) == -1 and b"not aligned" in fn["last_error"]()
    assert run(x=ctypes.c_void_p(4097)) == -1 and b"aligned to its element" in fn["last_error"]()
    assert run(y=ctypes.c_void_p(4096 + 2 * 100)) == -1 and b"overlaps" in fn["last_error"]()
    assert run(shape=(40000, 1, 1)) == -5
    assert run(x=None, y=None, batch=0) == 0


def test_engine_refuses_bad_arguments_before_any_launch():
    """On host tensors: shape, list and dtype errors are ``ValueError``; a well-formed call is refused as a CPU tensor."""
    from torchio_amd import ops

    engine = ops.Engine(_lib.load()[1], "cuda", "hip")
    data = torch.zeros(2, 1, 4, 5, 6)
    with pytest.raises(ValueError, match=r"ghost_lines: expected a \(B, C, I, J, K\) tensor"):
        engine.ghost_lines(data[0], 0, 0.5, [0])
    with pytest.raises(ValueError, match="ghost_lines: axes: 3 entries for a batch of 2"):
        engine.ghost_lines(data, [0, 1, 2], 0.5, [0])
    with pytest.raises(ValueError, match="ghost_lines: frequency_lists: 3 lists for a batch of 2"):
        engine.ghost_lines(data, 0, 0.5, [[0], [1], [2]])
    with pytest.raises(ValueError, match=r"ghost_lines: axis 3 \(0, 1 or 2\)"):
        engine.ghost_lines(data, 3, 0.5, [0])
    with pytest.raises(ValueError, match=r"ghost_lines: a frequency outside \[0, 5\) along axis 1"):
        engine.ghost_lines(data, 1, 0.5, [5])
    with pytest.raises(ValueError, match="ghost_lines: active must hold 2 uint8/bool flags"):
        engine.ghost_lines(data, 1, 0.5, [1], active=torch.ones(3, dtype=torch.uint8))
    with pytest.raises(ops.EngineError, match="ghost_lines: tensor on cpu"):
        engine.ghost_lines(data, 1, 0.5, [1])
    with pytest.raises(ValueError, match=r"spectrum_peak: expected a \(B, C, I, J, K\) tensor"):
        engine.spectrum_peak(data[0])
    with pytest.raises(ops.EngineError, match="spectrum_peak: tensor on cpu"):
        engine.spectrum_peak(data)
    peaks = torch.ones(2)
    with pytest.raises(ValueError, match=r"add_spikes: \(1, 2, 6\) is not a frequency triple inside \(4, 5, 6\)"):
        engine.add_spikes(data, [(1, 2, 6)], 1.0, peaks)
    with pytest.raises(ValueError, match="add_spikes: intensities: 1 entries for a batch of 2"):
        engine.add_spikes(data, [(1, 2, 3)], [1.0], peaks)
    with pytest.raises(ValueError, match="add_spikes: frequency_lists: 1 lists for a batch of 2"):
        engine.add_spikes(data, [[(1, 2, 3)]], 1.0, peaks)
    with pytest.raises(ValueError, match="add_spikes: peaks must hold 2 float32 values"):
        engine.add_spikes(data, [(1, 2, 3)], 1.0, torch.ones(3))
    with pytest.raises(ValueError, match="add_spikes: peaks must hold 2 float32 values"):
        engine.add_spikes(data, [(1, 2, 3)], 1.0, peaks.double())
    with pytest.raises(ops.EngineError, match="add_spikes: tensor on cpu"):
        engine.add_spikes(data, [(1, 2, 3)], 1.0, peaks)


# -- parameters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CASES)
def test_make_params_draws_in_the_reference_order(golden, name):
    """On a CPU batch, without an engine: the constructor's warning, the gate draw, then ``make_params`` — the recorded
    parameters of the reference for the shared, the per-instance and the gated cases."""
    transform, built = cases.construct(tio, name)
    assert built == golden[name]["built"]
    batch = cases.make_batch(tio, cases.case_input(name))
    torch.manual_seed(cases.case_seed(name))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if not transform._per_instance_p_active(batch):
            torch.rand(1)  # the batch-wide gate of `forward`
        params = transform.make_params(batch)
    assert params == golden[name]["params"]
    assert [str(w.message) for w in caught] == golden[name]["warnings"] == []
    assert golden[name]["name"] == type(transform).__name__


def test_golden_parameter_geometry(golden):
    assert "_batched_keys" not in golden["ghost_shared"]["params"] and "_batched_keys" not in golden["spike_shared"]["params"]
    gated = golden["ghost_gated"]["params"]
    assert gated["_batched_keys"] == ["num_ghosts", "axis", "intensity"] and gated["_batch_size"] == 6
    assert [n == 0 and s == 0.0 for n, s in zip(gated["num_ghosts"], gated["intensity"], strict=True)] == [not keep for keep in gated["_keep"]]
    gated = golden["spike_gated"]["params"]
    assert gated["_batched_keys"] == ["positions", "intensity"]
    assert [p == [] and s == 0.0 for p, s in zip(gated["positions"], gated["intensity"], strict=True)] == [not keep for keep in gated["_keep"]]
    counts = [len(p) for p in golden["spike_per_instance"]["params"]["positions"]]
    assert all(1 <= n <= 6 for n in counts) and len(set(counts)) > 1
    assert any(s < 0 for s in golden["spike_per_instance"]["params"]["intensity"])


def test_constructors_warnings_and_history():
    ghost, spikes = tio.Ghosting(intensity=0.5), tio.Spike(intensity=1.0)
    assert ghost.axes == (0, 1, 2) and ghost.restore is None and not ghost.invertible
    assert ghost.supports_per_instance_params and ghost.supports_per_instance_p and spikes.supports_per_instance_params and spikes.supports_per_instance_p
    assert ghost.num_ghosts.is_constant(4.0) and spikes.num_spikes.is_constant(1.0) and not spikes.invertible
    assert tio.transforms.Ghosting is tio.Ghosting and tio.transforms.Spike is tio.Spike and {"Ghosting", "Spike"} <= set(tio.__all__)
    for make, hint in ((tio.Ghosting, r"intensity=\(0.5, 1\)"), (tio.Spike, r"intensity=\(1, 3\)")):
        with pytest.warns(UserWarning, match=f"{make.__name__} is a no-op with the given parameters.*{hint}"):
            make()
    with pytest.warns(UserWarning, match="Ghosting is a no-op"):
        tio.Ghosting(intensity=0.5, num_ghosts=0)
    with pytest.warns(UserWarning, match="Spike is a no-op"):
        tio.Spike(intensity=0.5, num_spikes=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tio.Ghosting(intensity=(0.0, 1.0))
        tio.Spike(intensity=(-1.0, 1.0))  # Spike's intensity may be negative ...
    with pytest.raises(ValueError, match="non-negative"):
        tio.Ghosting(intensity=-0.5)  # ... Ghosting's may not
    with pytest.raises(ValueError, match="non-negative"):
        tio.Ghosting(intensity=0.5, num_ghosts=-1)
    with pytest.raises(ValueError, match="non-negative"):
        tio.Spike(intensity=0.5, num_spikes=(-2, 3))
    with pytest.raises(ValueError, match="Probability must be in"):
        tio.Spike(intensity=0.5, p=1.5)


@pytest.mark.parametrize("name", ["ghost_noop", "spike_noop"])
def test_a_noop_returns_the_input_object_and_is_recorded(golden, name):
    """Nothing active: no engine is needed, the image tensor is the object that came in, the history has the entry."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        transform = cases.case_transform(tio, name)
    transform.copy = False
    batch = cases.make_batch(tio, cases.case_input(name))
    before = batch.images["t1"].data
    torch.manual_seed(cases.case_seed(name))
    out = transform(batch)
    assert out.images["t1"].data is before and torch.equal(before, golden[name]["out"])
    assert out.applied_transforms[-1].name == golden[name]["name"] and out.applied_transforms[-1].params == golden[name]["params"]


# -- the host halves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restore", [None, 0.02, 0.5, 1.0, 1.5])
@pytest.mark.parametrize("size", [1, 2, 7, 16, 33])
def test_ghost_frequencies_match_a_brute_force_mask(size, restore):
    for num_ghosts in (1, 4, size, size + 50):
        fraction = 0.0 if restore is None else restore
        scaled = cases.brute_force_scaled(size, num_ghosts, fraction)
        assert np.nonzero(ghosting.ghost_line_mask(size, num_ghosts, fraction))[0].tolist() == scaled
        frequencies = ghosting.ghost_frequencies(size, num_ghosts, fraction)
        assert frequencies == [(u - size // 2) % size for u in scaled] and all(0 <= f < size for f in frequencies)
        # the shifted spectrum holds frequency f at index (f + size // 2) mod size: numpy's own convention
        shifted_frequencies = np.fft.fftshift(np.arange(size))
        assert [int(shifted_frequencies[u]) for u in scaled] == frequencies
        mask = cases.mask_from_frequencies(size, frequencies, 0.25)
        assert np.array_equal(mask, cases.reference_line_mask(size, num_ghosts, 0.25, fraction, float32_mask=False))
    if restore is None:
        assert 0 in cases.brute_force_scaled(size, 4, 0.0)  # `restore=None` restores nothing (ghosting.py:74, :193)
    if restore == 1.5 and size == 16:  # the window [8 - 12, 8 + 12) = [-4, 20): the slice [12, 16)
        assert cases.brute_force_scaled(16, 4, 1.5) == [0, 4, 8]


def test_mask_strength_is_what_the_float32_mask_removes():
    for strength in (0.05, 0.7, 0.5645329356193542, 1.0):
        assert ghosting._mask_strength(strength) == 1.0 - float(np.float32(1.0 - strength))
        assert abs(ghosting._mask_strength(strength) - strength) <= 2.0**-24
    assert ghosting._mask_strength(0.5) == 0.5 and ghosting._mask_strength(1.0) == 1.0


def test_spike_positions_become_unshifted_frequencies():
    shape = (5, 8, 1)
    positions = [[0.0, 0.0, 0.0], [0.999999, 0.5, 0.7], [0.5, 0.49, 0.0], [1.0, 0.126, 0.3]]
    indices = [(0, 0, 0), (4, 4, 0), (2, 3, 0), (0, 1, 0)]  # int(p * s) % s: a position of exactly 1 wraps
    assert cases.shifted_indices(positions, shape) == indices
    frequencies = spike.spike_frequencies(positions, shape)
    assert frequencies == [(3, 4, 0), (2, 0, 0), (0, 7, 0), (3, 5, 0)] == cases.unshifted(indices, shape)
    for (i, j, k), (f0, f1, f2) in zip(indices, frequencies, strict=True):  # numpy's own shift agrees
        assert (np.fft.fftshift(np.arange(5))[i], np.fft.fftshift(np.arange(8))[j], np.fft.fftshift(np.arange(1))[k]) == (f0, f1, f2)


# -- the restatements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CASES)
def test_the_fft_route_restatement_reproduces_the_reference(golden, name):
    entry = golden[name]
    image = cases.case_input(name)
    assert entry["out"].dtype == image.dtype
    cases.check(entry["out"], cases.expected_for(name, entry["params"]), name)


def _closed_form_ghost(line: np.ndarray, frequencies, strength: float) -> np.ndarray:
    """What the kernel computes, in float64, for lines along the LAST axis."""
    size = line.shape[-1]
    at = np.arange(size)
    out = line.copy()
    for f in frequencies:
        angle = 2 * np.pi * ((f * at) % size) / size
        a, b = (line * np.cos(angle)).sum(-1, keepdims=True), (line * np.sin(angle)).sum(-1, keepdims=True)
        out -= strength / size * (np.cos(angle) * a + np.sin(angle) * b)
    return out


@pytest.mark.parametrize("axis", cases.AXES)
def test_closed_form_ghosting_equals_the_fft_route(axis):
    image = cases.signed_image((1, 2, 6, 9, 7), 3)
    size = image.shape[2 + axis]
    for frequencies in ([0], [1, size - 1, 2], list(range(size)), [3, 3]):
        expected = cases.ghost_fft(image, [axis], [cases.mask_from_frequencies(size, frequencies, 0.6)])
        lines = np.moveaxis(image.double().numpy(), 2 + axis, -1)
        got = np.moveaxis(_closed_form_ghost(lines, frequencies, 0.6), -1, 2 + axis)
        assert np.abs(got - expected).max() <= 1e-12 * np.abs(expected).max()


def test_closed_form_spikes_equal_the_fft_route():
    image = cases.signed_image((2, 2, 6, 9, 7), 4)
    shape = tuple(image.shape[2:])
    indices = [[(1, 2, 3), (5, 8, 0), (1, 2, 3)], [(3, 4, 3)]]  # a duplicate; the second element's is the DC term
    intensities = [1.5, -0.7]
    expected, peaks = cases.spike_fft(image, indices, intensities)
    assert cases.unshifted(indices[1], shape) == [(0, 0, 0)]
    grids = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    got = image.double().numpy().copy()
    for b in range(2):
        waves = sum(np.cos(2 * np.pi * sum(f * g / s for f, g, s in zip(triple, grids, shape, strict=True))) for triple in cases.unshifted(indices[b], shape))
        got[b] += peaks[b].reshape(-1, 1, 1, 1) * intensities[b] / np.prod(shape) * waves
    assert np.abs(got - expected).max() <= 1e-12 * np.abs(expected).max()
    assert not np.allclose(peaks, np.abs(image.double().sum((-3, -2, -1)).numpy()))  # signed input: the peak is not the DC term
