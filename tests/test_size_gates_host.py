"""The library's size gates from the host side: no GPU call is made.

* ``tio_resample3d_plan_bytes`` runs the float route choice without a device: it is positive just under each limit of
  ``choose_float_road`` (resample.hip) and zero at it, everything else being equal.
* Every documented size refusal returns its status and names the limit in ``tio_last_error``.  The pointers are fakes
  (non-null, aligned, far apart): a refusal happens before anything is launched — on a machine without a GPU a launch would come
  back as ``TIO_ERR_LAUNCH`` (-4), which no case below accepts.  Refusals that other host tests already hold are not repeated here:
  the k-space artefact calls at 2^31 voxels per volume (``test_kspace_artefacts_host.py``) and ``tio_keep_largest_component``'s
  32-bit voxel indices (``test_label_transforms_host.py``).
* The trilinear reference of ``test_gpu_resample_size_gates.py`` has teeth: a source index wrapped modulo 2^30 elements or modulo
  2^32 bytes breaks its bound on 99 % or more of the voxels the wrap touches (``size_gate_cases.py``).
"""
from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

import size_gate_cases as gates
from torchio_amd import _abi, _lib

INVALID, UNSUPPORTED = -1, -5
SOME, OTHER, THIRD = (C.c_void_p(base) for base in (1 << 40, 1 << 44, 1 << 48))  # never dereferenced; 2^40 bytes and more apart
SWITCHES = ("TIO_FAST_KERNEL", "TIO_EXACT_LEAN", "TIO_EXACT_PLAN", "TIO_PLANNED_LEAN", "TIO_LEAN_MULTI", "TIO_RESAMPLE_PATH",
            "TIO_RESAMPLE_EXACT", "TIO_TILE_ABLATE", "TIO_NEAREST_KERNEL")


@pytest.fixture()
def fn():
    """The library's functions under its DEFAULT switches (restored afterwards)."""
    _, functions = _lib.load()
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}
    functions["reload_env"]()
    yield functions
    for name, value in saved.items():
        if value is not None:
            os.environ[name] = value
    functions["reload_env"]()


def _i32x3(values):
    return (C.c_int32 * 3)(*values)


def _geom(batch, in_shape, out_shape, precision=_abi.PRECISION_EXACT) -> _abi.ResampleGeom:
    geom = _abi.ResampleGeom()
    geom.batch = batch
    geom.in_shape[:] = in_shape
    geom.out_shape[:] = out_shape
    geom.affine_first = 1
    geom.mapping_dev = SOME.value
    geom.mapping_batched = 1
    geom.in_spacing[:] = geom.out_spacing[:] = (1.0, 1.0, 1.0)
    geom.precision = precision
    return geom


def _image(dtype=_abi.F32, interp=_abi.LINEAR):
    image = (_abi.ResampleImage * 1)()
    image[0].in_, image[0].out, image[0].channels, image[0].dtype, image[0].interp = OTHER.value, THIRD.value, 1, dtype, interp
    return image


# -- the float road's limits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [_abi.PRECISION_EXACT, _abi.PRECISION_TIGHT, _abi.PRECISION_FAST], ids=["exact", "tight", "fast"])
def test_the_staged_roads_end_at_2_30_input_voxels(fn, precision):
    """``I * J * K >= 2^30``: 32-bit byte offsets inside one float32 input channel end there (the brick DMA)."""
    out_shape = (256, 256, 256)  # 4096 bricks per element, 3 elements: the planned roads' 12 288
    at = fn["resample3d_plan_bytes"](C.byref(_geom(3, (1024, 1024, 1024), out_shape, precision)))
    # one plane fewer (K stays a multiple of 4: every precision's planned road) and one row of K fewer (1023 is no multiple of 4:
    # the FAST planned road needs 16-byte rows whatever the size, the exact ones fall back to the planned brick kernel)
    below = fn["resample3d_plan_bytes"](C.byref(_geom(3, (1023, 1024, 1024), out_shape, precision)))
    assert below > 0 and at == 0, (below, at)
    below_k = fn["resample3d_plan_bytes"](C.byref(_geom(3, (1024, 1024, 1023), out_shape, precision)))
    assert (below_k > 0) == (precision != _abi.PRECISION_FAST), below_k
    # one plane more, far from the limit in every other respect: still no plan
    assert fn["resample3d_plan_bytes"](C.byref(_geom(3, (1025, 1024, 1024), out_shape, precision))) == 0


@pytest.mark.parametrize("precision", [_abi.PRECISION_EXACT, _abi.PRECISION_TIGHT, _abi.PRECISION_FAST], ids=["exact", "tight", "fast"])
def test_the_staged_roads_end_at_an_output_plane_of_2_31_bytes(fn, precision):
    """``Jo * Ko * 8 >= 2^31``: 32-bit byte offsets inside one output plane."""
    in_shape = (64, 64, 64)
    below = fn["resample3d_plan_bytes"](C.byref(_geom(1, in_shape, (4, 16383, 16384), precision)))
    at = fn["resample3d_plan_bytes"](C.byref(_geom(1, in_shape, (4, 16384, 16384), precision)))
    assert below > 0 and at == 0, (below, at)
    bricks = 1 * 1024 * 1024
    assert below == (16 + 16 + bricks * 16) * 4  # [header] [batch x 16 floats] [bricks x 16-int descriptors]: test_plan_bytes_routes.py


# -- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(fn, status, expected, words, who):
    message = fn["last_error"]()
    assert status == expected, (who, status, message)
    assert who.encode() in message and all(word in message for word in words), message


def test_resample3d_refuses_2_31_voxels_per_channel(fn):
    for in_shape, out_shape in (((2048, 1024, 1024), (8, 8, 8)), ((8, 8, 8), (2048, 1024, 1024))):
        _refused(fn, fn["resample3d"](C.byref(_geom(1, in_shape, out_shape)), 1, _image(), None), INVALID, [b"2^31 voxels per channel"], "tio_resample3d")
    for interp, dtype in ((_abi.NEAREST, _abi.I16), (_abi.LABEL_PV, _abi.U8)):
        status = fn["resample3d"](C.byref(_geom(1, (2048, 1024, 1024), (8, 8, 8))), 1, _image(dtype, interp), None)
        _refused(fn, status, INVALID, [b"2^31 voxels per channel"], "tio_resample3d")
    # one row fewer is not refused for its size: the plan question is answered (by the gather road: no plan)
    assert fn["resample3d_plan_bytes"](C.byref(_geom(1, (2048, 1024, 1023), (8, 8, 8)))) == 0
    assert fn["resample3d_plan_bytes"](C.byref(_geom(1, (2048, 1024, 1024), (8, 8, 8)))) == 0


@pytest.mark.parametrize("interp, dtype", [(_abi.LINEAR, _abi.F32), (_abi.NEAREST, _abi.I16), (_abi.LABEL_PV, _abi.U8)], ids=["linear", "nearest", "label"])
def test_resample3d_refuses_a_grid_of_2_31_blocks(fn, interp, dtype):
    """Two 16^3 bricks per element (17 x 16 x 16 voxels) and 2^30 elements: 2^31 blocks, on every kernel's road (the per-voxel
    kernel of the label mode cuts other tiles: 2^30 elements of two of ITS tiles)."""
    out_shape = (17, 16, 16)
    status = fn["resample3d"](C.byref(_geom(1 << 30, (8, 8, 8), out_shape)), 1, _image(dtype, interp), None)
    _refused(fn, status, INVALID, [b"grid too large"], "tio_resample3d")


def test_geometry_grad_refuses_a_grid_of_2_31_blocks(fn):
    geom = _geom(1 << 30, (8, 8, 8), (17, 16, 16))
    nbytes = fn["resample3d_geometry_grad_workspace_bytes"](C.byref(geom))
    assert nbytes > 0
    status = fn["resample3d_geometry_grad"](C.byref(geom), 1, _image(), C.c_void_p(1 << 50), None, C.c_void_p(1 << 52), nbytes, None)
    _refused(fn, status, INVALID, [b"grid too large"], "tio_resample3d_geometry_grad")


def test_kspace_segment_mix_refuses_a_plane_of_2_31(fn):
    def run(shape, batch=1, channels=1):
        segments = (C.c_void_p * 2)(SOME.value, OTHER.value)
        bounds = (C.c_int32 * 3)(0, shape[0] // 2, shape[0])
        return fn["kspace_segment_mix"](segments, 2, bounds, THIRD, C.c_void_p(1 << 50), _abi.F32, batch, channels, _i32x3(shape), None, None)

    _refused(fn, run((4, 32768, 65536)), INVALID, [b"plane or batch*channels too large"], "tio_kspace_segment_mix")
    _refused(fn, run((4, 8, 8), batch=256, channels=257), INVALID, [b"plane or batch*channels too large"], "tio_kspace_segment_mix")


def test_points_warp_refuses_more_than_int32_max_points(fn):
    offsets = (C.c_int32 * 2)(0, 0)
    status = fn["points_warp"](SOME, OTHER, None, 1 << 31, offsets, THIRD, 1, C.c_void_p(1 << 50), None, 0, None)
    _refused(fn, status, INVALID, [b"2^31 - 1 points"], "tio_points_warp")


def test_conv_adjoint_refuses_a_tensor_beyond_its_block_limit(fn):
    """``ceil(total / 256) > 2^31 - 1`` blocks: 32768 x 8 elements of 2048^3 voxels are 2^51."""
    taps = (C.c_int32 * 3)(1, 1, 1)
    status = fn["separable_conv3d_adjoint"](SOME, OTHER, THIRD, 32768, 8, _i32x3((2048, 2048, 2048)), C.c_void_p(1 << 50), 0, 40, taps, None, None)
    _refused(fn, status, INVALID, [b"tensor too large"], "tio_separable_conv3d_adjoint")


def test_patch_gather_and_swap_refuse_a_patch_of_2_31_voxels(fn):
    volume, patch = (2048, 1024, 1024), (2048, 1024, 1024)
    status = fn["patch_gather"](SOME, OTHER, 1, 1, _i32x3(volume), _i32x3(patch), THIRD, 1, None)
    _refused(fn, status, UNSUPPORTED, [b"a patch of 2^31 voxels or more"], "tio_patch_gather")
    status = fn["swap_patches"](SOME, OTHER, 1, 1, 1, _i32x3(volume), _i32x3(patch), THIRD, C.c_void_p(1 << 50), 1, 1, None)
    _refused(fn, status, UNSUPPORTED, [b"a patch of 2^31 voxels or more"], "tio_swap_patches")
    for name in ("patch_gather", "swap_patches"):  # and both count at most 2^40 voxels
        huge = _i32x3((1 << 14, 1 << 14, 1 << 14))
        arguments = (SOME, OTHER, 1, 1, huge, _i32x3((1, 1, 1)), THIRD, 1, None) if name == "patch_gather" else \
                    (SOME, OTHER, 1, 1, 1, huge, _i32x3((1, 1, 1)), THIRD, C.c_void_p(1 << 50), 1, 1, None)
        _refused(fn, fn[name](*arguments), UNSUPPORTED, [b"2^40"], "tio_" + name)


def test_channel_pca_refuses_beyond_its_plan_limits(fn):
    plan = (C.c_int32 * 4)()
    voxels = (1 << 40) // 3 + 1
    _refused(fn, fn["channel_scatter_plan"](1, 3, voxels, plan), UNSUPPORTED, [b"2^40 elements"], "tio_channel_scatter_plan")
    assert fn["channel_scatter_workspace_bytes"](1, 3, voxels) == -1 and b"2^40 elements" in fn["last_error"]()
    aligned = [C.c_void_p(1 << shift) for shift in (50, 52, 54)]
    status = fn["channel_scatter"](SOME, 1, 3, voxels, *aligned, 1 << 40, None)
    _refused(fn, status, UNSUPPORTED, [b"2^40 elements"], "tio_channel_scatter")
    status = fn["channel_scatter"](SOME, 65536, 3, 16, *aligned, 1 << 40, None)
    _refused(fn, status, UNSUPPORTED, [b"65535"], "tio_channel_scatter")
    status = fn["channel_project"](SOME, 65536, 3, 16, OTHER, THIRD, aligned[0], 2, 0, aligned[1], None)
    _refused(fn, status, UNSUPPORTED, [b"65535"], "tio_channel_project")
    status = fn["channel_project"](SOME, 1, 3, voxels, OTHER, THIRD, aligned[0], 2, 0, aligned[1], None)
    _refused(fn, status, UNSUPPORTED, [b"2^40 elements"], "tio_channel_project")


# -- the large-offset helpers ------------------------------------------------------------------------------------------------------
def test_every_crossing_of_the_large_shapes_lies_inside_a_row():
    import large_offset_cases as big

    for dtype, wide, volume, wanted in ((torch.uint8, False, big.VOLUME, 2), (torch.float32, False, big.VOLUME, 2), (torch.float32, True, big.VOLUME, 3),
                                        (torch.float32, False, big.STENCIL_VOLUME, 2)):
        shape = big.shape_for(dtype, wide, volume)
        found = big.crossings(shape, dtype)  # (asserts 0 < k < K - 1 itself)
        assert len(found) == wanted and volume[2] % 4 == 0
        per_element = shape[1] * volume[0] * volume[1] * volume[2]
        assert per_element * 4 < big.SLICE_LIMIT  # one batch element as float32 stays below 2^31 bytes: a batch slice (`batch_step`) can be cut there
        for name, start, stop in big.windows(shape, dtype):
            assert 0 <= start < stop <= per_element * shape[0] and stop - start <= big.WINDOW, name
    small = (3, 2, 4, 5, 6)
    data = big.distinct(small, torch.uint8, "cpu")
    assert torch.equal(big.distinct((1, 2, 4, 5, 6), torch.uint8, "cpu", first_slice=2), data[1:2])
    assert big.batch_step(torch.empty((4, 1, 8, 8, 2**20), dtype=torch.uint8, device="meta"), 4) == 7  # 2^28 bytes of float32 per element
    field = big.affine_field(small, "cpu", torch.float64)
    assert float(field[2, 1, 3, 4, 5]) == pytest.approx(5 + 3 / 4 + 2 * 4 / 5 + 4 * 5 / 6)


# -- the analytic expectation of the long-axis cases is the reference chain's -------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_int16_2_23", "k_uint8_2_24"])
def test_the_oracle_gives_the_analytic_shift_on_a_long_axis(oracle, name):
    """At coordinates of 2^23 and 2^24 float32 holds integers only: the reference's coordinate chain must land on the right one.
    The CPU oracle (64-bit indices throughout) says it does, bit for bit; the GPU test asks the same of the device."""
    shape, dtype, shift, flips = gates.NEAREST_CASES[name]
    data = gates.analytic_input(shape, dtype, "cpu")
    (out,) = oracle.resample3d([data], out_shape=shape, mapping=gates.shift_flip_mapping(shape, shift, flips), control_points=None, in_spacing=(1, 1, 1),
                               out_spacing=(1, 1, 1), affine_first=True, interps=["nearest"], fills=[None], precision="exact")
    assert torch.equal(out, gates.shifted(data, shift, flips))


# -- the trilinear reference of the size-gate tests has teeth -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gates.TRILINEAR_CASES))
def test_a_wrapped_source_index_breaks_the_trilinear_bound(name):
    for wrap in ("2^30 elements", "2^32 bytes"):
        touched, broken = gates.simulated_wrap(name, wrap)
        assert touched >= 1000, (name, wrap, touched)
        assert broken >= 0.99 * touched, f"{name}, wrapped modulo {wrap}: {broken} of {touched} touched voxels break the bound"
