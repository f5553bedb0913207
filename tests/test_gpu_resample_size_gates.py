"""GPU: ``tio_resample3d`` on both sides of the size gates of its dispatcher (resample.hip), where a call changes kernels.

| gate                                   | just inside                                 | just beyond                                  |
|----------------------------------------|---------------------------------------------|----------------------------------------------|
| ``I * J <= 2^24`` (``nn_enabled``)     | (4096, 4096, 3): the general nearest kernel | (4097, 4096, 3): the per-voxel gather kernel |
| ``K < 2^24`` (``nn_enabled``)          | uint8 (1, 2, 2^24 - 1): general nearest     | (1, 2, 2^24): the per-voxel gather kernel    |
| ``K * es < 2^24`` (``narrow``)         | int16 (2, 2, 2^23 - 1): general nearest     | (2, 2, 2^23): general nearest as well        |
| ``n * es < 2^32 - 16`` (``narrow``)    | int64 (511, 1024, 1024): the exact kernel   | int64 (513, 1024, 1024): the general kernel  |
| ``I * J * K < 2^30`` (the float roads) | (1024, 1024, 1023): the planned brick road  | (1024, 1024, 1024): the gather road          |

Which kernels these are (resample.hip: ``sort_images``, ``launch_nearest``): the two ``nn_enabled`` gates, the int64 byte gate and the
float gate change the kernel.  The other two do not, at the sizes that reach them: the exact-coordinate nearest kernel (24-bit
offsets, buffer loads) also needs rows of at least 48 voxels and the short division, i.e. a normalising extent of at most 8193
on every axis — a K of 3 has no such rows, and an axis of 2^23 voxels is normalised by itself — so both neighbours of
``K * es = 2^24`` run ``resample_nearest_kernel``, and so does the inside neighbour of ``I * J = 2^24``.  Those cases hold the
general kernel and the gather kernel to the analytic answer at the largest planes and the longest rows the dispatcher lets them see;
the narrow kernel's own limits are reached only through the byte gate.

Nearest cases are an integer translation plus flips: the whole output equals the analytic input at the shifted position (zero
outside), ``torch.equal``.  Trilinear cases sample the affine input under a small rotation and are held, voxel by voxel, to the
float64 value at the float64 coordinate within the bound derived in ``size_gate_cases.py``; ``test_size_gates_host.py`` shows on
the CPU that a wrapped source index breaks that bound.
"""
from __future__ import annotations

import pytest
import torch

import large_offset_cases as big
import size_gate_cases as gates

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    big.release()


def _nearest_ids():
    found = []
    for name, (_, dtype, _, _) in gates.NEAREST_CASES.items():
        found += [(name, d) for d in (gates.NEAREST_DTYPES if dtype is None else (dtype,))]
    return found


@pytest.mark.parametrize("name, dtype", _nearest_ids(), ids=[f"{name}-{str(dtype).split('.')[-1]}" for name, dtype in _nearest_ids()])
def test_nearest_on_both_sides_of_a_gate(hip, name, dtype):
    shape, _, shift, flips = gates.NEAREST_CASES[name]
    voxels = shape[0] * shape[1] * shape[2]
    big.needs_gib(4 * voxels * dtype.itemsize / 1024**3 + 1)
    data = gates.analytic_input(shape, dtype, "cuda")
    (out,) = hip.resample3d([data], out_shape=shape, mapping=gates.shift_flip_mapping(shape, shift, flips).cuda(), control_points=None,
                            in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True, interps=["nearest"], fills=[None], precision="exact")
    expected = gates.shifted(data, shift, flips)
    assert big.same(out, expected), f"{name}: {big.first_difference(out, expected)}"
    assert int((out != 0).sum()) > 0.25 * voxels  # (the shift leaves a third of a K of 3 and half of a J of 2 outside)


@pytest.mark.parametrize("name", sorted(gates.TRILINEAR_CASES))
def test_trilinear_on_both_sides_of_2_30_voxels(hip, name):
    from test_gpu_resample_planned import starts_from_a_plan

    channels, shape = gates.TRILINEAR_CASES[name]
    voxels = shape[0] * shape[1] * shape[2]
    big.needs_gib(3 * channels * voxels * 4 / 1024**3 + 6)
    data = big.affine_field((1, channels, *shape), "cuda", torch.float64).float()  # formed in float64, rounded once: half an ulp of f
    mapping = gates.rotation_mapping(shape)
    geometry = dict(out_shape=shape, mapping=mapping.cuda(), control_points=None, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True)
    # at 2^30 voxels no staged road is left (the planned ones among them); one row of K fewer and the call is planned again
    assert starts_from_a_plan(hip, [data], precision="exact", **geometry) == (voxels < 2**30)
    (out,) = hip.resample3d([data], **geometry, interps=["linear"], fills=[None], precision="exact")
    compared, planes = 0, 64
    for channel in range(channels):
        for begin in range(0, shape[0], planes):
            rows = slice(begin, min(begin + planes, shape[0]))
            f, bound, interior, _ = gates.trilinear_reference(mapping, shape, channel, rows, "cuda")
            error = (out[0, channel, rows].double() - f).abs()
            bad = interior & (error > bound)
            assert not bool(bad.any()), (f"{name}, channel {channel}, planes {rows}: {int(bad.sum())} voxels beyond the bound, "
                                         f"worst error / bound = {float((error / bound)[interior].max()):.3g}")
            compared += int(interior.sum())
    assert compared > 0.9 * channels * voxels
