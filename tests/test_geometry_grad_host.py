"""Host side of the geometry gradient (``tio_resample3d_geometry_grad``): the ABI as ``ctypes`` sees it, the argument checks, the
fake kernel of the custom op, the public ``warp``, and the test reference itself - ``geometry_grad_reference``'s analytic restatement
against plain float64 autograd, and the conditions under which its kink allowance means anything, for every case the GPU tests use."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

import geometry_grad_reference as reference
import torchio_amd as tio
from torchio_amd import _abi
from torchio_amd import _lib


def test_the_header_declares_both_entry_points():
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    expected = {
        "resample3d_geometry_grad_workspace_bytes": (i64, [C.POINTER(_abi.ResampleGeom)]),
        "resample3d_geometry_grad": (C.c_int, [C.POINTER(_abi.ResampleGeom), i32, C.POINTER(_abi.ResampleImage), vp, vp, vp, i64, vp]),
    }
    for name, prototype in expected.items():
        assert _abi.HIP_ONLY_PROTOTYPES[name] == prototype, name
        assert name not in _abi.PROTOTYPES and "tio_" + name in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 18


def _valid_call():
    buffers = [C.create_string_buffer(1 << 16) for _ in range(6)]
    p = [C.c_void_p((C.addressof(b) + 15) & ~15) for b in buffers]
    geom = _abi.ResampleGeom()
    geom.batch = 1
    geom.in_shape[:] = geom.out_shape[:] = [4, 4, 4]
    geom.in_spacing[:] = geom.out_spacing[:] = [1.0, 1.0, 1.0]
    geom.mapping_dev = p[0]
    image = (_abi.ResampleImage * 1)()
    image[0].in_, image[0].out, image[0].channels, image[0].dtype, image[0].interp = p[1], p[2], 1, _abi.F32, _abi.LINEAR
    return buffers, p, geom, image


def test_the_library_checks_its_arguments_without_a_gpu():
    _, f = _lib.load()
    keep, p, geom, image = _valid_call()
    call, size = f["resample3d_geometry_grad"], f["resample3d_geometry_grad_workspace_bytes"]
    nbytes = size(C.byref(geom))
    assert nbytes > 0 and nbytes % 8 == 0
    geom.control_points_dev, geom.cp_shape[:] = p[5], [3, 4, 5]
    assert size(C.byref(geom)) == nbytes + 3 * 4 * 5 * 3 * 8
    geom.cp_batched, geom.batch = 1, 3
    geom.mapping_batched = 1
    assert size(C.byref(geom)) == 3 * nbytes + 3 * 3 * 4 * 5 * 3 * 8
    assert size(None) == 0 and b"null" in f["last_error"]()
    keep, p, geom, image = _valid_call()

    def refused(status, word, *, n_images=1, images=image, d_mapping=p[3], d_control=None, workspace=p[4], workspace_bytes=nbytes):
        assert call(C.byref(geom), n_images, images, d_mapping, d_control, workspace, workspace_bytes, None) == status, f["last_error"]()
        assert b"tio_resample3d" in f["last_error"]() and word in f["last_error"](), f["last_error"]()

    assert call(None, 1, image, p[3], None, p[4], nbytes, None) == -1 and b"null" in f["last_error"]()
    refused(-1, b"null", images=None)
    refused(-1, b"n_images", n_images=0)
    refused(-1, b"n_images", n_images=_abi.MAX_IMAGES + 1)
    refused(-1, b"neither", d_mapping=None)
    refused(-1, b"without control points", d_control=p[5])
    refused(-1, b"workspace", workspace=None)
    refused(-1, b"workspace", workspace_bytes=nbytes - 8)
    refused(-1, b"aligned", workspace=C.c_void_p(p[4].value + 4))
    image[0].interp = _abi.NEAREST
    refused(-1, b"TIO_LINEAR")
    image[0].interp = _abi.LINEAR_ADJOINT
    refused(-1, b"TIO_LINEAR")
    image[0].interp = _abi.LINEAR
    for dtype, status in ((_abi.I16, -2), (_abi.U8, -2), (99, -2), (-1, -2)):
        image[0].dtype = dtype
        refused(status, b"dtype" if dtype in (99, -1) else b"floating-point")
    image[0].dtype = _abi.F32
    image[0].channels = 0
    refused(-1, b"channels")
    image[0].channels = 1
    image[0].out = None
    refused(-1, b"null data")
    image[0].out = p[2]
    geom.out_shape[1] = 0
    refused(-1, b"shapes")
    geom.out_shape[1] = 4
    geom.mapping_dev = None
    refused(-1, b"mapping_dev")
    del keep


def test_the_fake_kernel_gives_the_shapes_of_the_geometry():
    import torchio_amd.torch_ops  # noqa: F401, PLC0415
    from torch._subclasses.fake_tensor import FakeTensorMode  # noqa: PLC0415

    with FakeTensorMode():
        x, g = torch.empty(2, 3, 6, 5, 8, device="cuda"), torch.empty(2, 3, 5, 7, 6, device="cuda")
        mapping, control = torch.empty(2, 3, 4, device="cuda", dtype=torch.float64), torch.empty(1, 4, 5, 6, 3, device="cuda")
        d_mapping, d_control = torch.ops.tio_hip.resample3d_geometry_grad([x], [g], mapping, control, [1, 1, 1], [1, 1, 1], [5, 7, 6], True, [None])
        assert d_mapping.shape == (2, 3, 4) and d_mapping.dtype == torch.float32 and d_mapping.device.type == "cuda"
        assert d_control.shape == (1, 4, 5, 6, 3) and d_control.dtype == torch.float32
        d_mapping, d_control = torch.ops.tio_hip.resample3d_geometry_grad([x], [g], mapping, None, [1, 1, 1], [1, 1, 1], [5, 7, 6], True, [None])
        assert d_mapping.shape == (2, 3, 4) and d_control.numel() == 0


def test_warp_is_exported():
    import inspect  # noqa: PLC0415

    assert "warp" in tio.__all__ and callable(tio.warp)
    parameters = inspect.signature(tio.warp).parameters
    assert list(parameters) == ["data", "mapping", "control_points", "out_shape", "in_spacing", "out_spacing", "affine_first", "fill"]
    assert parameters["control_points"].default is None and parameters["affine_first"].default is True
    with pytest.raises(ValueError, match=r"\(B, C, I, J, K\)"):
        tio.warp(torch.zeros(4, 4, 4), torch.eye(3, 4))


def test_lerp_matrix_is_the_align_corners_upsampling():
    for nodes, out in ((4, 7), (7, 128), (4, 4), (2, 1), (5, 3)):
        weights, error = reference.lerp_matrix(nodes, out)
        coarse = torch.randn(1, 1, nodes, 1, 1, dtype=torch.float64)
        fine = torch.nn.functional.interpolate(coarse, size=(out, 1, 1), mode="trilinear", align_corners=True)
        torch.testing.assert_close(weights @ coarse.reshape(nodes), fine.reshape(out), rtol=0, atol=1e-14)
        assert bool((error[weights > 0] > 0).all()) or nodes == out


@pytest.mark.parametrize("name", reference.CASE_NAMES)
def test_the_analytic_restatement_equals_float64_autograd_and_the_case_meets_its_conditions(name):
    case = reference.case(name)
    restated, (d_mapping, d_control) = case["analytic"], case["reference"]
    scale = float(restated["A_mapping"].max())
    assert scale > 0
    torch.testing.assert_close(restated["mapping"], d_mapping, rtol=0, atol=1e-12 * scale)
    assert bool((restated["A_mapping"] + 1e-300 >= restated["mapping"].abs() * (1 - 1e-12)).all())
    if d_control is not None:
        torch.testing.assert_close(restated["control"], d_control, rtol=0, atol=1e-12 * float(restated["A_control"].max()))
        assert bool((restated["A_control"] + 1e-300 >= restated["control"].abs() * (1 - 1e-12)).all())
    assert float(d_mapping.abs().max()) > 0
    reference.conditions(case)


def test_flags_and_degenerate_axes_are_exact_zeros_in_the_reference():
    flags = reference.case("4-flags")
    assert bool((flags["reference"][0][2] == 0).all()) and bool((flags["reference"][1][1:] == 0).all())
    assert bool((flags["reference"][0][1] != 0).any())  # cp_skip: the mapping of that element still has its gradient
    flat = reference.case("7-two-dimensional")
    assert bool((flat["reference"][0][:, 0] == 0).all()) and bool((flat["reference"][1][..., 0] == 0).all())
    assert bool((flat["analytic"]["R_mapping"][:, 0] == 0).all()) and bool((flat["analytic"]["R_control"][..., 0] == 0).all())
