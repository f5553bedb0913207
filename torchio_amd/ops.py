"""Tensor-facing wrappers over the C ABI (``include/tio_hip.h``).

PyTorch is plumbing here: it owns device memory (outputs come from the caching
allocator), the current HIP stream and nothing else.  Every function marshals
``torch.Tensor`` arguments into raw pointers and calls one ``tio_*`` entry point
on the tensor's device and the current stream.  Inputs are never modified and
outputs never alias inputs (callers with ``copy=False`` may alias user data,
reference transform.py:220-221).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from collections.abc import Sequence
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _abi
from . import _lib
# The side streams (streams.py) and the reference's noise stream (noise_stream.py) are modules of their own; their public
# names — and the error type and autograd helpers they share with the engine — are read through `ops` as well.
from ._autograd import _AttachBackward
from ._autograd import _AttachBackwardMany
from ._autograd import _AttachGeometryBackward
from ._autograd import _AttachParameterBackward
from ._autograd import _wants_grad
from ._lib import EngineError
from .noise_stream import HostNormalStream
from .noise_stream import get_noise_plan
from .noise_stream import noise_plan_on_device
from .noise_stream import set_noise_plan
from .streams import Ahead
from .streams import ahead_stream
from .streams import calibrate_draw_policy
from .streams import draw_stream
from .streams import get_draw_policy
from .streams import note_resample_launch
from .streams import on_draw_stream
from .streams import set_ahead_stream
from .streams import set_draw_policy

HostNormalStream._torch = staticmethod(lambda: torch)  # (this module's `torch`, whatever it is when the stream allocates)

_DTYPE_CODES = {
    torch.float32: _abi.F32,
    torch.float64: _abi.F64,
    torch.float16: _abi.F16,
    torch.bfloat16: _abi.BF16,
    torch.uint8: _abi.U8,
    torch.int8: _abi.I8,
    torch.int16: _abi.I16,
    torch.int32: _abi.I32,
    torch.int64: _abi.I64,
}
FLOAT_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
INTERP_CODES = {
    "nearest": _abi.NEAREST, "linear": _abi.LINEAR, "label": _abi.LABEL_PV, "linear_adjoint": _abi.LINEAR_ADJOINT,
    "quadratic": _abi.QUADRATIC, "cubic": _abi.CUBIC,  # the image handed over holds B-spline coefficients (bspline_prefilter)
    "fourth": _abi.BSPLINE4, "fifth": _abi.BSPLINE5, "sixth": _abi.BSPLINE6, "seventh": _abi.BSPLINE7,
}


PRECISION_CODES = {"exact": _abi.PRECISION_EXACT, "fast": _abi.PRECISION_FAST, "tight": _abi.PRECISION_TIGHT}
_RESAMPLE_PRECISION = "exact"
_FAST_OPTED_IN = False  # set_resample_precision("fast", allow_out_of_tolerance=True) was called in this process


def set_resample_precision(mode: str, *, allow_out_of_tolerance: bool = False) -> None:
    """Process-wide arithmetic of ``tio_resample3d`` for float32 trilinear images.

    ``"exact"`` (default) reproduces the reference's float32 operation sequence bit for bit.
    ``"tight"`` keeps every sampling coordinate the reference's float32 value bit for bit — hence the same eight taps,
    the same weights and the same fill decisions — and fuses only the interpolation (three nested fma lerps): results
    within the rounding of seven multiply-adds of the reference, i.e. inside the north-star bar PER VOXEL
    (``|d| <= 1e-4 max(|ref|, 1e-3 range)``) even on white noise.  The mode of the bench's headline.
    ``"fast"`` is NOT north-star compliant and is refused unless ``allow_out_of_tolerance=True``: coordinates as a line
    per control cell, within 1e-4 of the intensity RANGE but not per voxel on noisy data (one ulp of a coordinate already
    moves a white-noise value by more than the per-voxel bar allows: 4.4 M of 134 M voxels of a bare launch beyond it).
    It is kept for A/B measurements of the coordinate chain's cost; once a process has opted in, the mode can be
    re-selected (restoring a saved mode) without repeating the flag.  Label maps resampled with ``"nearest"`` and
    ``"label"`` (partial-volume) images are bit-identical to the reference in every mode.
    """
    global _RESAMPLE_PRECISION, _FAST_OPTED_IN
    if mode not in PRECISION_CODES:
        raise ValueError(f"precision must be one of {sorted(PRECISION_CODES)}, got {mode!r}")
    if mode == "fast":
        if not (allow_out_of_tolerance or _FAST_OPTED_IN):
            raise ValueError('resample precision "fast" is outside the per-voxel tolerance (1e-4 relative) on noisy data; '
                             'pass allow_out_of_tolerance=True to select it for measurements')
        _FAST_OPTED_IN = True
    _RESAMPLE_PRECISION = mode


def get_resample_precision() -> str:
    return _RESAMPLE_PRECISION


_STENCIL_PRECISION = "exact"


def set_stencil_precision(mode: str) -> None:
    """Process-wide arithmetic of the fused Blur launch (``tio_blur_fused``): ``"exact"`` (default) accumulates every tap with
    a separately rounded multiply and add, like the reference's convolution (bit-identical to the unfused launches);
    ``"fast"`` uses fused multiply-adds — one rounding per tap, results within float rounding (~1e-7 relative; the
    contract for intensities is 1e-4), and a J + K (+ noise) pass, which is bound by vector instructions, ~25 % shorter."""
    global _STENCIL_PRECISION
    if mode not in ("exact", "fast"):
        raise ValueError(f'stencil precision must be "exact" or "fast", got {mode!r}')
    _STENCIL_PRECISION = mode


def get_stencil_precision() -> str:
    return _STENCIL_PRECISION


def reload_env() -> None:
    """Have ``libtio_hip.so`` parse its ``TIO_*`` environment switches again (it reads them once per process, at the first
    call that needs one: ``tio_reload_env``, ABI 10).  Only A/B experiments and tests change them after start-up."""
    _lib.load()[1]["reload_env"]()


def h2d(tensor: Tensor, device) -> Tensor:
    """Upload a (small) host tensor without stalling the device.

    ``tensor.to(device)`` from pageable memory blocks the host until everything already
    queued on the stream has finished, so a pipeline of transforms can never run ahead of
    the GPU (measured: ~1 ms of idle gaps per 4.7 ms bench step).  Staging through the
    caching pinned allocator + ``non_blocking`` keeps the copy stream-ordered and the host
    free; the allocator holds the staging block until the copy has completed.
    """
    device = torch.device(device)
    if device.type != "cuda" or tensor.device.type != "cpu":
        return tensor.to(device)
    return tensor.contiguous().pin_memory().to(device, non_blocking=True)


def h2d_packed(tensors: Sequence[Tensor | None], device) -> list[Tensor | None]:
    """Upload several small float32 host tensors with ONE staging copy; returns device views of the same shapes.

    Each stream-ordered upload is a ~4 us copy kernel plus a ~6 us gap on the GPU's timeline, in front of whatever needs
    it; a transform (or a fused launch of three) that needs three parameter blocks pays that three times.  Entries that are
    ``None`` or already on the device pass through.  Segments start on 256-byte boundaries (vector loads in the kernels).
    """
    device = torch.device(device)
    todo = [i for i, t in enumerate(tensors) if t is not None and t.device.type == "cpu"]
    out: list[Tensor | None] = list(tensors)
    if device.type != "cuda" or not todo:
        return [None if t is None else t.to(device) for t in tensors]
    if len(todo) == 1:
        out[todo[0]] = h2d(tensors[todo[0]].to(torch.float32), device)
        return out
    offsets, total = [], 0
    for i in todo:
        offsets.append(total)
        total += (tensors[i].numel() + 63) // 64 * 64
    staging = torch.empty(total, dtype=torch.float32).pin_memory()
    for i, off in zip(todo, offsets, strict=True):
        staging[off : off + tensors[i].numel()] = tensors[i].reshape(-1).to(torch.float32)
    block = staging.to(device, non_blocking=True)
    for i, off in zip(todo, offsets, strict=True):
        out[i] = block[off : off + tensors[i].numel()].view(tensors[i].shape)
    return out


_MINIMUM_STATE = threading.local()  # (per THREAD — Queue's workers run Composes concurrently; one thread's withdrawal used to disarm another's announcement)


def expect_minimum_fill(flag: bool) -> None:
    """Announce (or withdraw) that the consumer of the next resampling's output will ask for the per-channel minimum of its
    first element (``default_pad_value="minimum"``): large FAST launches then fold it into their stores (``resample3d``)."""
    _MINIMUM_STATE.wanted = bool(flag)


def minimum_fill_expected() -> bool:
    return getattr(_MINIMUM_STATE, "wanted", False)


def folded_channel_min(data: Tensor) -> Tensor | None:
    """The per-channel minimum of element 0 that the launch which produced *data* left behind, if it did and the
    tensor has not been written since (``Engine.resample3d``); ``None`` otherwise."""
    record = getattr(data, "_tio_channel_min", None)
    if record is None or record[0] != data._version:
        return None
    return record[1]


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DTYPE_CODES[dtype]
    except KeyError:
        raise TypeError(f"unsupported image dtype {dtype}") from None


def _ptr(t: Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i32x3(values) -> C.Array:
    return (C.c_int32 * 3)(*[int(v) for v in values])


class _PadConstantFn(torch.autograd.Function):
    """Constant padding (one value, or one per batch element for the statistic modes) with its two gradients: the
    interior of the incoming gradient for the data, the sum over the border for each element's fill value."""

    @staticmethod
    def forward(ctx, data, fill_per_element, engine, padding, fill):
        ctx.padding, ctx.in_shape, ctx.has_fills = padding, data.shape, fill_per_element is not None
        ctx.fill_dtype = None if fill_per_element is None else fill_per_element.dtype
        ctx.fill_shape = None if fill_per_element is None else fill_per_element.shape
        fills = None if fill_per_element is None else fill_per_element.detach()
        return engine.pad3d(data.detach(), padding, "constant", fill, fills)

    @staticmethod
    def backward(ctx, grad):
        p, (_, _, si, sj, sk) = ctx.padding, ctx.in_shape
        inner = grad[:, :, p[0] : p[0] + si, p[2] : p[2] + sj, p[4] : p[4] + sk]
        grad_fill = None
        if ctx.has_fills:
            border = grad.sum(dim=(1, 2, 3, 4)) - inner.sum(dim=(1, 2, 3, 4))
            grad_fill = border.to(ctx.fill_dtype).reshape(ctx.fill_shape)
        return inner.contiguous(), grad_fill, None, None, None


class Engine:
    """One loaded implementation of the C ABI bound to one device type.

    Autograd: the reference's transforms are differentiable with respect to the image data (they are compositions
    of torch ops).  Here every op that has a derivative takes inputs that require grad, runs its kernel on the
    detached data and attaches a backward: the adjoint scatter kernel for trilinear resampling
    (``TIO_LINEAR_ADJOINT``), the same multiply for the bias field, the flip for the flip, closed-form tensor algebra
    for gamma / noise, the transposed clamped stencil for the blur (``tio_separable_conv3d_adjoint``, round 6).
    The geometry of a trilinear resampling is differentiable too: a ``mapping`` or ``control_points`` tensor that requires a
    gradient receives one from ``tio_resample3d_geometry_grad`` (``resample3d``, ``resample3d_geometry_grad``).  So are the
    parameters of the intensity ops: a coarse bias grid, blur taps, a noise mean / deviation or a gamma exponent that requires a
    gradient receives one from the fused reductions of ``intensity_param_grad.hip`` (``bias_field_grad``, ``separable_conv3d_taps_grad``,
    ``noise_grad``, ``gamma_grad``); plain numbers get none.
    The pre-processing ops are linear in the data and attach their transposes: the gather adjoints of ``interpolate_adjoint.hip`` for
    ``interpolate3d``, ``axis_gather_lerp`` and the reflect / replicate / circular ``pad3d``; ``ghost_lines`` and ``kspace_segment_mix`` are
    symmetric operators and run their own kernel on the gradient.
    """

    def __init__(self, functions: dict, device_type: str, name: str):
        self._fn = functions
        self.device_type = device_type
        self.name = name

    # -- plumbing -----------------------------------------------------------
    def _check(self, what: str, *tensors: Tensor | None) -> None:
        for t in tensors:
            if t is None:
                continue
            if t.device.type != self.device_type:
                raise EngineError(
                    f"{what}: tensor on {t.device} but the {self.name} engine runs on {self.device_type} tensors — move the data"
                    f" to the GPU (`subject.to('cuda')`), or keep using `torchio` itself with"
                    " `torchio_amd.reference_binding.bind()`: there, host tensors stay on the reference's own code"
                )
            if t.requires_grad and torch.is_grad_enabled():  # (with grad disabled a tensor that requires grad is just data)
                raise EngineError(
                    f"{what}: this {self.name} engine op has no backward (differentiable: trilinear resampling, bias field, blur,"
                    " noise, gamma, flip, permute, pad, interpolate3d, axis_gather_lerp, ghost_lines, kspace_segment_mix) — detach"
                    " the tensor, or use `torchio` with `torchio_amd.reference_binding.bind()`,"
                    " which leaves autograd inputs to the reference's own path"
                )

    def _stream(self, ref: Tensor):
        if self.device_type == "cuda":
            # torch._C._cuda_getCurrentRawStream: the raw handle without building a torch.cuda.Stream object per call
            return C.c_void_p(torch._C._cuda_getCurrentRawStream(ref.device.index if ref.device.index is not None else torch.cuda.current_device()))
        return None

    def _call(self, name: str, ref: Tensor, *args) -> None:
        if self.device_type == "cuda" and ref.device.index != torch.cuda.current_device():
            with torch.cuda.device(ref.device):
                status = self._fn[name](*args)
        else:
            status = self._fn[name](*args)
        if status != _abi.OK:
            message = ""
            if "last_error" in self._fn:
                message = (self._fn["last_error"]() or b"").decode(errors="replace")
            raise EngineError(f"tio_{name} failed with status {status}: {message}")

    @staticmethod
    def _flags(flags: Tensor | None, batch: int, what: str) -> Tensor | None:
        if flags is None:
            return None
        if flags.dtype not in (torch.uint8, torch.bool) or flags.numel() != batch:
            raise ValueError(f"{what} must hold {batch} uint8/bool flags")
        return flags.to(torch.uint8).contiguous()

    def _parameter_kernel(self, name: str, what: str) -> None:
        """A parameter that requires a gradient needs ``tio_<name>``: only the HIP library has it (no quiet ``None``)."""
        if name not in self._fn:
            raise NotImplementedError(
                f"{what} requires a gradient, but the {self.name} engine has no tio_{name}: the parameter gradients of the intensity"
                " ops exist on the HIP engine only - detach the parameter, or run on the GPU")

    def _data_adjoint_kernel(self, name: str, what: str) -> None:
        """The gather adjoints of ``interpolate_adjoint.hip`` (``tio_<name>``): only the HIP library has them."""
        if name not in self._fn:
            raise NotImplementedError(
                f"{what}: the {self.name} engine has no tio_{name}: the data gradients of interpolate3d, axis_gather_lerp and the"
                " reflect / replicate / circular pad3d exist on the HIP engine only - detach the tensor, or run on the GPU")

    def _workspace(self, name: str, ref: Tensor, *args) -> tuple[Tensor, int]:
        nbytes = int(self._fn[name](*args))
        return torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=ref.device), nbytes

    # -- spatial ------------------------------------------------------------
    def _resample_geom(
        self, batch: int, in_shape, out_shape, mapping: Tensor, control_points: Tensor | None, in_spacing, out_spacing,
        affine_first: bool, cp_skip: Tensor | None, passthrough: Tensor | None, norm_shape, precision: str | None,
        large_boxes: bool = False,
    ):
        """``tio_resample_geom`` of one launch and the tensors it points into (mapping, control points, flags — keep them alive)."""
        if mapping.dtype != torch.float32 or not mapping.is_contiguous():
            mapping = mapping.to(torch.float32).contiguous()
        if mapping.ndim != 3 or mapping.shape[1:] != (3, 4) or mapping.shape[0] not in (1, batch):
            raise ValueError(f"mapping must be (1|B, 3, 4), got {tuple(mapping.shape)}")
        geom = _abi.ResampleGeom()
        geom.batch = batch
        geom.in_shape = _i32x3(in_shape)
        geom.out_shape = _i32x3(out_shape)
        geom.affine_first = int(bool(affine_first))
        geom.mapping_dev = mapping.data_ptr()
        geom.mapping_batched = int(mapping.shape[0] == batch and batch > 1)
        if control_points is not None:
            if control_points.dtype != torch.float32 or not control_points.is_contiguous():
                control_points = control_points.to(torch.float32).contiguous()
            if control_points.ndim != 5 or control_points.shape[-1] != 3 or control_points.shape[0] not in (1, batch):
                raise ValueError(f"control_points must be (1|B, ni, nj, nk, 3), got {tuple(control_points.shape)}")
            geom.control_points_dev = control_points.data_ptr()
            geom.cp_batched = int(control_points.shape[0] == batch and batch > 1)
            geom.cp_shape = _i32x3(control_points.shape[1:4])
        cp_skip = self._flags(cp_skip, batch, "cp_skip")
        passthrough = self._flags(passthrough, batch, "passthrough")
        geom.cp_skip_dev = None if cp_skip is None else cp_skip.data_ptr()
        geom.passthrough_dev = None if passthrough is None else passthrough.data_ptr()
        geom.in_spacing = (C.c_float * 3)(*[float(s) for s in in_spacing])
        geom.out_spacing = (C.c_float * 3)(*[float(s) for s in out_spacing])
        if norm_shape is not None:  # the shape the coordinates are normalised with, when it is not the images' own
            geom.norm_shape = _i32x3(norm_shape)
        geom.precision = PRECISION_CODES[precision if precision is not None else _RESAMPLE_PRECISION]
        geom.flags = (0, _abi.GEOM_LARGE_BOXES, _abi.GEOM_MOSTLY_LARGE_BOXES)[min(int(large_boxes), 2)]  # (0 / False: no hint, 1 / True: some bricks, 2: most)
        self._check("resample3d", mapping, control_points, cp_skip, passthrough)
        return geom, [mapping, control_points, cp_skip, passthrough]

    @staticmethod
    def _plan_signature(geom) -> tuple:
        """What a brick plan is made for (include/tio_hip.h: plan_dev): the road and the plan's layout follow from these fields
        — the C side checks only a plan's size, and a plan made under another hint or precision can have the size of the call's."""
        return (geom.precision, geom.flags, geom.batch, tuple(geom.in_shape), tuple(geom.out_shape), geom.control_points_dev is not None,
                geom.affine_first)

    def resample_plan(
        self, *, batch: int, in_shape, out_shape, mapping: Tensor, control_points: Tensor | None, in_spacing, out_spacing,
        affine_first: bool, cp_skip: Tensor | None = None, passthrough: Tensor | None = None, norm_shape=None,
        precision: str | None = None, large_boxes: bool = False,
    ) -> Tensor | None:
        """The brick plan of the launch ``resample3d`` would make for this geometry with float32 trilinear images, enqueued on
        the CURRENT stream of the mapping's device (``tio_resample3d_plan``, ABI 11) — or ``None`` when that launch takes a
        road without a plan (small batches, ...).  Hand the tensor to ``resample3d(..., plan=...)`` with the same geometry, on
        a stream ordered behind this one; the planning kernel then leaves that call's critical path.  The plan serves any number
        of such calls; it carries what it was made for (precision, hint, batch, shapes, control points or not, composition
        order), and a call made for something else ignores it."""
        if "resample3d_plan" not in self._fn or mapping.device.type != self.device_type:
            return None
        geom, keep_alive = self._resample_geom(
            batch, tuple(in_shape), tuple(int(s) for s in out_shape), mapping, control_points, in_spacing, out_spacing,
            affine_first, cp_skip, passthrough, norm_shape, precision, large_boxes,
        )
        reference = keep_alive[0]
        if self.device_type == "cuda" and reference.device.index != torch.cuda.current_device():
            with torch.cuda.device(reference.device):
                size = self._fn["resample3d_plan_bytes"](C.byref(geom))
        else:
            size = self._fn["resample3d_plan_bytes"](C.byref(geom))
        if size <= 0:
            return None
        plan = torch.empty((size + 3) // 4, dtype=torch.int32, device=reference.device)
        self._call("resample3d_plan", reference, C.byref(geom), C.c_void_p(plan.data_ptr()), size, self._stream(reference))
        plan._tio_plan_signature = self._plan_signature(geom)  # (`resample3d` hands the plan only to calls of this signature)
        del keep_alive
        return plan

    def resample3d(
        self,
        images: Sequence[Tensor],
        *,
        out_shape: Sequence[int],
        mapping: Tensor,
        control_points: Tensor | None,
        in_spacing: Sequence[float],
        out_spacing: Sequence[float],
        affine_first: bool,
        interps: Sequence[str | int],
        fills: Sequence[Tensor | None],
        cp_skip: Tensor | None = None,
        passthrough: Tensor | None = None,
        label_tables: Sequence[Tensor | None] | None = None,
        pad_labels: Sequence[float] | None = None,
        norm_shape: Sequence[int] | None = None,
        precision: str | None = None,
        plan: Tensor | None = None,
        large_boxes: bool = False,
        _adjoint_of: Sequence[Tensor] | None = None,
    ) -> list[Tensor]:
        """Resample every ``(B, C, I, J, K)`` tensor in *images* through one coordinate pass.

        ``mapping`` is ``(1|B, 3, 4)`` float32 (output voxel → input voxel),
        ``control_points`` ``(1|B, ni, nj, nk, 3)`` float32 in mm or ``None``;
        ``fills[n]`` is ``None`` (zero padding, no mask) or a ``(C,)`` float32
        tensor.  Returns new contiguous tensors ``(B, C, *out_shape)`` with the
        input dtypes.  Images with interpolation ``"label"`` (single channel) take the
        fused partial-volume mode: ``label_tables[n]`` is ``torch.unique(images[n])`` as
        float64 on the data's device (or ``None``: exact for fewer than 16 labels) and
        ``pad_labels[n]`` the out-of-bounds label; ``fills[n]`` is ignored for them.
        ``large_boxes``: the caller's hint that some (1 / True: ``TIO_GEOM_LARGE_BOXES``) or most (2: ``TIO_GEOM_MOSTLY_LARGE_BOXES``)
        bricks' input boxes exceed the staging tile (transforms/spatial.py: ``_expects_large_boxes``) — a choice of road, never of values.
        """
        if not images:
            return []
        if not (len(images) == len(interps) == len(fills)):
            raise ValueError("images, interps and fills must have the same length")
        first = images[0]
        if first.ndim != 5:
            raise ValueError(f"expected (B, C, I, J, K) tensors, got {tuple(first.shape)}")
        batch = first.shape[0]
        in_shape = tuple(first.shape[2:])
        out_shape = tuple(int(s) for s in out_shape)
        # geometry that takes part in autograd (a mapping or control points that require a gradient): the kernels see the detached
        # float32 values on the images' device, the float trilinear outputs get `tio_resample3d_geometry_grad` as their backward
        geometry_leaves = (mapping, control_points)
        wants_geometry = _adjoint_of is None and (_wants_grad(mapping) or _wants_grad(control_points))
        if wants_geometry:
            mapping = h2d(mapping.detach().to(torch.float32), first.device)
            control_points = None if control_points is None else h2d(control_points.detach().to(torch.float32), first.device)
        geom, keep_alive = self._resample_geom(
            batch, in_shape, out_shape, mapping, control_points, in_spacing, out_spacing, affine_first, cp_skip, passthrough,
            norm_shape, precision, large_boxes,
        )
        mapping, control_points, cp_skip, passthrough = keep_alive[:4]
        # made ahead by `resample_plan` for this geometry: a plan made under another hint or precision — or not by
        # `resample_plan` — stays with its maker (the call plans for itself)
        if plan is not None and plan.device == first.device and getattr(plan, "_tio_plan_signature", None) == self._plan_signature(geom):
            geom.plan_dev = plan.data_ptr()
            geom.plan_bytes = plan.numel() * plan.element_size()
            keep_alive.append(plan)

        # images that take part in autograd (float, trilinear): the kernel sees the detached data, the result gets
        # the adjoint launch as its backward
        sources = list(images)
        codes = [INTERP_CODES[i] if isinstance(i, str) else int(i) for i in interps]
        if _adjoint_of is None and any(t.requires_grad for t in images):
            wants = [_wants_grad(t) and t.dtype in FLOAT_DTYPES and codes[n] == _abi.LINEAR for n, t in enumerate(images)]
            images = [t.detach() if t.requires_grad else t for t in images]
            for n, t in enumerate(sources):
                if _wants_grad(t) and not wants[n]:
                    raise EngineError("resample3d: only floating-point images resampled trilinearly are differentiable")
        else:  # (the usual call: nothing takes part in autograd)
            wants = [False] * len(images)

        # The folded minimum: a large planned launch (FAST, TIGHT, and EXACT on the lean exact-coordinate kernel) can hand back the per-channel minimum of element 0 of each output
        # (tio_resample_image.out_min_dev), which is what the NEXT spatial transform's default_pad_value="minimum" will ask
        # of exactly this tensor (`folded_channel_min`).  Requested when somebody has announced that consumer
        # (`expect_minimum_fill`: a Compose that draws ahead knows its next child) or with TIO_FOLDED_MIN=1; only the bricks of
        # element 0 track what they store, in an instantiation of its own, and a ~2 us kernel (resample_plan.hpp: min_finish_kernel) decodes the
        # result: it replaces the ~21 us reduction and its re-read of the volume.  Requested only where the C side folds it
        # (the rule of resample.hip's planned path, mirrored loosely: a miss costs one tio_channel_min launch, never a wrong
        # value).
        fold_min = (
            _adjoint_of is None and (minimum_fill_expected() or os.environ.get("TIO_FOLDED_MIN", "") not in ("", "0"))
            and batch * -(-out_shape[0] // 16) * -(-out_shape[1] // 16) * -(-out_shape[2] // 16) >= 12288 and not any(wants)
            and len(images) <= _abi.MAX_IMAGES and all(t.dtype == torch.float32 for t in images) and all(c == _abi.LINEAR for c in codes)
        )
        folded: list[Tensor | None] = []

        outputs: list[Tensor] = []
        for start in range(0, len(images), _abi.MAX_IMAGES):
            chunk = range(start, min(start + _abi.MAX_IMAGES, len(images)))
            descs = (_abi.ResampleImage * len(chunk))()
            for slot, n in enumerate(chunk):
                data = images[n]
                if data.ndim != 5 or data.shape[0] != batch or tuple(data.shape[2:]) != in_shape:
                    raise ValueError("all images must share the batch size and spatial shape")
                if not data.is_contiguous():
                    data = data.contiguous()
                fill = fills[n]
                if fill is not None:
                    if fill.dtype != torch.float32 or fill.device != data.device or not fill.is_contiguous():
                        fill = h2d(fill.to(torch.float32), data.device).contiguous()
                    if fill.numel() != data.shape[1]:
                        raise ValueError("fill must have one value per channel")
                self._check("resample3d", data, fill)
                if _adjoint_of is not None:  # `data` is the zeroed accumulator, `out` the incoming gradient (read)
                    out = _adjoint_of[n].to(torch.float32).contiguous()
                    if tuple(out.shape) != (batch, data.shape[1], *out_shape):
                        raise ValueError("gradient shape does not match the forward output")
                else:
                    out = torch.empty((batch, data.shape[1], *out_shape), dtype=data.dtype, device=data.device)
                descs[slot].in_ = data.data_ptr()
                descs[slot].out = out.data_ptr()
                descs[slot].channels = data.shape[1]
                descs[slot].dtype = dtype_code(data.dtype)
                descs[slot].interp = codes[n]
                descs[slot].fill_dev = None if fill is None else fill.data_ptr()
                if descs[slot].interp == _abi.LABEL_PV:
                    table = None if label_tables is None else label_tables[n]
                    if table is not None:
                        table = table.to(device=data.device, dtype=torch.float64).contiguous()
                        self._check("resample3d", table)
                        descs[slot].labels_dev = table.data_ptr()
                        descs[slot].n_labels = table.numel()
                    descs[slot].pad_label = 0.0 if pad_labels is None else float(pad_labels[n])
                    keep_alive.append(table)
                minimum = torch.empty(data.shape[1], dtype=torch.float32, device=data.device) if fold_min else None
                descs[slot].out_min_dev = None if minimum is None else minimum.data_ptr()
                folded.append(minimum)
                keep_alive += [data, fill]
                outputs.append(out)
            self._call("resample3d", first, C.byref(geom), len(chunk), descs, self._stream(first))
        note_resample_launch(first)
        del keep_alive
        for out, minimum in zip(outputs, folded, strict=True):
            if minimum is not None:
                out._tio_channel_min = (out._version, minimum)
        if _adjoint_of is not None:
            return [t for t in images]  # the accumulators now hold dL/d(input)
        if any(wants):
            shared = dict(
                out_shape=out_shape, mapping=mapping, control_points=control_points, in_spacing=tuple(in_spacing),
                out_spacing=tuple(out_spacing), affine_first=affine_first, cp_skip=cp_skip, passthrough=passthrough,
                norm_shape=norm_shape, precision="exact",
            )
            for n, want in enumerate(wants):
                if not want:
                    continue
                source, fill = sources[n], fills[n]

                def backward(grad, source=source, fill=fill):
                    accumulator = torch.zeros(source.shape, dtype=torch.float32, device=source.device)
                    self.resample3d([accumulator], interps=["linear_adjoint"], fills=[fill], _adjoint_of=[grad], **shared)
                    return accumulator.to(source.dtype)

                outputs[n] = _AttachBackward.apply(source, outputs[n], backward)
        if wants_geometry:
            # every float trilinear output of the call joins ONE graph node, so that a backward pass launches once per MAX_IMAGES
            # chunk whatever the number of outputs; the other images (label maps riding along) took part in the forward and carry
            # no gradient
            members = [n for n, t in enumerate(images) if t.dtype in FLOAT_DTYPES and codes[n] == _abi.LINEAR]
            if members:
                shared = dict(
                    out_shape=out_shape, mapping=mapping, control_points=control_points, in_spacing=tuple(in_spacing),
                    out_spacing=tuple(out_spacing), affine_first=affine_first, cp_skip=cp_skip, passthrough=passthrough, norm_shape=norm_shape,
                )
                data, member_fills = [images[n] for n in members], [fills[n] for n in members]

                def geometry_backward(grads, want_mapping, want_control_points):
                    present = [n for n, grad in enumerate(grads) if grad is not None]
                    if not present:
                        return None, None
                    return self.resample3d_geometry_grad(
                        [data[n] for n in present], [grads[n] for n in present], fills=[member_fills[n] for n in present],
                        want_mapping=want_mapping, want_control_points=want_control_points, **shared)

                attached = _AttachGeometryBackward.apply(geometry_backward, *geometry_leaves, *[outputs[n] for n in members])
                for n, out in zip(members, attached, strict=True):
                    outputs[n] = out
        return outputs

    def resample3d_geometry_grad(
        self,
        images: Sequence[Tensor],
        grads: Sequence[Tensor],
        *,
        out_shape: Sequence[int],
        mapping: Tensor,
        control_points: Tensor | None,
        in_spacing: Sequence[float],
        out_spacing: Sequence[float],
        affine_first: bool,
        fills: Sequence[Tensor | None],
        cp_skip: Tensor | None = None,
        passthrough: Tensor | None = None,
        norm_shape: Sequence[int] | None = None,
        want_mapping: bool = True,
        want_control_points: bool = True,
    ) -> tuple[Tensor | None, Tensor | None]:
        """``d <resample3d(images), grads> / d(mapping, control_points)`` in one fused launch per ``MAX_IMAGES`` images
        (``tio_resample3d_geometry_grad``: include/tio_hip.h has the definition).  *images* are the float tensors ``(B, C, I, J, K)``
        that ``resample3d`` resampled trilinearly with this geometry and *fills*, *grads* the gradients ``(B, C, *out_shape)`` of
        their outputs.  Returns float32 tensors in the shapes of *mapping* ``(1|B, 3, 4)`` and *control_points*, ``None`` for the
        one that is not wanted (or, for the control points, not there).  Nothing here takes part in autograd."""
        if not images or not (len(images) == len(grads) == len(fills)):
            raise ValueError("images, grads and fills must be non-empty and of the same length")
        want_control_points = want_control_points and control_points is not None
        if not (want_mapping or want_control_points):
            return None, None
        first = images[0]
        if first.ndim != 5:
            raise ValueError(f"expected (B, C, I, J, K) tensors, got {tuple(first.shape)}")
        batch, in_shape, out_shape = first.shape[0], tuple(first.shape[2:]), tuple(int(s) for s in out_shape)
        with torch.no_grad():
            geom, keep_alive = self._resample_geom(
                batch, in_shape, out_shape, mapping.detach(), None if control_points is None else control_points.detach(), in_spacing,
                out_spacing, affine_first, cp_skip, passthrough, norm_shape, "exact",
            )
            mapping, control_points = keep_alive[:2]
            d_mapping = torch.empty_like(mapping) if want_mapping else None
            d_control = torch.empty_like(control_points) if want_control_points else None
            nbytes = int(self._fn["resample3d_geometry_grad_workspace_bytes"](C.byref(geom)))
            workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=first.device)
            total_mapping = total_control = None
            for start in range(0, len(images), _abi.MAX_IMAGES):
                chunk = range(start, min(start + _abi.MAX_IMAGES, len(images)))
                descs = (_abi.ResampleImage * len(chunk))()
                for slot, n in enumerate(chunk):
                    data, grad, fill = images[n].detach(), grads[n].detach(), fills[n]
                    if data.ndim != 5 or data.shape[0] != batch or tuple(data.shape[2:]) != in_shape:
                        raise ValueError("all images must share the batch size and spatial shape")
                    if data.dtype not in FLOAT_DTYPES:
                        raise EngineError("resample3d_geometry_grad: only floating-point images resampled trilinearly carry a geometry gradient")
                    if tuple(grad.shape) != (batch, data.shape[1], *out_shape):
                        raise ValueError("gradient shape does not match the forward output")
                    data, grad = data.contiguous(), grad.to(torch.float32).contiguous()
                    if fill is not None:
                        if fill.dtype != torch.float32 or fill.device != data.device or not fill.is_contiguous():
                            fill = h2d(fill.to(torch.float32), data.device).contiguous()
                        if fill.numel() != data.shape[1]:
                            raise ValueError("fill must have one value per channel")
                    self._check("resample3d_geometry_grad", data, grad, fill)
                    descs[slot].in_ = data.data_ptr()
                    descs[slot].out = grad.data_ptr()
                    descs[slot].channels = data.shape[1]
                    descs[slot].dtype = dtype_code(data.dtype)
                    descs[slot].interp = _abi.LINEAR
                    descs[slot].fill_dev = None if fill is None else fill.data_ptr()
                    keep_alive += [data, grad, fill]
                if start > 0:  # a further chunk: fresh outputs, summed below (the launch overwrites its outputs)
                    total_mapping, total_control = d_mapping, d_control
                    d_mapping = torch.empty_like(mapping) if want_mapping else None
                    d_control = torch.empty_like(control_points) if want_control_points else None
                self._call("resample3d_geometry_grad", first, C.byref(geom), len(chunk), descs, _ptr(d_mapping), _ptr(d_control), _ptr(workspace),
                           nbytes, self._stream(first))
                if start > 0:
                    d_mapping = None if d_mapping is None else total_mapping + d_mapping
                    d_control = None if d_control is None else total_control + d_control
            del keep_alive
        return d_mapping, d_control

    def bspline_prefilter(self, data: Tensor, order: int) -> Tensor:
        """B-spline coefficients (float32) of a ``(B, C, I, J, K)`` tensor for ``resample3d``'s ``"quadratic"`` (order 2) /
        ``"cubic"`` (order 3) images: the recursive prefilter with the half-sample-symmetric boundary that
        ``interpol.grid_pull(prefilter=True, bound="dct2")`` applies before sampling (spatial.py:1753-1760)."""
        if data.ndim != 5:
            raise ValueError("expected a (B, C, I, J, K) tensor")
        if order not in (2, 3, 4, 5, 6, 7):
            raise NotImplementedError(f"B-spline order {order} is not implemented (2 ... 7 are)")
        if _wants_grad(data):
            raise EngineError("bspline_prefilter: B-spline resampling is not differentiable here (use reference_binding)")
        data = data.detach().contiguous()
        self._check("bspline_prefilter", data)
        out = torch.empty(data.shape, dtype=torch.float32, device=data.device)
        self._call(
            "bspline_prefilter", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0] * data.shape[1],
            _i32x3(data.shape[2:]), int(order), self._stream(data),
        )
        return out

    def channel_min(self, data: Tensor) -> Tensor:
        """Per-channel minimum of the first batch element as a ``(C,)`` float32 device tensor."""
        data = data.detach()  # a fill VALUE (the reference takes `.item()`): no gradient flows through it
        self._check("channel_min", data)
        first = data if data.is_contiguous() else data[0].contiguous()  # element 0 of a dense batch starts at the batch's pointer
        channels = data.shape[1]
        n_spatial = 1
        for extent in data.shape[2:]:
            n_spatial *= int(extent)
        out = torch.empty(channels, dtype=torch.float32, device=data.device)
        self._call("channel_min", data, _ptr(first), dtype_code(data.dtype), channels, n_spatial, _ptr(out), self._stream(data))
        return out

    # -- intensity ----------------------------------------------------------
    def separable_conv3d(
        self, data: Tensor, taps: Tensor, radius: Sequence[int], skip: Tensor | None = None
    ) -> Tensor:
        """Per-axis cross-correlation with replicate padding; ``taps`` is ``(1|B, 3, stride)``."""
        if data.ndim != 5:
            raise ValueError("expected a (B, C, I, J, K) tensor")
        if data.dtype not in FLOAT_DTYPES:
            raise TypeError(f"separable_conv3d needs a floating dtype, got {data.dtype}")
        if _wants_grad(taps):  # the kernel sees the detached float32 taps on the data's device; the result gets the tap correlation as its backward
            self._parameter_kernel("separable_conv3d_taps_grad", "separable_conv3d: taps")
            values, source = h2d(taps.detach().to(torch.float32), data.device), data.detach()
            result = self.separable_conv3d(data, values, radius, skip=skip)
            return _AttachParameterBackward.apply(
                "separable_conv3d", lambda grad, wants: [self.separable_conv3d_taps_grad(source, grad, values, radius, skip=skip)], result, taps)
        if _wants_grad(data):
            detached = data.detach()
            result = self.separable_conv3d(detached, taps, radius, skip=skip)
            return _AttachBackward.apply(data, result, lambda grad: self.separable_conv3d_adjoint(grad, taps, radius, skip=skip).to(data.dtype))
        batch, channels = data.shape[:2]
        data = data.contiguous()
        taps = taps.to(torch.float32).contiguous()
        if taps.ndim != 3 or taps.shape[1] != 3 or taps.shape[0] not in (1, batch):
            raise ValueError(f"taps must be (1|B, 3, stride), got {tuple(taps.shape)}")
        skip = self._flags(skip, batch, "skip")
        self._check("separable_conv3d", data, taps, skip)
        out = torch.empty_like(data)
        active = sum(1 for r in radius if int(r) > 0)
        tmp = None
        if active > 1:
            tmp = torch.empty((2, *data.shape), dtype=torch.float32, device=data.device)
        self._call(
            "separable_conv3d", data, _ptr(data), _ptr(out), _ptr(tmp), dtype_code(data.dtype), batch, channels,
            _i32x3(data.shape[2:]), _ptr(taps), int(taps.shape[0] == batch and batch > 1), taps.shape[2],
            _i32x3(radius), _ptr(skip), self._stream(data),
        )
        return out

    def separable_conv3d_adjoint(self, grad: Tensor, taps: Tensor, radius: Sequence[int], skip: Tensor | None = None) -> Tensor:
        """Backward of ``separable_conv3d`` with respect to its data (``tio_separable_conv3d_adjoint``, ABI 16): the transposes
        of the three replicate-padded correlations in reverse order, float32 — what autograd derives through the reference's
        ``F.pad(mode="replicate")`` + grouped ``conv3d`` per axis (blur.py:157-252).  The transpose of a CLAMPED stencil folds the
        taps that were clamped onto a border voxel back onto it; rows flagged in *skip* pass their gradient through."""
        if grad.ndim != 5:
            raise ValueError("expected a (B, C, I, J, K) gradient")
        batch, channels = grad.shape[:2]
        grad = grad.detach().to(torch.float32).contiguous()
        taps = taps.to(device=grad.device, dtype=torch.float32).contiguous()
        if taps.ndim != 3 or taps.shape[1] != 3 or taps.shape[0] not in (1, batch):
            raise ValueError(f"taps must be (1|B, 3, stride), got {tuple(taps.shape)}")
        skip = self._flags(skip, batch, "skip")
        if skip is not None and skip.device != grad.device:
            skip = skip.to(grad.device)
        self._check("separable_conv3d_adjoint", grad, taps, skip)
        out = torch.empty_like(grad)
        tmp = torch.empty_like(grad) if sum(1 for r in radius if int(r) > 0) > 1 else None
        self._call(
            "separable_conv3d_adjoint", grad, _ptr(grad), _ptr(out), _ptr(tmp), batch, channels, _i32x3(grad.shape[2:]), _ptr(taps),
            int(taps.shape[0] == batch and batch > 1), taps.shape[2], _i32x3(radius), _ptr(skip), self._stream(grad),
        )
        return out

    def blur_fused(
        self,
        data: Tensor,
        taps: Tensor,
        radius: Sequence[int],
        *,
        bias_coarse: Tensor | None = None,
        noise: tuple | None = None,
    ) -> Tensor | None:
        """``Noise(Blur(BiasField(data)))`` in the passes of the separable stencil (``tio_blur_fused``).

        ``bias_coarse``: ``(B, C, si, sj, sk)`` float32 or ``None``; ``noise``: ``(mean, std,
        philox_seed)`` with scalar or ``(B,)`` tensors, or ``(mean, std, draws)`` with *draws* a float32
        device tensor of the data's shape holding one normal draw per element (the reference's seeded
        stream, ``HostNormalStream.randn_ahead``), or ``None``.  Returns ``None`` when this
        engine / these arguments have no fused form (nothing was launched): the caller then runs
        the three ops one after the other, which gives the same values.
        """
        if "blur_fused" not in self._fn or data.dtype != torch.float32 or data.ndim != 5:
            return None
        batch, channels = data.shape[:2]
        data = data.contiguous()
        taps = taps.to(torch.float32).contiguous()
        self._check("blur_fused", data, taps, bias_coarse)
        coarse_shape = None
        if bias_coarse is not None:
            bias_coarse = bias_coarse.to(torch.float32).contiguous()
            if bias_coarse.ndim != 5 or bias_coarse.shape[:2] != data.shape[:2]:
                raise ValueError("bias_coarse must be (B, C, si, sj, sk)")
            coarse_shape = _i32x3(bias_coarse.shape[2:])
        noise_on, mean_f, std_f, mean_t, std_t, batched, seed, base = 0, 0.0, 0.0, None, None, 0, 0, None
        if noise is not None:
            mean, std, seed = noise
            noise_on = 1
            if isinstance(seed, Tensor):  # explicit draws
                base, seed, noise_on = seed, 0, 2
                if base.dtype != torch.float32 or base.device != data.device or base.numel() != data.numel() or not base.is_contiguous():
                    raise ValueError("blur_fused: the draws must be a dense float32 tensor of the data's size on its device")
            batched = int(isinstance(mean, Tensor) or isinstance(std, Tensor))
            if batched:
                mean_t = torch.as_tensor(mean, dtype=torch.float32, device=data.device).expand(batch).contiguous()
                std_t = torch.as_tensor(std, dtype=torch.float32, device=data.device).expand(batch).contiguous()
            else:
                mean_f, std_f = float(mean), float(std)
        out = torch.empty_like(data)
        tmp = torch.empty((2, *data.shape), dtype=torch.float32, device=data.device)
        arguments = (
            _ptr(data), _ptr(out), _ptr(tmp), dtype_code(data.dtype), batch, channels, _i32x3(data.shape[2:]), _ptr(taps),
            int(taps.shape[0] == batch and batch > 1), taps.shape[2], _i32x3(radius), _ptr(bias_coarse), coarse_shape,
            noise_on, mean_f, std_f, _ptr(mean_t), _ptr(std_t), batched, int(seed) & (2**64 - 1), _ptr(base),
            int(_STENCIL_PRECISION == "fast"), self._stream(data),
        )
        if self.device_type == "cuda" and data.device.index != torch.cuda.current_device():
            with torch.cuda.device(data.device):
                status = self._fn["blur_fused"](*arguments)
        else:
            status = self._fn["blur_fused"](*arguments)
        if status == _abi.UNSUPPORTED_CONFIG:
            return None
        if status != _abi.OK:
            message = (self._fn["last_error"]() or b"").decode(errors="replace")
            raise EngineError(f"tio_blur_fused failed with status {status}: {message}")
        return out

    def bias_field_apply(
        self, data: Tensor, coarse: Tensor, *, divide: bool = False, skip: Tensor | None = None
    ) -> Tensor:
        """``data * exp(trilinear_upsample(coarse))`` (or ``/``); ``coarse`` is ``(B, C, si, sj, sk)``."""
        if data.ndim != 5 or coarse.ndim != 5 or coarse.shape[:2] != data.shape[:2]:
            raise ValueError("data and coarse must be 5-D with the same (B, C)")
        if data.dtype not in FLOAT_DTYPES:
            raise TypeError(f"bias_field_apply needs a floating dtype, got {data.dtype}")
        if _wants_grad(coarse):
            self._parameter_kernel("bias_field_grad", "bias_field_apply: coarse")
            values, source = h2d(coarse.detach().to(torch.float32), data.device), data.detach()
            result = self.bias_field_apply(data, values, divide=divide, skip=skip)
            return _AttachParameterBackward.apply(
                "bias_field_apply", lambda grad, wants: [self.bias_field_grad(source, grad, values, divide=divide, skip=skip)], result, coarse)
        if _wants_grad(data):  # y = x * f (or x / f): the gradient is the same multiply applied to the incoming gradient
            result = self.bias_field_apply(data.detach(), coarse, divide=divide, skip=skip)
            return _AttachBackward.apply(data, result, lambda grad: self.bias_field_apply(grad.to(data.dtype), coarse, divide=divide, skip=skip))
        data = data.contiguous()
        coarse = coarse.to(torch.float32).contiguous()
        skip = self._flags(skip, data.shape[0], "skip")
        self._check("bias_field_apply", data, coarse, skip)
        out = torch.empty_like(data)
        self._call(
            "bias_field_apply", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], data.shape[1],
            _i32x3(data.shape[2:]), _ptr(coarse), _i32x3(coarse.shape[2:]), int(bool(divide)), _ptr(skip),
            self._stream(data),
        )
        return out

    def add_noise(
        self,
        data: Tensor,
        mean: float | Tensor,
        std: float | Tensor,
        *,
        rician: bool = False,
        base1: Tensor | None = None,
        base2: Tensor | None = None,
        philox_seed: int = 0,
        keep: Tensor | None = None,
    ) -> Tensor:
        """``data + (mean + std * z)``; ``z`` from *base1*/*base2* or in-kernel Philox when ``None``."""
        if data.dtype not in FLOAT_DTYPES:
            raise TypeError(f"add_noise needs a floating dtype, got {data.dtype}")
        leaves = [p if isinstance(p, Tensor) and _wants_grad(p) else None for p in (mean, std)]
        if any(leaf is not None for leaf in leaves):
            self._parameter_kernel("noise_grad", "add_noise: mean / std")
            mean_v, std_v = (h2d(p.detach().to(torch.float32), data.device) if isinstance(p, Tensor) else p for p in (mean, std))
            source = data.detach()
            result = self.add_noise(data, mean_v, std_v, rician=rician, base1=base1, base2=base2, philox_seed=philox_seed, keep=keep)

            def parameter_backward(grad, wants):
                return list(self.noise_grad(source, grad, mean_v, std_v, rician=rician, base1=base1, base2=base2, philox_seed=philox_seed,
                                            keep=keep, want_mean=wants[0], want_std=wants[1]))

            return _AttachParameterBackward.apply("add_noise", parameter_backward, result, *leaves)
        if _wants_grad(data):
            detached = data.detach()
            result = self.add_noise(detached, mean, std, rician=rician, base1=base1, base2=base2, philox_seed=philox_seed, keep=keep)
            if not rician:  # additive: dy/dx = 1 (gated-out rows are copies: 1 as well)
                return _AttachBackward.apply(data, result, lambda grad: grad)

            def rician_backward(grad):
                # y = sqrt((x + n1)^2 + n2^2): dy/dx = (x + n1) / y, with n1 the FIRST draw of the forward pass
                draws = base1 if base1 is not None else self.philox_normal(detached.shape, philox_seed, 0, detached.device)
                shape = (-1,) + (1,) * (detached.ndim - 1)
                mean_b = mean.to(detached.device).reshape(shape) if isinstance(mean, Tensor) else mean
                std_b = std.to(detached.device).reshape(shape) if isinstance(std, Tensor) else std
                numerator = detached.float() + (mean_b + std_b * draws)
                slope = torch.where(result != 0, numerator / result.float(), torch.zeros_like(numerator))
                if keep is not None:  # gated-out rows are exact copies of the input
                    rows = keep.to(detached.device).bool().reshape(shape)
                    slope = torch.where(rows, slope, torch.ones_like(slope))
                return (grad.float() * slope).to(data.dtype)

            return _AttachBackward.apply(data, result, rician_backward)
        data = data.contiguous()
        batch = data.shape[0]
        batched = isinstance(mean, Tensor) or isinstance(std, Tensor)
        mean_t = std_t = None
        if batched:
            mean_t = h2d(torch.as_tensor(mean, dtype=torch.float32), data.device).expand(batch).contiguous()
            std_t = h2d(torch.as_tensor(std, dtype=torch.float32), data.device).expand(batch).contiguous()
        for base in (base1, base2):
            if base is not None and (base.shape != data.shape or base.dtype != torch.float32):
                raise ValueError("base noise must be float32 and shaped like data")
        base1 = None if base1 is None else base1.contiguous()
        base2 = None if base2 is None else base2.contiguous()
        keep = self._flags(keep, batch, "keep")
        self._check("add_noise", data, mean_t, std_t, base1, base2, keep)
        out = torch.empty_like(data)
        n_per_element = data[0].numel() if batch else 0
        self._call(
            "add_noise", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, n_per_element,
            0.0 if batched else float(mean), 0.0 if batched else float(std), _ptr(mean_t), _ptr(std_t),
            int(batched), int(bool(rician)), _ptr(base1), _ptr(base2), int(philox_seed) & (2**64 - 1),
            _ptr(keep), self._stream(data),
        )
        return out

    def philox_normal(self, shape: Sequence[int], seed: int, stream_id: int, device) -> Tensor:
        """Standard normals of the fast noise mode (Philox4x32-10 + Box-Muller)."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        self._check("philox_normal", out)
        self._call(
            "philox_normal", out, _ptr(out), out.numel(), int(seed) & (2**64 - 1), int(stream_id),
            self._stream(out),
        )
        return out

    def gamma_pow(self, data: Tensor, gamma: float | Tensor) -> Tensor:
        """``sign(data) * |data| ** gamma`` with a scalar or per-element ``(B,)`` exponent."""
        if data.dtype not in FLOAT_DTYPES:
            raise TypeError(f"gamma_pow needs a floating dtype, got {data.dtype}")
        if isinstance(gamma, Tensor) and _wants_grad(gamma):
            self._parameter_kernel("gamma_grad", "gamma_pow: gamma")
            values, source = h2d(gamma.detach().to(torch.float32), data.device), data.detach()
            result = self.gamma_pow(data, values)
            return _AttachParameterBackward.apply("gamma_pow", lambda grad, wants: [self.gamma_grad(source, grad, values)], result, gamma)
        if _wants_grad(data):  # y = sign(x) |x|^g: dy/dx = g |x|^(g - 1)
            detached = data.detach()
            result = self.gamma_pow(detached, gamma)

            def backward(grad):
                exponent = gamma.to(detached.device, torch.float32).reshape((-1,) + (1,) * (detached.ndim - 1)) if isinstance(gamma, Tensor) else float(gamma)
                return (grad.float() * exponent * detached.float().abs().pow(exponent - 1)).to(data.dtype)

            return _AttachBackward.apply(data, result, backward)
        data = data.contiguous()
        batch = data.shape[0]
        gamma_t = None
        if isinstance(gamma, Tensor):
            gamma_t = h2d(gamma.to(torch.float32), data.device).expand(batch).contiguous()
        self._check("gamma_pow", data, gamma_t)
        out = torch.empty_like(data)
        self._call(
            "gamma_pow", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch,
            data[0].numel() if batch else 0, 0.0 if gamma_t is not None else float(gamma), _ptr(gamma_t),
            int(gamma_t is not None), self._stream(data),
        )
        return out

    # -- gradients with respect to the parameters of the four ops above (intensity_param_grad.hip; nothing here takes part in autograd)
    def _grad_pair(self, what: str, data: Tensor, grad: Tensor) -> tuple[Tensor, Tensor]:
        if data.dtype not in FLOAT_DTYPES:
            raise TypeError(f"{what} needs a floating dtype, got {data.dtype}")
        if tuple(grad.shape) != tuple(data.shape):
            raise ValueError(f"{what}: the gradient {tuple(grad.shape)} is not shaped like the data {tuple(data.shape)}")
        return data.detach().contiguous(), grad.detach().to(torch.float32).contiguous()

    def _shared_or_batched(self, value: float | Tensor, batch: int, device, what: str) -> Tensor | float:
        """A parameter as the kernels take it: a number, or a float32 device tensor of 1 or *batch* values."""
        if not isinstance(value, Tensor):
            return float(value)
        if value.numel() not in (1, batch):
            raise ValueError(f"{what} must hold 1 or {batch} values, got {tuple(value.shape)}")
        return h2d(value.detach().to(torch.float32), device).reshape(-1).contiguous()

    def bias_field_grad(self, data: Tensor, grad: Tensor, coarse: Tensor, *, divide: bool = False, skip: Tensor | None = None) -> Tensor:
        """``d <bias_field_apply(data, coarse), grad> / d coarse`` as a float32 tensor shaped like *coarse* (``tio_bias_field_grad``):
        ``s * sum_v grad * y * W(node; v)`` with the forward's own field and lerp weights, one read of *data* and *grad*."""
        if data.ndim != 5 or coarse.ndim != 5 or coarse.shape[:2] != data.shape[:2]:
            raise ValueError("data and coarse must be 5-D with the same (B, C)")
        with torch.no_grad():
            data, grad = self._grad_pair("bias_field_grad", data, grad)
            coarse = h2d(coarse.detach().to(torch.float32), data.device).contiguous()
            skip = self._flags(skip, data.shape[0], "skip")
            if skip is not None and skip.device != data.device:
                skip = skip.to(data.device)
            self._check("bias_field_grad", data, grad, coarse, skip)
            out = torch.empty_like(coarse)
            workspace, nbytes = self._workspace("bias_field_grad_workspace_bytes", data, data.shape[0], data.shape[1], _i32x3(coarse.shape[2:]))
            self._call(
                "bias_field_grad", data, _ptr(data), _ptr(grad), dtype_code(data.dtype), data.shape[0], data.shape[1], _i32x3(data.shape[2:]),
                _ptr(coarse), _i32x3(coarse.shape[2:]), int(bool(divide)), _ptr(skip), _ptr(out), _ptr(workspace), nbytes, self._stream(data),
            )
        return out

    def gamma_grad(self, data: Tensor, grad: Tensor, gamma: float | Tensor) -> Tensor:
        """``d <gamma_pow(data, gamma), grad> / d gamma`` (``tio_gamma_grad``): ``sum grad * y * log|x|`` over ``x != 0``, float32,
        one value per element for a ``(B,)`` exponent (``B > 1``), else one value."""
        with torch.no_grad():
            data, grad = self._grad_pair("gamma_grad", data, grad)
            batch = data.shape[0]
            gamma = self._shared_or_batched(gamma, batch, data.device, "gamma")
            gamma_t = gamma if isinstance(gamma, Tensor) else None
            batched = gamma_t is not None and gamma_t.numel() == batch and batch > 1
            self._check("gamma_grad", data, grad, gamma_t)
            out = torch.empty(batch if batched else 1, dtype=torch.float32, device=data.device)
            workspace, nbytes = self._workspace("gamma_grad_workspace_bytes", data, batch, int(batched))
            self._call(
                "gamma_grad", data, _ptr(data), _ptr(grad), dtype_code(data.dtype), batch, data[0].numel() if batch else 0,
                0.0 if gamma_t is not None else gamma, _ptr(gamma_t), int(batched), _ptr(out), _ptr(workspace), nbytes, self._stream(data),
            )
        return out

    def noise_grad(
        self,
        data: Tensor,
        grad: Tensor,
        mean: float | Tensor,
        std: float | Tensor,
        *,
        rician: bool = False,
        base1: Tensor | None = None,
        base2: Tensor | None = None,
        philox_seed: int = 0,
        keep: Tensor | None = None,
        want_mean: bool = True,
        want_std: bool = True,
    ) -> tuple[Tensor | None, Tensor | None]:
        """``d <add_noise(data, mean, std, ...), grad> / d (mean, std)`` (``tio_noise_grad``), float32, ``None`` for the one that
        is not wanted.  With *base1* ``None`` the draws are regenerated from *philox_seed* in the kernel.  Each result has as many
        values as its parameter (a number counts as one); where one parameter holds ``B`` values and the other one, the single
        one's ``B`` per-element sums are added in float64."""
        if not (want_mean or want_std):
            return None, None
        with torch.no_grad():
            data, grad = self._grad_pair("noise_grad", data, grad)
            batch = data.shape[0]
            mean = self._shared_or_batched(mean, batch, data.device, "mean")
            std = self._shared_or_batched(std, batch, data.device, "std")
            sizes = [p.numel() if isinstance(p, Tensor) else 1 for p in (mean, std)]
            batched = batch > 1 and max(sizes) == batch
            mean_t = std_t = None
            if isinstance(mean, Tensor) or isinstance(std, Tensor):  # device values: B of each when either holds B, else the shared ones
                count = batch if batched else 1
                mean_t = torch.as_tensor(mean, dtype=torch.float32, device=data.device).expand(count).contiguous()
                std_t = torch.as_tensor(std, dtype=torch.float32, device=data.device).expand(count).contiguous()
            for base in (base1, base2):
                if base is not None and (base.shape != data.shape or base.dtype != torch.float32):
                    raise ValueError("base noise must be float32 and shaped like data")
            base1 = None if base1 is None else base1.detach().contiguous()
            base2 = None if base2 is None else base2.detach().contiguous()
            keep = self._flags(keep, batch, "keep")
            if keep is not None and keep.device != data.device:
                keep = keep.to(data.device)
            self._check("noise_grad", data, grad, mean_t, std_t, base1, base2, keep)
            groups = batch if batched else 1
            d_mean = torch.empty(groups, dtype=torch.float32, device=data.device) if want_mean else None
            d_std = torch.empty(groups, dtype=torch.float32, device=data.device) if want_std else None
            workspace, nbytes = self._workspace("noise_grad_workspace_bytes", data, batch, int(batched))
            self._call(
                "noise_grad", data, _ptr(data), _ptr(grad), dtype_code(data.dtype), batch, data[0].numel() if batch else 0,
                0.0 if mean_t is not None else mean, 0.0 if std_t is not None else std, _ptr(mean_t), _ptr(std_t), int(batched),
                int(bool(rician)), _ptr(base1), _ptr(base2), int(philox_seed) & (2**64 - 1), _ptr(keep), _ptr(d_mean), _ptr(d_std),
                _ptr(workspace), nbytes, self._stream(data),
            )
            if batched:  # a single value next to B of the other: its per-element sums, added in float64
                if d_mean is not None and sizes[0] == 1:
                    d_mean = d_mean.double().sum().float().reshape(1)
                if d_std is not None and sizes[1] == 1:
                    d_std = d_std.double().sum().float().reshape(1)
        return d_mean, d_std

    def separable_conv3d_taps_grad(self, data: Tensor, grad: Tensor, taps: Tensor, radius: Sequence[int], skip: Tensor | None = None) -> Tensor:
        """``d <separable_conv3d(data, taps, radius), grad> / d taps`` as a float32 tensor shaped like *taps*
        (``tio_separable_conv3d_taps_grad``): per active axis one clamped tap correlation of the gradient carried back through the
        later axes with the data carried forward through the earlier ones; zero beyond ``2 * radius + 1``."""
        if data.ndim != 5:
            raise ValueError("expected a (B, C, I, J, K) tensor")
        with torch.no_grad():
            data, grad = self._grad_pair("separable_conv3d_taps_grad", data, grad)
            batch, channels = data.shape[:2]
            taps = h2d(taps.detach().to(torch.float32), data.device).contiguous()
            if taps.ndim != 3 or taps.shape[1] != 3 or taps.shape[0] not in (1, batch):
                raise ValueError(f"taps must be (1|B, 3, stride), got {tuple(taps.shape)}")
            skip = self._flags(skip, batch, "skip")
            if skip is not None and skip.device != data.device:
                skip = skip.to(data.device)
            self._check("separable_conv3d_taps_grad", data, grad, taps, skip)
            batched = int(taps.shape[0] == batch and batch > 1)
            out = torch.empty_like(taps)
            scratch = torch.empty((2, *data.shape), dtype=torch.float32, device=data.device)
            workspace, nbytes = self._workspace("separable_conv3d_taps_grad_workspace_bytes", data, batch, batched)
            self._call(
                "separable_conv3d_taps_grad", data, _ptr(data), dtype_code(data.dtype), _ptr(grad), _ptr(scratch), batch, channels,
                _i32x3(data.shape[2:]), _ptr(taps), batched, taps.shape[2], _i32x3(radius), _ptr(skip), _ptr(out), _ptr(workspace), nbytes,
                self._stream(data),
            )
        return out


    # -- F.interpolate users ---------------------------------------------------
    def interpolate3d(self, data: Tensor, out_shape: Sequence[int], mode: str) -> Tensor:
        """``F.interpolate(data.float(), size=out_shape, mode).to(data.dtype)``: ``"nearest"`` or ``"linear"`` (trilinear, align_corners)."""
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if _wants_grad(data) and mode in ("nearest", "linear"):  # linear in the data: the backward is its transpose, a gather
            self._data_adjoint_kernel("interpolate3d_adjoint", "interpolate3d: the data requires a gradient")
            result = self.interpolate3d(data.detach(), out_shape, mode)
            in_shape = tuple(data.shape[2:])
            return _AttachBackward.apply(data, result, lambda grad: self.interpolate3d_adjoint(grad, in_shape, mode).to(data.dtype))
        data = data.contiguous()
        self._check("interpolate3d", data)
        out_shape = tuple(int(s) for s in out_shape)
        out = torch.empty((*data.shape[:2], *out_shape), dtype=data.dtype, device=data.device)
        self._call(
            "interpolate3d", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0] * data.shape[1],
            _i32x3(data.shape[2:]), _i32x3(out_shape), INTERP_CODES[mode], self._stream(data),
        )
        return out

    def interpolate3d_adjoint(self, grad: Tensor, in_shape: Sequence[int], mode: str) -> Tensor:
        """The transpose of ``interpolate3d(., grad.shape[2:], mode)`` applied to *grad* ``(B, C, *out_shape)``: dL/d(input),
        float32 ``(B, C, *in_shape)`` (``tio_interpolate3d_adjoint``: one thread per input voxel, no atomics, reproducible)."""
        if grad.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) gradient, got {tuple(grad.shape)}")
        if mode not in ("nearest", "linear"):
            raise ValueError(f'interpolate3d_adjoint: mode must be "nearest" or "linear", got {mode!r}')
        self._data_adjoint_kernel("interpolate3d_adjoint", "interpolate3d_adjoint")
        grad = grad.to(torch.float32).contiguous()
        self._check("interpolate3d_adjoint", grad)
        in_shape = tuple(int(s) for s in in_shape)
        out = torch.empty((*grad.shape[:2], *in_shape), dtype=torch.float32, device=grad.device)
        self._call("interpolate3d_adjoint", grad, _ptr(grad), _ptr(out), grad.shape[0] * grad.shape[1], _i32x3(in_shape),
                   _i32x3(grad.shape[2:]), INTERP_CODES[mode], self._stream(grad))
        return out

    def axis_gather_lerp(self, data: Tensor, axis: int, lower: Tensor, upper: Tensor | None = None,
                         weight: Tensor | None = None, active: Tensor | None = None) -> Tensor:
        """Per-element gather (``upper is None``) or two-point blend along one spatial axis; tables are ``(B, length)``."""
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        data = data.contiguous()
        batch, length = data.shape[0], data.shape[2 + axis]

        def table(t, dtype):
            if t is None:
                return None
            t = h2d(t.to(dtype).contiguous(), data.device)
            if tuple(t.shape) != (batch, length):
                raise ValueError(f"index / weight tables must be (B, length) = {(batch, length)}, got {tuple(t.shape)}")
            return t

        lower, upper, weight = table(lower, torch.int32), table(upper, torch.int32), table(weight, torch.float32)
        active = self._flags(active, batch, "active")
        if active is not None:
            active = h2d(active, data.device)
        if _wants_grad(data):  # linear in the data: the backward gathers along the inverted tables (already on the device)
            self._data_adjoint_kernel("axis_gather_lerp_adjoint", "axis_gather_lerp: the data requires a gradient")
            result = self.axis_gather_lerp(data.detach(), axis, lower, upper, weight, active)
            return _AttachBackward.apply(
                data, result, lambda grad: self.axis_gather_lerp_adjoint(grad, axis, lower, upper, weight, active).to(data.dtype))
        self._check("axis_gather_lerp", data, lower, upper, weight, active)
        out = torch.empty_like(data)
        self._call(
            "axis_gather_lerp", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, data.shape[1], _i32x3(data.shape[2:]),
            int(axis), _ptr(lower), _ptr(upper), _ptr(weight), _ptr(active), self._stream(data),
        )
        return out

    @staticmethod
    def axis_gather_lists(lower: Tensor, upper: Tensor | None = None, weight: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor | None]:
        """The ``(B, length)`` tables of ``axis_gather_lerp`` inverted into one list per source index, with torch ops on the
        tables' own device and no read-back: ``offsets`` int32 ``(B, length + 1)``, ``positions`` int32 ``(B, E)`` and
        ``weights`` float32 ``(B, E)`` (``None`` for the nearest form), ``E = length`` or ``2 * length``.  The entries
        ``offsets[b, p] .. offsets[b, p + 1]`` of element ``b`` are the outputs that read source ``p``: the ``lower`` uses by
        ascending position with the weight ``1 - w`` (rounded as the forward rounds it), then the ``upper`` uses with ``w``
        (a stable sort by source).  Entries whose source lies outside ``[0, length)`` belong to no list."""
        batch, length = lower.shape
        positions = torch.arange(length, dtype=torch.int32, device=lower.device)
        if upper is None:
            sources, positions, weights = lower, positions.expand(batch, length), None
        else:
            sources = torch.cat([lower, upper], dim=1)
            positions = torch.cat([positions, positions]).expand(batch, 2 * length)
            weights = torch.cat([1.0 - weight, weight], dim=1)
        sources, order = torch.sort(sources.to(torch.int32), dim=1, stable=True)
        ends = torch.arange(length + 1, dtype=torch.int32, device=lower.device).expand(batch, length + 1).contiguous()
        offsets = torch.searchsorted(sources.contiguous(), ends, out_int32=True)
        positions = positions.gather(1, order).contiguous()
        return offsets.contiguous(), positions, None if weights is None else weights.gather(1, order).contiguous()

    def axis_gather_lerp_adjoint(self, grad: Tensor, axis: int, lower: Tensor, upper: Tensor | None = None,
                                 weight: Tensor | None = None, active: Tensor | None = None) -> Tensor:
        """The transpose of ``axis_gather_lerp(., axis, lower, upper, weight, active)`` applied to *grad*: dL/d(input), float32
        (``tio_axis_gather_lerp_adjoint`` over the lists of ``axis_gather_lists``; inactive elements pass *grad* on)."""
        if grad.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) gradient, got {tuple(grad.shape)}")
        self._data_adjoint_kernel("axis_gather_lerp_adjoint", "axis_gather_lerp_adjoint")
        grad = grad.to(torch.float32).contiguous()
        batch, length = grad.shape[0], grad.shape[2 + axis]
        tables = [None if t is None else h2d(t.to(dtype).contiguous(), grad.device)
                  for t, dtype in ((lower, torch.int32), (upper, torch.int32), (weight, torch.float32))]
        for t in tables:
            if t is not None and tuple(t.shape) != (batch, length):
                raise ValueError(f"index / weight tables must be (B, length) = {(batch, length)}, got {tuple(t.shape)}")
        if tables[1] is not None and tables[2] is None:
            raise ValueError("axis_gather_lerp_adjoint: upper without weights")
        active = self._flags(active, batch, "active")
        if active is not None:
            active = h2d(active, grad.device)
        offsets, positions, weights = self.axis_gather_lists(*tables)
        self._check("axis_gather_lerp_adjoint", grad, offsets, positions, weights, active)
        out = torch.empty_like(grad)
        self._call("axis_gather_lerp_adjoint", grad, _ptr(grad), _ptr(out), batch, grad.shape[1], _i32x3(grad.shape[2:]), int(axis),
                   _ptr(offsets), _ptr(positions), _ptr(weights), positions.shape[1], _ptr(active), self._stream(grad))
        return out

    def flip3d(self, data: Tensor, axes: Sequence[int] | None = None, per_element: Tensor | None = None) -> Tensor:
        """``torch.flip`` along spatial ``axes`` (0..2), or per element with a ``(B, 3)`` flag tensor."""
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if _wants_grad(data):  # a permutation: its transpose is itself
            result = self.flip3d(data.detach(), axes, per_element)
            return _AttachBackward.apply(data, result, lambda grad: self.flip3d(grad, axes, per_element))
        data = data.contiguous()
        mask = 0
        for axis in axes or ():
            if axis not in (0, 1, 2):
                raise ValueError(f"Axis must be 0, 1, or 2; got {axis}")
            mask |= 1 << axis
        flags = None
        if per_element is not None:
            if tuple(per_element.shape) != (data.shape[0], 3):
                raise ValueError(f"per-element flags must be (B, 3), got {tuple(per_element.shape)}")
            flags = h2d(per_element.to(torch.uint8).contiguous(), data.device)
        self._check("flip3d", data, flags)
        out = torch.empty_like(data)
        self._call("flip3d", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], data.shape[1],
                   _i32x3(data.shape[2:]), mask, _ptr(flags), self._stream(data))
        return out

    def permute3d(self, data: Tensor, perm: Sequence[int], flip_axes: Sequence[int] = ()) -> Tensor:
        """``torch.flip(data, flip_axes)`` (spatial input axes 0..2), then ``permute(0, 1, 2 + perm[0], 2 + perm[1],
        2 + perm[2]).contiguous()``, as one launch (``tio_permute3d``: nibabel's ``apply_orientation`` order)."""
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        perm = [int(p) for p in perm]
        if sorted(perm) != [0, 1, 2]:
            raise ValueError(f"perm must be a permutation of (0, 1, 2), got {tuple(perm)}")
        mask = 0
        for axis in flip_axes:
            if axis not in (0, 1, 2):
                raise ValueError(f"Axis must be 0, 1, or 2; got {axis}")
            mask |= 1 << int(axis)
        if _wants_grad(data):  # the transpose of a permutation is its inverse: the flips move to the axes they land on
            result = self.permute3d(data.detach(), perm, flip_axes)
            inverse = [perm.index(d) for d in range(3)]
            carried = [d for d in range(3) if mask & (1 << perm[d])]
            return _AttachBackward.apply(data, result, lambda grad: self.permute3d(grad, inverse, carried))
        data = data.contiguous()
        self._check("permute3d", data)
        out = torch.empty((*data.shape[:2], *(data.shape[2 + p] for p in perm)), dtype=data.dtype, device=data.device)
        self._call("permute3d", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], data.shape[1],
                   _i32x3(data.shape[2:]), _i32x3(perm), mask, self._stream(data))
        return out

    def pad3d(self, data: Tensor, padding: Sequence[int], mode: str = "constant", fill: float = 0.0,
              fill_per_element: Tensor | None = None) -> Tensor:
        """``F.pad`` of the three spatial axes: ``padding = (i0, i1, j0, j1, k0, k1)``, ``mode`` as in ``F.pad``.

        ``fill_per_element``: ``(B,)`` constants (one per batch element, any dtype: cast to the data's).
        """
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        code = {"constant": _abi.PAD_CONSTANT, "reflect": _abi.PAD_REFLECT, "replicate": _abi.PAD_REPLICATE, "circular": _abi.PAD_CIRCULAR}[mode]
        if _wants_grad(data) or _wants_grad(fill_per_element):
            if mode == "constant":
                return _PadConstantFn.apply(data, fill_per_element, self, [int(p) for p in padding], float(fill))
            if not _wants_grad(data):
                raise EngineError(f"pad3d: fill values take no part in mode {mode!r}, they have no gradient there (constant / statistic padding)")
            # the border repeats voxels of the image: the backward folds it back onto them (a gather per input voxel)
            self._data_adjoint_kernel("pad3d_adjoint", f"pad3d: the data requires a gradient through mode {mode!r}")
            fills = None if fill_per_element is None else fill_per_element.detach()
            result = self.pad3d(data.detach(), padding, mode, fill, fills)
            in_shape, padding = tuple(data.shape[2:]), [int(p) for p in padding]
            return _AttachBackward.apply(data, result, lambda grad: self.pad3d_adjoint(grad, in_shape, padding, mode).to(data.dtype))
        data = data.contiguous()
        padding = [int(p) for p in padding]
        if len(padding) != 6:
            raise ValueError("padding must have 6 values (i0, i1, j0, j1, k0, k1)")
        shape = [data.shape[2 + d] + padding[2 * d] + padding[2 * d + 1] for d in range(3)]
        fills = None
        if fill_per_element is not None:
            fills = fill_per_element.to(device=data.device, dtype=data.dtype).contiguous()
            if fills.numel() != data.shape[0]:
                raise ValueError("one fill value per batch element")
        self._check("pad3d", data, fills)
        out = torch.empty((*data.shape[:2], *shape), dtype=data.dtype, device=data.device)
        self._call("pad3d", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], data.shape[1], _i32x3(data.shape[2:]),
                   (C.c_int32 * 6)(*padding), code, float(fill), _ptr(fills), self._stream(data))
        return out

    def pad3d_adjoint(self, grad: Tensor, in_shape: Sequence[int], padding: Sequence[int], mode: str) -> Tensor:
        """The transpose of ``pad3d(., padding, mode)`` for ``"reflect"`` / ``"replicate"`` / ``"circular"`` applied to *grad*
        ``(B, C, *(in_shape + padding))``: dL/d(input), float32 ``(B, C, *in_shape)`` (``tio_pad3d_adjoint``)."""
        if grad.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) gradient, got {tuple(grad.shape)}")
        if mode not in ("reflect", "replicate", "circular"):
            raise ValueError(f'pad3d_adjoint: mode must be "reflect", "replicate" or "circular", got {mode!r}')
        code = {"reflect": _abi.PAD_REFLECT, "replicate": _abi.PAD_REPLICATE, "circular": _abi.PAD_CIRCULAR}[mode]
        in_shape, padding = [int(s) for s in in_shape], [int(p) for p in padding]
        if len(padding) != 6:
            raise ValueError("padding must have 6 values (i0, i1, j0, j1, k0, k1)")
        if [in_shape[d] + padding[2 * d] + padding[2 * d + 1] for d in range(3)] != list(grad.shape[2:]):
            raise ValueError(f"pad3d_adjoint: a gradient of {tuple(grad.shape[2:])} is not {tuple(in_shape)} padded by {tuple(padding)}")
        self._data_adjoint_kernel("pad3d_adjoint", "pad3d_adjoint")
        grad = grad.to(torch.float32).contiguous()
        self._check("pad3d_adjoint", grad)
        out = torch.empty((*grad.shape[:2], *in_shape), dtype=torch.float32, device=grad.device)
        self._call("pad3d_adjoint", grad, _ptr(grad), _ptr(out), grad.shape[0], grad.shape[1], _i32x3(in_shape),
                   (C.c_int32 * 6)(*padding), code, self._stream(grad))
        return out

    def unique_labels(self, data: Tensor) -> Tensor:
        """``torch.unique(data).double()`` (sorted) of a label map; a bitmap pass for 8- / 16-bit integers.

        One 4-byte read-back of the count, like ``torch.unique`` itself (the table's length is a host quantity).
        """
        if data.dtype not in (torch.uint8, torch.int8, torch.int16):
            return torch.unique(data).to(torch.float64)  # wide / floating label maps: ATen's sort
        data = data.contiguous()
        if data.data_ptr() % 16 != 0:
            data = data.clone()
        self._check("unique_labels", data)
        capacity = 256 if data.dtype != torch.int16 else 65536
        table = torch.empty(capacity, dtype=torch.float64, device=data.device)
        count = torch.empty(1, dtype=torch.int32, device=data.device)
        workspace = torch.empty(2048, dtype=torch.int32, device=data.device)
        self._call("unique_labels", data, _ptr(data), dtype_code(data.dtype), data.numel(), _ptr(table), _ptr(count), _ptr(workspace),
                   self._stream(data))
        return table[: int(count.item())]

    # -- label-map transforms (transforms/label/*.py of the reference) ---------------------------------------------------
    def label_remap(self, data: Tensor, mapping, *, default: float | None = None, inplace: bool = False) -> Tensor:
        """``out[v] = mapping[data[v]]`` for every pair at once, compared against the ORIGINAL values (``{1: 2, 2: 1}`` swaps).

        A value that is no key stays (``default=None``) or becomes ``default``.  ``mapping``: a dict or a sequence of
        ``(old, new)`` pairs with unique keys (at most 65536).  ``inplace=True`` writes into ``data`` (which must be dense).
        """
        pairs = sorted((float(old), float(new)) for old, new in (mapping.items() if hasattr(mapping, "items") else mapping))
        if len({old for old, _ in pairs}) != len(pairs):
            raise ValueError("label_remap: the keys of the mapping must be unique")
        if len(pairs) > _abi.REMAP_MAX_PAIRS:
            raise ValueError(f"label_remap: at most {_abi.REMAP_MAX_PAIRS} pairs, got {len(pairs)}")
        if inplace and not data.is_contiguous():
            raise ValueError("label_remap: inplace needs a contiguous tensor")
        data = data.contiguous()
        table = None
        if pairs:
            table = h2d(torch.tensor(pairs, dtype=torch.float64).t().contiguous(), data.device)  # row 0: keys, row 1: values
        self._check("label_remap", data, table)
        out = data if inplace else torch.empty_like(data)
        scratch = torch.empty(65536, dtype=torch.int16, device=data.device) if data.dtype == torch.int16 else None
        mode = _abi.REMAP_KEEP if default is None else _abi.REMAP_CONSTANT
        self._call("label_remap", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.numel(),
                   None if table is None else C.c_void_p(table[0].data_ptr()), None if table is None else C.c_void_p(table[1].data_ptr()),
                   len(pairs), mode, 0.0 if default is None else float(default), _ptr(scratch), self._stream(data))
        return out

    def label_one_hot(self, data: Tensor, num_classes: int = -1) -> Tensor:
        """``F.one_hot(data[:, 0].long(), num_classes)`` as float32 ``(B, num_classes, I, J, K)``; ``-1``: ``max + 1``.

        One 4-byte read-back (the status word; ``F.one_hot`` synchronises for the same check), one more to infer the classes.
        """
        if data.ndim != 5 or data.shape[1] != 1:
            raise ValueError(f"expected a (B, 1, I, J, K) label map, got {tuple(data.shape)}")
        data = data.contiguous()
        self._check("label_one_hot", data)
        num_classes = int(num_classes)
        if num_classes < 0:
            if data.numel() == 0:
                raise RuntimeError("Can not infer total number of classes from empty tensor.")
            num_classes = int(data.max().item()) + 1
            if num_classes <= 0:
                raise RuntimeError("Class values must be non-negative.")
        out = torch.empty((data.shape[0], num_classes, *data.shape[2:]), dtype=torch.float32, device=data.device)
        status = torch.empty(1, dtype=torch.int32, device=data.device)
        spatial = data.shape[2] * data.shape[3] * data.shape[4]
        self._call("label_one_hot", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], spatial, num_classes, _ptr(status),
                   self._stream(data))
        if data.numel() and int(status.item()) != 0:
            raise RuntimeError(f"label_one_hot: class values must be integers in [0, {num_classes})")
        return out

    def label_contour(self, data: Tensor) -> Tensor:
        """The reference's ``_extract_contour``: float32 1 where the 27-point minimum (-1 outside the volume) differs from the voxel."""
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        data = data.contiguous()
        self._check("label_contour", data)
        out = torch.empty(data.shape, dtype=torch.float32, device=data.device)
        self._call("label_contour", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0] * data.shape[1], _i32x3(data.shape[2:]),
                   self._stream(data))
        return out

    def keep_largest_component(self, data: Tensor, labels, *, background: float = 0, fully_connected: bool = True) -> Tensor:
        """Per batch element and listed label value, every connected component but the largest becomes ``background``.

        ``labels``: numbers, or a float64 tensor on the data's device (sorted, unique — ``unique_labels``'s result).  All labels
        of a call are handled by one pass; a list beyond the library's cap is split into several.
        """
        if data.ndim != 5:
            raise ValueError(f"expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if data.shape[1] != 1:
            raise RuntimeError(f"KeepLargestComponent requires single-channel label maps, got {data.shape[1]} channels")
        data = data.contiguous()
        if not isinstance(labels, Tensor):
            values = sorted({float(v) for v in labels})
            labels = h2d(torch.tensor(values, dtype=torch.float64), data.device) if values else None
        elif labels.numel() == 0:
            labels = None
        else:
            labels = labels.to(torch.float64).contiguous()
        self._check("keep_largest_component", data, labels)
        if labels is None:
            return data.clone()
        shape = _i32x3(data.shape[2:])
        result = None
        for begin in range(0, labels.numel(), _abi.KEEP_LARGEST_MAX_LABELS):
            chunk = labels[begin : begin + _abi.KEEP_LARGEST_MAX_LABELS]
            out = torch.empty_like(data)
            nbytes = int(self._fn["keep_largest_workspace_bytes"](data.shape[0], shape, chunk.numel()))
            workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=data.device)
            self._call("keep_largest_component", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.shape[0], shape, _ptr(chunk),
                       chunk.numel(), float(background), int(bool(fully_connected)), _ptr(workspace), nbytes, self._stream(data))
            # (every chunk works on the original data: a removed voxel never counts for a later chunk's label)
            result = out if result is None else torch.where(out != data, out, result)
        return result

    # -- LabelsToImage (transforms/intensity/labels_to_image.py) ---------------------------------------------------------
    def labels_to_image(self, labels: Tensor, keys, means, stds, *, seed: int | None = None, base: Tensor | None = None,
                        base_key: int | None = None, out: Tensor | None = None) -> Tensor:
        """The synthetic float32 ``(B, 1, I, J, K)`` image of a ``(B, C, I, J, K)`` label map (channel 0 is read).

        ``keys``: the label values, strictly ascending; ``means`` / ``stds``: one value per key, or ``(B, len(keys))`` of
        them for per-element parameters.  A voxel whose label is no key becomes 0.

        Fused mode (``seed``): one launch, ``mean + std * z`` with ``z = philox_normal(out.shape, seed, 0)``.
        One-label mode (``base``, ``base_key``): only ``keys[base_key]`` is looked at; its voxels become
        ``base * std + mean`` with the caller's float32 normals ``base`` (shaped like the result), every other voxel keeps
        what ``out`` holds (``out=None``: zeros).  Called once per label with ``torch.randn`` draws this is the reference.
        """
        what = "labels_to_image"
        if labels.ndim != 5:
            raise ValueError(f"{what}: expected a (B, C, I, J, K) tensor, got {tuple(labels.shape)}")
        if (seed is None) == (base is None):
            raise ValueError(f"{what}: give either seed (fused mode) or base and base_key (one-label mode)")
        batch, channels = int(labels.shape[0]), int(labels.shape[1])
        keys_t = keys.detach().to(torch.float64).reshape(-1) if isinstance(keys, Tensor) else torch.tensor([float(k) for k in keys], dtype=torch.float64)
        n_keys = keys_t.numel()
        if n_keys > _abi.REMAP_MAX_PAIRS:
            raise ValueError(f"{what}: at most {_abi.REMAP_MAX_PAIRS} keys, got {n_keys}")
        if n_keys > 1 and not bool((keys_t[1:] > keys_t[:-1]).all()):  # (keys on the device: one read-back)
            raise ValueError(f"{what}: the keys must be strictly ascending")
        mean_t, std_t = (torch.as_tensor(v, dtype=torch.float32) for v in (means, stds))
        if mean_t.shape != std_t.shape or tuple(mean_t.shape) not in ((n_keys,), (batch, n_keys)):
            raise ValueError(f"{what}: means {tuple(mean_t.shape)} and stds {tuple(std_t.shape)} for {n_keys} keys and a batch of {batch}")
        batched = mean_t.ndim == 2
        result_shape = (batch, 1, *labels.shape[2:])
        if base is not None:
            if base_key is None or not 0 <= int(base_key) < n_keys:
                raise ValueError(f"{what}: base_key {base_key!r} outside [0, {n_keys})")
            if tuple(base.shape) != result_shape or base.dtype != torch.float32:
                raise ValueError(f"{what}: base must be float32 of shape {result_shape}")
            base = base.contiguous()
        if out is not None:
            if base is None:
                raise ValueError(f"{what}: out is reused in one-label mode only")
            if tuple(out.shape) != result_shape or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError(f"{what}: out must be contiguous float32 of shape {result_shape}")
        labels = labels.contiguous()
        device = labels.device
        # (the doubles travel as pairs of float32 words: one staging copy for the three blocks)
        keys_dev, mean_dev, std_dev = h2d_packed([keys_t.contiguous().view(torch.float32) if keys_t.device.type == "cpu" else keys_t, mean_t.contiguous(), std_t.contiguous()], device)
        if keys_dev.dtype != torch.float64:
            keys_dev = keys_dev.view(torch.float64)
        self._check(what, labels, keys_dev, mean_dev, std_dev, base, out)
        if out is None:
            out = torch.empty(result_shape, dtype=torch.float32, device=device)
            if base is not None:
                out.zero_()
        n_spatial = labels[0, 0].numel() if batch and channels else 0
        self._call(what, labels, _ptr(labels), dtype_code(labels.dtype), batch, channels, n_spatial, _ptr(keys_dev), n_keys, _ptr(mean_dev),
                   _ptr(std_dev), int(batched), _ptr(out), (int(seed) if seed is not None else 0) & (2**64 - 1), _ptr(base),
                   int(base_key) if base is not None else 0, self._stream(labels))
        return out

    # -- intensity preprocessing with on-device statistics (normalize.py, standardize.py, clamp.py, mask.py) -------------
    _MAP_MODES = {"rescale_clip": _abi.MAP_RESCALE_CLIP, "rescale": _abi.MAP_RESCALE, "sub_div": _abi.MAP_SUB_DIV, "mul_add": _abi.MAP_MUL_ADD}

    @staticmethod
    def _first_element_and_mask(data: Tensor, mask: Tensor | None, what: str) -> tuple[Tensor, Tensor | None]:
        """``data[0]`` as a dense ``(C, I, J, K)`` tensor and the mask as a dense ``(1 or C, I, J, K)`` one (bool as uint8)."""
        if data.ndim not in (4, 5):
            raise ValueError(f"{what}: expected a (B, C, I, J, K) or (C, I, J, K) tensor, got {tuple(data.shape)}")
        first = (data[0] if data.ndim == 5 else data).contiguous()
        if mask is not None:
            if mask.ndim != 4 or tuple(mask.shape[1:]) != tuple(first.shape[1:]) or mask.shape[0] not in (1, first.shape[0]):
                raise ValueError(f"{what}: a mask of shape {tuple(mask.shape)} does not broadcast over data of shape {tuple(first.shape)}")
            mask = mask.contiguous()
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)
        return first, mask

    def _statistics_call(self, name: str, first: Tensor, mask: Tensor | None, record_words: int, *extra) -> Tensor:
        """One statistics launch and its one read-back: the record as int64 words on the host."""
        record = torch.empty(record_words, dtype=torch.int64, device=first.device)
        nbytes = int(self._fn["intensity_stats_workspace_bytes"]())
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=first.device)
        spatial = first.shape[1] * first.shape[2] * first.shape[3]
        self._call(name, first, _ptr(first), dtype_code(first.dtype), first.shape[0], spatial, _ptr(mask),
                   0 if mask is None else dtype_code(mask.dtype), 0 if mask is None else mask.shape[0], *extra, _ptr(record), _ptr(workspace),
                   nbytes, self._stream(first))
        return record.cpu()

    def intensity_moments(self, data: Tensor, mask: Tensor | None = None) -> tuple[int, float, float]:
        """``(count, mean, std)`` of ``data[0]`` (all channels) inside ``mask`` — ``values.float().mean()`` / ``.std()`` of the
        reference's Standardize, accumulated in float64 and rounded once to float32; bitwise reproducible.

        ``mask``: ``(1 or C, I, J, K)`` on the device, any dtype, nonzero = inside.  One read-back of 16 bytes.  ``count == 0``:
        both NaN; ``count == 1``: ``std`` is NaN, as ``torch.std`` has it.
        """
        first, mask = self._first_element_and_mask(data, mask, "intensity_moments")
        self._check("intensity_moments", first, mask)
        record = self._statistics_call("intensity_moments", first, mask, 2)
        mean, std = record[1:].view(torch.float32).tolist()
        return int(record[0]), mean, std

    def _order_statistics(self, data: Tensor, fractions: Sequence[float], mask: Tensor | None = None) -> list[tuple[Tensor, Tensor, int]]:
        """Per fraction ``q``: ``(lower_value, upper_value, n)`` — with ``n`` the number of elements of ``data[0]`` inside
        ``mask`` and ``lower = floor(q * (n - 1))``, the ``(lower + 1)``-th and ``(lower + 2)``-th smallest of them
        (``torch.kthvalue``'s; the same value twice when ``lower == n - 1``) as 0-dim float32 CPU tensors; NaN when ``n == 0``.

        Selected on the device, two fractions per launch sequence and read-back (32 bytes).
        """
        fractions = [float(q) for q in fractions]
        for q in fractions:
            if not 0 <= q <= 1:
                raise ValueError(f"Only values 0 <= q <= 1 are supported, but got {q!r}")
        first, mask = self._first_element_and_mask(data, mask, "intensity_quantiles")
        self._check("intensity_quantiles", first, mask)
        found = []
        for begin in range(0, len(fractions), 2):
            chunk = fractions[begin : begin + 2]
            record = self._statistics_call("intensity_quantiles", first, mask, 2 * len(chunk), (C.c_double * len(chunk))(*chunk), len(chunk))
            selected = record.view(torch.float32)
            found += [(selected[4 * k], selected[4 * k + 1], int(record[2 * k + 1])) for k in range(len(chunk))]
        return found

    def intensity_quantiles(self, data: Tensor, fractions: Sequence[float], mask: Tensor | None = None, *, return_count: bool = False):
        """``[compute_quantile(values.float(), q) for q in fractions]`` of the reference (``_statistics.py:36-43``) as Python
        floats, ``values`` being ``data[0]`` inside ``mask``: the order statistics come from the device
        (``_order_statistics``), the interpolation is the reference's own ``lerp`` on 0-dim CPU tensors.

        Nothing inside the mask: ``ValueError``, or — with ``return_count=True``, which returns ``(values, count)`` — NaNs.
        """
        fractions = [float(q) for q in fractions]
        found = self._order_statistics(data, fractions, mask)
        count = found[0][2] if found else 0  # (the same for every fraction: the number of inside elements)
        values: list[float] = []
        for q, (lower_value, upper_value, _) in zip(fractions, found, strict=True):
            if count == 0:
                values.append(math.nan)
                continue
            index = q * (count - 1)
            lower = math.floor(index)
            value = lower_value if index == lower else lower_value.lerp(upper_value, index - lower)
            values.append(float(value.item()))
        if return_count:
            return values, count
        if fractions and count == 0:
            raise ValueError("intensity_quantiles: no element inside the mask")
        return values

    def intensity_map(self, data: Tensor, mode: str, *, in_min: float = 0.0, in_max: float = 0.0, in_range: float = 1.0,
                      out_min: float | Tensor = 0.0, out_range: float | Tensor = 1.0) -> Tensor:
        """One float32 pass over ``data`` of any dtype, every operation rounded on its own like ATen's CPU kernels:

        ``"rescale_clip"``  ``(clamp(x, in_min, in_max) - in_min) / in_range * out_range + out_min``  (Normalize);
        ``"rescale"``       ``(x - out_min) / out_range * in_range + in_min``  (its inverse);
        ``"sub_div"``       ``(x - in_min) / in_range``  (Standardize);
        ``"mul_add"``       ``x * in_range + in_min``  (its inverse).

        ``out_min`` / ``out_range``: numbers, or float32 device tensors with one value per batch element (the rescale modes);
        with tensors, ``"rescale"`` leaves an element whose ``out_range`` is 0 unchanged.
        """
        if mode not in self._MAP_MODES:
            raise ValueError(f"intensity_map: unknown mode {mode!r} (one of {sorted(self._MAP_MODES)})")
        if data.ndim < 1:
            raise ValueError("intensity_map: expected a tensor with a batch dimension")
        per_element = isinstance(out_min, Tensor)
        if per_element != isinstance(out_range, Tensor):
            raise ValueError("intensity_map: out_min and out_range are both numbers or both tensors")
        data = data.contiguous()
        batch = data.shape[0]
        if per_element:
            if mode not in ("rescale_clip", "rescale"):
                raise ValueError(f"intensity_map: mode {mode!r} takes no per-element parameters")
            if out_min.numel() != batch or out_range.numel() != batch or out_min.dtype != torch.float32 or out_range.dtype != torch.float32:
                raise ValueError(f"intensity_map: per-element out_min / out_range must hold {batch} float32 values")
            out_min, out_range = out_min.contiguous(), out_range.contiguous()
            self._check("intensity_map", data, out_min, out_range)
        else:
            self._check("intensity_map", data)
        out = torch.empty(data.shape, dtype=torch.float32, device=data.device)
        self._call("intensity_map", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, data.numel() // batch if batch else 0,
                   self._MAP_MODES[mode], float(in_min), float(in_max), float(in_range), 0.0 if per_element else float(out_min),
                   1.0 if per_element else float(out_range), _ptr(out_min) if per_element else None, _ptr(out_range) if per_element else None,
                   self._stream(data))
        return out

    @staticmethod
    def _promoted(dtype: torch.dtype) -> torch.dtype:
        """torch's result dtype for an op of a tensor with a Python float: floating dtypes stay, integers become float32."""
        return dtype if dtype in FLOAT_DTYPES else torch.float32

    def clamp(self, data: Tensor, out_min: float | None = None, out_max: float | None = None) -> Tensor:
        """``data.clamp(min=out_min, max=out_max)`` with Python numbers: NaN propagates, integer data becomes float32."""
        if out_min is None and out_max is None:
            raise RuntimeError("torch.clamp: At least one of 'min' or 'max' must not be None")
        data = data.contiguous()
        self._check("clamp", data)
        out = torch.empty(data.shape, dtype=self._promoted(data.dtype), device=data.device)
        self._call("intensity_clamp", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.numel(), int(out_min is not None),
                   0.0 if out_min is None else float(out_min), int(out_max is not None), 0.0 if out_max is None else float(out_max),
                   self._stream(data))
        return out

    def mask_where(self, data: Tensor, mask: Tensor, outside_value: float) -> Tensor:
        """``torch.where(mask.expand_as(data), data, outside_value)``: ``data`` is ``(B, C, I, J, K)``, ``mask`` ``(1 or C, I, J, K)``
        on the device, any dtype, nonzero = inside; broadcast over the batch (and the channels).  Integer data becomes float32."""
        if data.ndim != 5:
            raise ValueError(f"mask_where: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if mask.ndim != 4 or tuple(mask.shape[1:]) != tuple(data.shape[2:]) or mask.shape[0] not in (1, data.shape[1]):
            raise ValueError(f"mask_where: a mask of shape {tuple(mask.shape)} does not broadcast over data of shape {tuple(data.shape)}")
        data, mask = data.contiguous(), mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        self._check("mask_where", data, mask)
        out = torch.empty(data.shape, dtype=self._promoted(data.dtype), device=data.device)
        self._call("intensity_mask", data, _ptr(data), _ptr(out), dtype_code(data.dtype), data.numel(), _ptr(mask), dtype_code(mask.dtype),
                   mask.numel(), float(outside_value), self._stream(data))
        return out

    # -- Swap and HistogramStandardization (transforms/intensity/swap.py, histogram_standardization.py) ------------------
    def swap_patches(self, data: Tensor, locations, patch_size: Sequence[int]) -> Tensor:
        """``_apply_swaps`` / ``_apply_swaps_per_instance`` of the reference: ``data`` is ``(B, C, I, J, K)`` of any dtype,
        ``locations`` one list of ``((ai, aj, ak), (bi, bj, bk))`` origin pairs for the whole batch or one such list per batch
        element, applied one after the other to every channel; where a pair's patches overlap, the second one's write stays.

        One copy and one launch whatever the number of swaps; one packed upload carries the origins and the counts.
        """
        if data.ndim != 5:
            raise ValueError(f"swap_patches: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        patch = [int(p) for p in patch_size]
        shape = [int(s) for s in data.shape[2:]]
        if len(patch) != 3 or any(p < 1 for p in patch):
            raise ValueError(f"swap_patches: patch_size must be three positive integers, got {tuple(patch_size)}")
        if any(p > s for p, s in zip(patch, shape, strict=True)):
            raise ValueError(f"Patch size {tuple(patch)} cannot be larger than spatial shape {tuple(shape)}")
        locations = list(locations)

        def is_pair(entry) -> bool:  # ((ai, aj, ak), (bi, bj, bk)), as opposed to an element's list of such pairs
            return len(entry) == 2 and all(len(origin) == 3 and not hasattr(origin[0], "__len__") for origin in entry)

        shared = all(is_pair(entry) for entry in locations)
        lists = [locations] if shared else locations
        if not shared and len(lists) != data.shape[0]:
            raise ValueError(f"swap_patches: {len(lists)} location lists for a batch of {data.shape[0]}")
        s_max = max((len(entries) for entries in lists), default=0)
        packed = torch.zeros(len(lists) * (s_max * 6 + 1), dtype=torch.int32)
        if s_max:
            origins = packed[: len(lists) * s_max * 6].view(len(lists), s_max, 2, 3)
            for index, entries in enumerate(lists):
                if entries:
                    origins[index, : len(entries)] = torch.tensor(entries, dtype=torch.int32).view(len(entries), 2, 3)
            limit = torch.tensor([s - p for s, p in zip(shape, patch, strict=True)], dtype=torch.int32)
            if bool((origins < 0).any()) or bool((origins > limit).any()):
                raise ValueError(f"swap_patches: an origin lies outside [0, shape - patch] = [0, {tuple(limit.tolist())}]")
        packed[len(lists) * s_max * 6 :] = torch.tensor([len(entries) for entries in lists], dtype=torch.int32)
        data = data.contiguous()
        self._check("swap_patches", data)
        out = torch.empty_like(data)
        device_packed = h2d(packed, data.device) if s_max else None
        origins_ptr = None if device_packed is None else C.c_void_p(device_packed.data_ptr())
        counts_ptr = None if device_packed is None else C.c_void_p(device_packed.data_ptr() + len(lists) * s_max * 6 * 4)
        self._call("swap_patches", data, _ptr(data), _ptr(out), data.element_size(), data.shape[0], data.shape[1], _i32x3(shape), _i32x3(patch),
                   origins_ptr, counts_ptr, len(lists), s_max, self._stream(data))
        return out

    def _batch_and_mask(self, data: Tensor, mask: Tensor | None, what: str) -> tuple[Tensor, Tensor | None]:
        if data.ndim != 5:
            raise ValueError(f"{what}: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        data = data.contiguous()
        if mask is not None:
            if mask.ndim != 4 or tuple(mask.shape[1:]) != tuple(data.shape[2:]) or mask.shape[0] not in (1, data.shape[1]):
                raise ValueError(f"{what}: a mask of shape {tuple(mask.shape)} does not broadcast over data of shape {tuple(data.shape)}")
            mask = mask.contiguous()
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)
        self._check(what, data, mask)
        return data, mask

    def intensity_multi_quantiles(self, data: Tensor, fractions: Sequence[float], mask: Tensor | None = None) -> tuple[Tensor, Tensor]:
        """``np.percentile(values, [100 * q for q in fractions])`` for every batch element of ``data`` ``(B, C, I, J, K)``,
        ``values`` being the element's voxels (all channels) inside ``mask`` as float32: ``(percentiles, counts)``, a float64
        ``(B, len(fractions))`` and an int64 ``(B,)`` tensor ON THE DEVICE — nothing is read back, nothing synchronises.

        ``mask``: ``(1 or C, I, J, K)`` on the device, any dtype, nonzero = inside, the same for every element.  Up to 32
        fractions.  A NaN inside an element, or nothing inside, makes its percentiles NaN.
        """
        fractions = [float(q) for q in fractions]
        if not 1 <= len(fractions) <= _abi.MULTI_QUANTILE_MAX_FRACTIONS:
            raise ValueError(f"intensity_multi_quantiles: 1 to {_abi.MULTI_QUANTILE_MAX_FRACTIONS} fractions, got {len(fractions)}")
        for q in fractions:
            if not 0 <= q <= 1:
                raise ValueError(f"Only values 0 <= q <= 1 are supported, but got {q!r}")
        data, mask = self._batch_and_mask(data, mask, "intensity_multi_quantiles")
        batch = data.shape[0]
        values = torch.empty((batch, len(fractions)), dtype=torch.float64, device=data.device)
        counts = torch.empty(batch, dtype=torch.int64, device=data.device)
        nbytes = int(self._fn["intensity_multi_quantiles_workspace_bytes"](batch, len(fractions)))
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=data.device)
        spatial = data.shape[2] * data.shape[3] * data.shape[4]
        self._call("intensity_multi_quantiles", data, _ptr(data), dtype_code(data.dtype), batch, data.shape[1], spatial, _ptr(mask),
                   0 if mask is None else dtype_code(mask.dtype), 0 if mask is None else mask.shape[0],
                   (C.c_double * len(fractions))(*fractions), len(fractions), _ptr(values), _ptr(counts), _ptr(workspace), nbytes,
                   self._stream(data))
        return values, counts

    def histogram_standardize(self, data: Tensor, landmarks: Tensor, quantiles: Sequence[float]) -> Tensor:
        """``_apply_histogram_standardization`` of the reference for every element of ``data`` ``(B, C, I, J, K)``: the
        element's percentiles at ``quantiles`` (``intensity_multi_quantiles``), the piecewise-linear map onto ``landmarks`` (a
        float32 tensor with one value per quantile), the result in ``data``'s dtype.  No read-back, no synchronisation.
        """
        if landmarks.ndim != 1 or landmarks.numel() != len(quantiles):
            raise ValueError(f"histogram_standardize: {landmarks.numel()} landmarks for {len(quantiles)} quantiles")
        if landmarks.numel() < 2:
            raise ValueError("histogram_standardize: at least 2 landmarks")
        percentiles, _ = self.intensity_multi_quantiles(data, quantiles)
        data = data.contiguous()
        landmarks = landmarks.to(torch.float32).contiguous()
        if landmarks.device != data.device:
            landmarks = h2d(landmarks, data.device)
        self._check("histogram_standardize", landmarks)
        batch = data.shape[0]
        out = torch.empty_like(data)
        table = torch.empty((max(batch, 1), 3, _abi.MULTI_QUANTILE_MAX_FRACTIONS), dtype=torch.float32, device=data.device)
        self._call("histogram_standardize", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, data.numel() // batch if batch else 0,
                   _ptr(percentiles), _ptr(landmarks), landmarks.numel(), _ptr(table), self._stream(data))
        return out

    # -- Ghosting and Spike (transforms/intensity/ghosting.py, spike.py) ---------------------------------------------------
    def _phase_tables(self, shape: Sequence[int], device) -> Tensor:
        """``(I + J + K, 2)`` float32 on *device*: per axis ``(cos, sin)(2 pi r / S)``, evaluated in float64 on the host and
        rounded once (built once per shape)."""
        cache = self.__dict__.setdefault("_phase_table_cache", {})
        key = (tuple(int(s) for s in shape), str(device))
        table = cache.get(key)
        if table is None:
            rows = []
            for size in key[0]:
                angle = 2.0 * np.pi * np.arange(size, dtype=np.float64) / max(size, 1)
                rows.append(np.stack([np.cos(angle), np.sin(angle)], axis=1))
            host = torch.from_numpy(np.concatenate(rows).astype(np.float32))
            if len(cache) >= 8:
                cache.clear()
            table = cache[key] = h2d(host, device)
        return table

    @staticmethod
    def _per_element(value, batch: int, what: str) -> list:
        """A scalar for the whole batch, or one entry per element."""
        if isinstance(value, (list, tuple)):
            if len(value) != batch:
                raise ValueError(f"{what}: {len(value)} entries for a batch of {batch}")
            return list(value)
        return [value] * batch

    @staticmethod
    def _per_element_lists(lists, batch: int, what: str, item_is_sequence: bool) -> list[list]:
        """One list of items for the whole batch, or one such list per element (an item: an integer, or a triple when
        ``item_is_sequence``).  An empty entry is an element's empty list."""
        lists = list(lists)

        def is_element_list(entry) -> bool:
            if not isinstance(entry, (list, tuple)):
                return False
            return not item_is_sequence or len(entry) == 0 or isinstance(entry[0], (list, tuple))

        if not any(is_element_list(entry) for entry in lists):
            return [lists] * batch
        if len(lists) != batch or not all(is_element_list(entry) for entry in lists):
            raise ValueError(f"{what}: {len(lists)} lists for a batch of {batch}")
        return [list(entry) for entry in lists]

    def ghost_lines(self, data: Tensor, axes, strengths, frequency_lists, active: Tensor | None = None) -> Tensor:
        """``_add_ghosting`` / ``_add_ghosting_per_element`` of the reference in image space: along ``axes[b]`` every line of
        element ``b`` loses ``strengths[b]`` of its components at the UNSHIFTED frequencies ``frequency_lists[b]`` (the
        k-space planes the reference scales by ``1 - strength``).  ``axes`` / ``strengths``: one value or one per element;
        ``frequency_lists``: one list of integers or one list per element.  ``data`` is ``(B, C, I, J, K)`` of any dtype; the
        result has its dtype.  Elements with ``active[b] == 0``, an empty list or zero strength are exact copies.

        One reduction and one update per line, no FFT, no complex volume; one packed upload carries every list.
        """
        if data.ndim != 5:
            raise ValueError(f"ghost_lines: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if _wants_grad(data):  # per line x - (strength / S) sum_f (c_f c_f^T + s_f s_f^T) x: a symmetric matrix, its own transpose
            result = self.ghost_lines(data.detach(), axes, strengths, frequency_lists, active)
            return _AttachBackward.apply(
                data, result, lambda grad: self.ghost_lines(grad.to(torch.float32), axes, strengths, frequency_lists, active).to(data.dtype))
        batch, shape = int(data.shape[0]), [int(s) for s in data.shape[2:]]
        axes = [int(a) for a in self._per_element(axes, batch, "ghost_lines: axes")]
        strengths = [float(s) for s in self._per_element(strengths, batch, "ghost_lines: strengths")]
        lists = self._per_element_lists(frequency_lists, batch, "ghost_lines: frequency_lists", False)
        for axis, frequencies in zip(axes, lists, strict=True):
            if axis not in (0, 1, 2):
                raise ValueError(f"ghost_lines: axis {axis} (0, 1 or 2)")
            if any(int(f) != f or not 0 <= f < max(shape[axis], 1) for f in frequencies):
                raise ValueError(f"ghost_lines: a frequency outside [0, {shape[axis]}) along axis {axis}")
        flags = self._flags(active, batch, "ghost_lines: active")
        data = data.contiguous()
        self._check("ghost_lines", data, flags)
        out = torch.empty_like(data)
        if data.numel() == 0:
            return out
        words = [0] * (4 * batch)
        for b, (axis, strength, frequencies) in enumerate(zip(axes, strengths, lists, strict=True)):
            words[4 * b : 4 * b + 4] = [axis, len(frequencies), len(words), int(np.float32(strength).view(np.int32))]
            words.extend(int(f) for f in frequencies)
        params = h2d(torch.tensor(words, dtype=torch.int32), data.device)
        mask = 0
        for axis in axes:
            mask |= 1 << axis
        tables = self._phase_tables(shape, data.device)
        self._call("kspace_ghost_lines", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, data.shape[1], _i32x3(shape), mask,
                   _ptr(params), len(words), max(len(f) for f in lists), _ptr(tables), _ptr(flags), self._stream(data))
        return out

    #: bytes of half spectrum (the rfftn result) that `spectrum_peak` holds at a time; one volume's always fits
    RFFTN_CHUNK_BYTES = 256 << 20

    def complex_abs_max(self, spectrum: Tensor, out: Tensor | None = None) -> Tensor:
        """``spectrum.abs().amax(1)`` of a contiguous complex64 ``(rows, n)`` device tensor: ``rows`` float32 maxima, each
        element read once (``tio_complex_abs_max``; finite input).  ``out``: a float32 ``(rows,)`` tensor to write into."""
        if spectrum.ndim != 2 or spectrum.dtype != torch.complex64:
            raise ValueError(f"complex_abs_max: expected a complex64 (rows, n) tensor, got {spectrum.dtype} {tuple(spectrum.shape)}")
        spectrum = spectrum.contiguous()
        self._check("complex_abs_max", spectrum, out)
        rows, n = spectrum.shape
        if out is None:
            out = torch.empty(rows, dtype=torch.float32, device=spectrum.device)
        elif out.dtype != torch.float32 or out.numel() != rows or not out.is_contiguous():
            raise ValueError(f"complex_abs_max: out must be {rows} contiguous float32 values")
        self._call("complex_abs_max", spectrum, _ptr(spectrum), rows, n, _ptr(out), self._stream(spectrum))
        return out

    def spectrum_peak(self, data: Tensor) -> Tensor:
        """``fftn(data.float()).abs().amax`` over the spatial axes of ``(B, C, I, J, K)`` data: ``(B * C,)`` float32 ON THE
        DEVICE.  The input is real, so the half spectrum of ``rfftn`` holds the same maximum; it is taken a few volumes at a
        time (at most ``RFFTN_CHUNK_BYTES`` of spectrum, one volume at least) and reduced by ``complex_abs_max`` in one read.
        The library FFT of this family lives here only.
        """
        if data.ndim != 5:
            raise ValueError(f"spectrum_peak: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        self._check("spectrum_peak", data)
        volumes = int(data.shape[0] * data.shape[1])
        peaks = torch.empty(volumes, dtype=torch.float32, device=data.device)
        if data.numel() == 0:
            return peaks.zero_()
        spatial = tuple(int(s) for s in data.shape[2:])
        flat = data.reshape(volumes, *spatial)
        per_volume = spatial[0] * spatial[1] * (spatial[2] // 2 + 1) * 8
        step = max(1, self.RFFTN_CHUNK_BYTES // per_volume)
        for start in range(0, volumes, step):
            spectrum = torch.fft.rfftn(flat[start : start + step].float(), dim=(-3, -2, -1))
            self.complex_abs_max(spectrum.reshape(spectrum.shape[0], -1), peaks[start : start + step])
        return peaks

    def add_spikes(self, data: Tensor, frequency_lists, intensities, peaks: Tensor, active: Tensor | None = None) -> Tensor:
        """``_add_spikes`` / ``_add_spikes_per_instance`` of the reference in image space: element ``b`` gains
        ``peaks[b, c] * intensities[b] / (I J K)`` times the sum of the plane waves at the UNSHIFTED frequency triples
        ``frequency_lists[b]`` (a triple listed twice counts twice).  ``frequency_lists``: one list of triples or one list per
        element; ``intensities``: one value or one per element; ``peaks``: the ``(B * C,)`` float32 device tensor of
        ``spectrum_peak`` — never read back.  Elements with ``active[b] == 0``, no triple or zero intensity are exact copies.
        """
        if data.ndim != 5:
            raise ValueError(f"add_spikes: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        batch, shape = int(data.shape[0]), [int(s) for s in data.shape[2:]]
        intensities = [float(s) for s in self._per_element(intensities, batch, "add_spikes: intensities")]
        lists = self._per_element_lists(frequency_lists, batch, "add_spikes: frequency_lists", True)
        for triples in lists:
            for triple in triples:
                if len(triple) != 3 or any(int(f) != f or not 0 <= f < max(s, 1) for f, s in zip(triple, shape, strict=True)):
                    raise ValueError(f"add_spikes: {tuple(triple)} is not a frequency triple inside {tuple(shape)}")
        if peaks.dtype != torch.float32 or peaks.numel() != batch * data.shape[1]:
            raise ValueError(f"add_spikes: peaks must hold {batch * data.shape[1]} float32 values, got {peaks.numel()} of {peaks.dtype}")
        flags = self._flags(active, batch, "add_spikes: active")
        data, peaks = data.contiguous(), peaks.contiguous()
        self._check("add_spikes", data, peaks, flags)
        out = torch.empty_like(data)
        if data.numel() == 0:
            return out
        words = [0] * (4 * batch)
        for b, (intensity, triples) in enumerate(zip(intensities, lists, strict=True)):
            words[4 * b : 4 * b + 4] = [len(triples), len(words), int(np.float32(intensity).view(np.int32)), 0]
            for triple in triples:
                words.extend(int(f) for f in triple)
        params = h2d(torch.tensor(words, dtype=torch.int32), data.device)
        tables = self._phase_tables(shape, data.device)
        self._call("kspace_add_spikes", data, _ptr(data), _ptr(out), dtype_code(data.dtype), batch, data.shape[1], _i32x3(shape), _ptr(params),
                   len(words), max(len(t) for t in lists), _ptr(tables), _ptr(peaks), _ptr(flags), self._stream(data))
        return out

    def kspace_segment_mix(self, segments: Sequence[Tensor], bounds: Sequence[int], out_dtype: torch.dtype,
                           active: Tensor | None = None) -> Tensor:
        """Motion's k-space composite (motion.py:334-372) of float32 ``(B, C, I, J, K)`` images.

        ``segments[0]`` is the still image, ``segments[s]`` the moved image whose spectrum fills
        the k-space planes ``[bounds[s], bounds[s + 1])`` along the first spatial axis.  Rows
        of inactive elements (``active[b] == 0``) are left unwritten.
        """
        first = segments[0]
        if first.ndim != 5:
            raise ValueError(f"expected (B, C, I, J, K) tensors, got {tuple(first.shape)}")
        if len(segments) > _abi.MAX_SEGMENTS:
            raise ValueError(f"at most {_abi.MAX_SEGMENTS - 1} motion transforms are supported, got {len(segments) - 1}")
        if len(bounds) != len(segments) + 1:
            raise ValueError("bounds must have one more entry than segments")
        if any(_wants_grad(s) for s in segments):
            return self._segment_mix_with_backward(list(segments), [int(v) for v in bounds], out_dtype, active)
        segments = [s.contiguous() for s in segments]
        for s in segments:
            if s.dtype != torch.float32 or s.shape != first.shape:
                raise ValueError("segments must be float32 tensors of one shape")
        self._check("kspace_segment_mix", *segments, active)
        length = int(first.shape[2])
        table = self._mix_table(length, tuple(int(v) for v in bounds), first.device)
        flags = None if active is None else active.to(torch.uint8).contiguous()
        out = torch.empty(first.shape, dtype=out_dtype, device=first.device)
        self._segment_mix_launch(segments, bounds, table, out, flags)
        return out

    def _segment_mix_launch(self, segments: Sequence[Tensor], bounds: Sequence[int], table: Tensor, out: Tensor, flags: Tensor | None) -> None:
        first = segments[0]
        pointers = (C.c_void_p * len(segments))(*[s.data_ptr() for s in segments])
        self._call("kspace_segment_mix", first, pointers, len(segments), (C.c_int32 * len(bounds))(*[int(v) for v in bounds]),
                   _ptr(table), _ptr(out), dtype_code(out.dtype), first.shape[0], first.shape[1], _i32x3(first.shape[2:]),
                   _ptr(flags), self._stream(first))

    def _segment_mix_with_backward(self, segments: list[Tensor], bounds: list[int], out_dtype: torch.dtype, active: Tensor | None) -> Tensor:
        """``kspace_segment_mix`` of segments that require gradients.  The launch evaluates ``out = x_0 + sum_{s >= 1} W[s]
        (x_s - x_0)`` and ``W[s][i'][i]`` depends on ``i - i'`` through a cosine only: every ``W[s]`` is symmetric, so
        ``dL/dx_s = W[s] g`` and ``dL/dx_0 = g - sum_{s >= 1} W[s] g`` are launches of the same kernel on the gradient — with the
        zero volume as the still image and ``W[s]`` as the only moved block, and with the gradient as the still image and the
        zero volume moved everywhere.  Rows of inactive elements receive zero (the launch skips them both ways)."""
        result = self.kspace_segment_mix([s.detach() for s in segments], bounds, out_dtype, active)
        length, device = int(result.shape[2]), result.device
        flags = None if active is None else active.to(torch.uint8).contiguous()

        def backward(grad, needs):
            grad = grad.to(torch.float32).contiguous()
            self._check("kspace_segment_mix (backward)", grad)
            table = self._mix_table(length, tuple(bounds), device)
            zero = torch.zeros_like(grad)
            grads: list[Tensor | None] = [None] * len(segments)
            for s, need in enumerate(needs):
                if not need:
                    continue
                # (rows of inactive elements are not written by the launch: they start, and stay, at zero)
                grads[s] = torch.zeros_like(grad) if flags is not None else torch.empty(grad.shape, dtype=torch.float32, device=grad.device)
                if s == 0:
                    self._segment_mix_launch([grad] + [zero] * (len(segments) - 1), bounds, table, grads[s], flags)
                else:  # the kernel reads block 1 of the table it is given: hand it the blocks s - 1 and s
                    self._segment_mix_launch([zero, grad], [0, 0, length], table[s - 1 : s + 1], grads[s], flags)
            return grads

        return _AttachBackwardMany.apply(backward, result, *segments)

    def _mix_table(self, length: int, bounds: tuple, device) -> Tensor:
        """The ``(n_segments, I, I)`` band-pass table of ``tio_kspace_segment_mix`` on *device* (built once per shape)."""
        cache = self.__dict__.setdefault("_mix_tables", {})
        key = (length, bounds, str(device))
        table = cache.get(key)
        if table is None:
            host = torch.empty(len(bounds) - 1, length, length, dtype=torch.float32)
            status = self._fn["kspace_mix_table"](length, len(bounds) - 1, (C.c_int32 * len(bounds))(*bounds), C.c_void_p(host.data_ptr()))
            if status != _abi.OK:
                message = (self._fn["last_error"]() or b"").decode(errors="replace") if "last_error" in self._fn else ""
                raise EngineError(f"tio_kspace_mix_table failed with status {status}: {message}")
            if len(cache) >= 8:
                cache.clear()
            table = cache[key] = h2d(host, device) if self.device_type == "cuda" else host
        return table

    # -- PCA (transforms/intensity/pca.py) ---------------------------------------------------------------------------------
    def _channel_matrix(self, data: Tensor, what: str) -> tuple[Tensor, int, int, int]:
        """``data`` as the contiguous float32 ``(B, C, voxels)`` tensor the two PCA kernels read, with its three sizes."""
        if data.ndim != 5:
            raise ValueError(f"{what}: expected a (B, C, I, J, K) tensor, got {tuple(data.shape)}")
        if data.dtype != torch.float32:
            raise TypeError(f"{what}: float32 data only (the reference's `.float()` is the caller's), got {data.dtype}")
        batch, channels = int(data.shape[0]), int(data.shape[1])
        voxels = int(data.shape[2]) * int(data.shape[3]) * int(data.shape[4])
        if not 1 <= channels <= _abi.PCA_MAX_CHANNELS or voxels < 1:
            raise ValueError(f"{what}: 1 to {_abi.PCA_MAX_CHANNELS} channels of at least one voxel, got {tuple(data.shape)}")
        if "channel_scatter" not in self._fn:
            raise EngineError(f"{what}: the {self.name} engine has no PCA kernels")
        return data.contiguous(), batch, channels, voxels

    def channel_scatter(self, data: Tensor) -> tuple[Tensor, Tensor]:
        """``(mean, scatter)`` of every batch element of a float32 ``(B, C, I, J, K)`` tensor over its voxels: the channel means
        ``(B, C)`` and ``sum_v (x_v - mean)(x_v - mean)^T`` ``(B, C, C)``, float64 ON THE DEVICE, from one read of the data
        (``tio_channel_scatter``).  Nothing is read back, nothing synchronises; two calls give the same bits."""
        data, batch, channels, voxels = self._channel_matrix(data, "channel_scatter")
        self._check("channel_scatter", data)
        mean = torch.empty((batch, channels), dtype=torch.float64, device=data.device)
        scatter = torch.empty((batch, channels, channels), dtype=torch.float64, device=data.device)
        if batch == 0:
            return mean, scatter
        nbytes = int(self._fn["channel_scatter_workspace_bytes"](batch, channels, voxels))
        if nbytes < 0:
            raise EngineError("channel_scatter: " + (self._fn["last_error"]() or b"").decode(errors="replace"))
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=data.device)
        self._call("channel_scatter", data, _ptr(data), batch, channels, voxels, _ptr(mean), _ptr(scatter), _ptr(workspace), nbytes,
                   self._stream(data))
        return mean, scatter

    def channel_project(self, data: Tensor, center: Tensor, weights: Tensor, offset: Tensor, *, clip: bool) -> Tensor:
        """``out[b, k] = sum_c weights[b, k, c] (data[b, c] - center[b, c]) + offset[b, k]`` per voxel, clamped to ``[0, 1]`` when
        ``clip`` (a NaN stays NaN): float32 ``(B, q, I, J, K)`` from float32 ``(B, C, I, J, K)`` data and float32 device tensors
        ``center (B, C)``, ``weights (B, q, C)``, ``offset (B, q)`` in one pass (``tio_channel_project``)."""
        data, batch, channels, voxels = self._channel_matrix(data, "channel_project")
        if weights.ndim != 3 or weights.shape[0] != batch or weights.shape[2] != channels or not 1 <= weights.shape[1] <= channels:
            raise ValueError(f"channel_project: weights of shape {tuple(weights.shape)} for data of shape {tuple(data.shape)} (B, 1 .. C, C)")
        components = int(weights.shape[1])
        if tuple(center.shape) != (batch, channels) or tuple(offset.shape) != (batch, components):
            raise ValueError(f"channel_project: center {tuple(center.shape)} and offset {tuple(offset.shape)} must be (B, C) and (B, q)")
        for name, tensor in (("center", center), ("weights", weights), ("offset", offset)):
            if tensor.dtype != torch.float32:
                raise TypeError(f"channel_project: {name} must be float32, got {tensor.dtype}")
        center, weights, offset = center.contiguous(), weights.contiguous(), offset.contiguous()
        self._check("channel_project", data, center, weights, offset)
        out = torch.empty((batch, components, *data.shape[2:]), dtype=torch.float32, device=data.device)
        if batch == 0:
            return out
        self._call("channel_project", data, _ptr(data), batch, channels, voxels, _ptr(center), _ptr(weights), _ptr(offset), components,
                   int(bool(clip)), _ptr(out), self._stream(data))
        return out

    # -- annotations (data/points.py, data/bboxes.py) -------------------------------------------------------------------------
    def warp_points(self, points: Tensor, offsets, blocks: Tensor, control_points: Tensor | None = None, *,
                    return_status: bool = False):
        """The points of a whole batch through ``s^-1`` of each element's resampling, in ONE launch (``tio_points_warp``).

        ``points``: float32 ``(N, 3)`` on the device, input voxel coordinates (IJK), the elements' points one after the other;
        ``offsets``: ``B + 1`` host integers, element ``b`` owns ``points[offsets[b]:offsets[b + 1]]`` (an empty element costs
        nothing); ``blocks``: float64 ``(B, 40)``, one parameter block per element as ``include/tio_hip.h`` lays it out
        (``transforms/_annotations.py: parameter_block``); ``control_points``: the float32 buffer the blocks' offsets point
        into, or ``None`` when no element has a field.  Host ``blocks`` / ``control_points`` are uploaded with one staging copy.
        Returns float32 ``(N, 3)`` output voxel coordinates, with ``return_status`` also the int8 ``(N,)`` solver status
        (0 converged).  Nothing is read back and nothing synchronises.
        """
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"warp_points: expected (N, 3) points, got {tuple(points.shape)}")
        if points.dtype != torch.float32:
            raise TypeError(f"warp_points: float32 points only, got {points.dtype}")
        if "points_warp" not in self._fn:
            raise EngineError(f"warp_points: the {self.name} engine has no tio_points_warp")
        self._check("warp_points", points)
        host_offsets = torch.as_tensor(offsets, device="cpu").to(torch.int32).contiguous().reshape(-1)
        batch, total = host_offsets.numel() - 1, int(points.shape[0])
        if batch < 0 or blocks.dtype != torch.float64 or tuple(blocks.shape) != (batch, _abi.POINTS_BLOCK_DOUBLES):
            raise ValueError(
                f"warp_points: {host_offsets.numel()} offsets need float64 blocks of shape ({batch}, {_abi.POINTS_BLOCK_DOUBLES}),"
                f" got {blocks.dtype} {tuple(blocks.shape)}"
            )
        if control_points is not None and control_points.dtype != torch.float32:
            raise TypeError(f"warp_points: float32 control points only, got {control_points.dtype}")
        points = points.contiguous()
        out = torch.empty((total, 3), dtype=torch.float32, device=points.device)
        status = torch.empty((total,), dtype=torch.int8, device=points.device) if return_status else None
        if batch > 0 and total > 0:
            # one staging copy for whatever is still on the host; h2d_packed moves float32 words, so the int32 offsets and the
            # float64 blocks travel as their own bits
            field = None if control_points is None else control_points.contiguous().reshape(-1)
            staged = [host_offsets.view(torch.float32), blocks.contiguous().reshape(-1), field]
            if blocks.device.type == "cpu":
                staged[1] = staged[1].view(torch.float32)
            offsets_dev, blocks_dev, field = h2d_packed(staged, points.device)
            self._check("warp_points", offsets_dev, blocks_dev, field)
            self._call(
                "points_warp", points, _ptr(points), _ptr(out), _ptr(status), total, _ptr(host_offsets), _ptr(offsets_dev), batch,
                _ptr(blocks_dev), _ptr(field), 0 if field is None else field.numel(), self._stream(points),
            )
        return (out, status) if return_status else out

    # -- feeding side -------------------------------------------------------
    def patch_accumulate(
        self,
        out: Tensor,
        weight_sum: Tensor | None,
        patches: Tensor,
        placements: Sequence[tuple[Sequence[int], Sequence[int], Sequence[int]]],
        mode: str,
        windows: Sequence[Tensor] | None = None,
    ) -> None:
        """Add ``patches`` ``(N, C, pi, pj, pk)`` into the ``(C, I, J, K)`` accumulators IN PLACE, in patch order.

        ``placements[n] = (dst_ini, src_ini, extent)``; ``mode`` is ``"crop"`` (element copy),
        ``"average"`` or ``"hann"`` (then ``windows`` = three float32 1-D windows on the device).
        """
        if patches.ndim != 5 or out.ndim != 4 or patches.shape[1] != out.shape[0]:
            raise ValueError(f"expected patches (N, C, i, j, k) and out (C, I, J, K), got {tuple(patches.shape)} / {tuple(out.shape)}")
        if patches.dtype != out.dtype or (weight_sum is not None and weight_sum.dtype != out.dtype):
            raise TypeError("patches and accumulators must share one dtype")
        if not out.is_contiguous() or (weight_sum is not None and not weight_sum.is_contiguous()):
            raise ValueError("accumulators must be contiguous")
        if len(placements) != patches.shape[0]:
            raise ValueError("one placement per patch")
        code = {"crop": _abi.OVERLAP_CROP, "average": _abi.OVERLAP_AVERAGE, "hann": _abi.OVERLAP_HANN}[mode]
        if code != _abi.OVERLAP_CROP and out.dtype not in FLOAT_DTYPES:
            raise TypeError(f"overlap_mode {mode!r} needs floating-point patches, got {out.dtype}")
        patches = patches.contiguous()
        window_tensors = [None, None, None]
        if code == _abi.OVERLAP_HANN:
            window_tensors = [w.to(device=out.device, dtype=torch.float32).contiguous() for w in windows]
        self._check("patch_accumulate", out, weight_sum, patches, *window_tensors)
        for start in range(0, patches.shape[0], _abi.MAX_PATCHES):
            chunk = patches[start : start + _abi.MAX_PATCHES]
            table = (_abi.PatchPlacement * chunk.shape[0])()
            for slot, (dst_ini, src_ini, extent) in enumerate(placements[start : start + chunk.shape[0]]):
                table[slot].dst_ini = _i32x3(dst_ini)
                table[slot].src_ini = _i32x3(src_ini)
                table[slot].extent = _i32x3(extent)
            self._call(
                "patch_accumulate", out, _ptr(out), _ptr(weight_sum), dtype_code(out.dtype), out.shape[0],
                _i32x3(out.shape[1:]), _ptr(chunk), chunk.shape[0], _i32x3(chunk.shape[2:]), table, code,
                _ptr(window_tensors[0]), _ptr(window_tensors[1]), _ptr(window_tensors[2]), self._stream(out),
            )


    def centre_draw(self, source: Tensor, patch_size: Sequence[int], num_draws: int, *, label_table: Sequence[tuple[float, float]] | None = None,
                    seed: int = 0, uniforms: Tensor | None = None, return_uniforms: bool = False) -> "CentreDraw":
        """``num_draws`` patch centres drawn with replacement from the border-masked law of ``source`` ``(I, J, K)``
        (``tio_centre_law_sums`` + ``tio_centre_draw``: three launches, nothing read back, nothing synchronises).

        ``label_table is None``: ``source`` holds the weights, any engine dtype, each voxel converted to float32.  Otherwise
        ``source`` holds labels and the table at most 64 ``(label value, weight)`` pairs, later pairs overriding earlier ones;
        an empty table means ``weight = label > 0``.  ``uniforms``: float64 ``(num_draws,)`` in ``[0, 1)`` on the device, or
        ``None`` for the package's Philox stream under ``seed``.  The result's ``corners`` and ``record`` are views of one int32
        tensor ``packed``, so one ``packed.cpu()`` brings both to the host.
        """
        if source.ndim != 3:
            raise ValueError(f"centre_draw: expected an (I, J, K) weight source, got {tuple(source.shape)}")
        patch = [int(p) for p in patch_size]
        if len(patch) != 3 or any(p < 1 for p in patch):
            raise ValueError(f"centre_draw: patch_size must be three positive integers, got {tuple(patch_size)}")
        num_draws = int(num_draws)
        if num_draws < 0:
            raise ValueError("centre_draw: a negative number of draws")
        if source.numel() == 0 and num_draws:
            raise ValueError("centre_draw: draws from an empty volume")
        pairs = [] if label_table is None else [(float(value), float(weight)) for value, weight in label_table]
        if len(pairs) > _abi.CENTRE_MAX_LABELS:
            raise ValueError(f"centre_draw: a label table of {len(pairs)} entries (at most {_abi.CENTRE_MAX_LABELS})")
        values = (C.c_double * max(len(pairs), 1))(*[value for value, _ in pairs])
        weights = (C.c_float * max(len(pairs), 1))(*[weight for _, weight in pairs])
        source = source.contiguous()
        if uniforms is not None:
            if uniforms.dtype != torch.float64 or tuple(uniforms.shape) != (num_draws,):
                raise ValueError(f"centre_draw: uniforms must be float64 of shape ({num_draws},), got {uniforms.dtype} {tuple(uniforms.shape)}")
            uniforms = uniforms.contiguous()
        self._check("centre_draw", source, uniforms)
        device = source.device
        segments = (source.numel() + _abi.CENTRE_SEGMENT - 1) // _abi.CENTRE_SEGMENT
        prefix = torch.empty((segments,), dtype=torch.float64, device=device)
        corner_words = (3 * num_draws + 3) // 4 * 4  # (the record starts on a 16-byte boundary)
        packed = torch.empty((corner_words + _abi.CENTRE_RECORD_BYTES // 4,), dtype=torch.int32, device=device)
        centres = torch.empty((num_draws,), dtype=torch.int64, device=device)
        used = torch.empty((num_draws,), dtype=torch.float64, device=device) if return_uniforms else None
        corners, record = packed[: 3 * num_draws].view(num_draws, 3), packed[corner_words:]
        law = (_ptr(source), dtype_code(source.dtype), int(label_table is not None), values, weights, len(pairs), _i32x3(source.shape), _i32x3(patch))
        self._call("centre_law_sums", source, *law, _ptr(prefix), _ptr(record), self._stream(source))
        if num_draws:
            self._call("centre_draw", source, *law, _ptr(prefix), _ptr(record), num_draws, int(seed) & (2**64 - 1), _ptr(uniforms), _ptr(used),
                       _ptr(centres), _ptr(corners), self._stream(source))
        return CentreDraw(centres, corners, record, packed, used, prefix)

    def patch_gather(self, data: Tensor, corners: Tensor, patch_size: Sequence[int]) -> Tensor:
        """``torch.stack([data[:, i:i + pi, j:j + pj, k:k + pk] for (i, j, k) in corners])`` in ONE launch (``tio_patch_gather``).

        ``data``: ``(C, I, J, K)`` of any dtype (moved by element width); ``corners``: int32 ``(N, 3)``, on the device as a
        draw leaves them or on the host (one small staged upload); a corner outside ``[0, shape - patch]`` is clamped by the
        kernel.  Returns ``(N, C, pi, pj, pk)``.
        """
        if data.ndim != 4:
            raise ValueError(f"patch_gather: expected a (C, I, J, K) tensor, got {tuple(data.shape)}")
        patch = [int(p) for p in patch_size]
        shape = [int(s) for s in data.shape[1:]]
        if len(patch) != 3 or any(p < 1 for p in patch):
            raise ValueError(f"patch_gather: patch_size must be three positive integers, got {tuple(patch_size)}")
        if any(p > s for p, s in zip(patch, shape, strict=True)):
            raise ValueError(f"Patch size {tuple(patch)} cannot be larger than spatial shape {tuple(shape)}")
        if corners.ndim != 2 or corners.shape[1] != 3 or corners.dtype != torch.int32:
            raise ValueError(f"patch_gather: corners must be int32 of shape (N, 3), got {corners.dtype} {tuple(corners.shape)}")
        data = data.contiguous()
        corners = h2d(corners, data.device).contiguous()
        self._check("patch_gather", data, corners)
        out = torch.empty((corners.shape[0], data.shape[0], *patch), dtype=data.dtype, device=data.device)
        self._call("patch_gather", data, _ptr(data), _ptr(out), data.element_size(), data.shape[0], _i32x3(shape), _i32x3(patch), _ptr(corners),
                   corners.shape[0], self._stream(data))
        return out

    def nifti_decode(self, raw: Tensor, *, disk_type: int, shape: Sequence[int], channels: int = 1, batch: int = 1, swap_bytes: bool = False,
                     slope: float | None = None, inter: float = 0.0, out_dtype: torch.dtype | None = None) -> Tensor:
        """The payloads of ``batch`` NIfTI-1 files, as bytes on the device, to one ``(batch, channels, I, J, K)`` tensor in
        ONE launch (``tio_nifti_decode``): byte swap, Fortran-to-C reorder, promotion or scaling and conversion.

        ``raw``: uint8, ``batch * channels`` dense volumes of ``I * J * K`` elements of ``disk_type`` (a NIfTI datatype
        code) back to back, 16-byte aligned.  ``slope``: ``None`` for an unscaled read, else ``float64(x) * slope + inter``
        with two roundings.  ``out_dtype``: the natural dtype (default; float64 when scaled), or float32 / float64 reached
        in one rounding.
        """
        from .data.nifti import DATATYPES  # noqa: PLC0415

        if disk_type not in DATATYPES:
            raise ValueError(f"nifti_decode: datatype {disk_type} is not supported (supported: {sorted(DATATYPES)})")
        shape = [int(s) for s in shape]
        if len(shape) != 3 or min(shape) < 1 or channels < 1 or batch < 1:
            raise ValueError(f"nifti_decode: shape {tuple(shape)}, channels {channels} and batch {batch} must be positive")
        scaled = slope is not None
        natural = torch.float64 if scaled else DATATYPES[disk_type][2]
        out_dtype = natural if out_dtype is None else out_dtype
        needed = batch * channels * shape[0] * shape[1] * shape[2] * DATATYPES[disk_type][1]
        if raw.dtype != torch.uint8 or raw.ndim != 1 or not raw.is_contiguous() or raw.numel() < needed:
            raise ValueError(f"nifti_decode: raw must be a contiguous 1-D uint8 tensor of at least {needed} bytes, got {raw.dtype} {tuple(raw.shape)}")
        self._check("nifti_decode", raw)
        layout = _abi.NiftiLayout(disk_type=int(disk_type), swap_bytes=int(bool(swap_bytes)), shape=_i32x3(shape), channels=int(channels),
                                  scaled=int(scaled), slope=float(slope) if scaled else 1.0, inter=float(inter) if scaled else 0.0)
        out = torch.empty((batch, channels, *shape), dtype=out_dtype, device=raw.device)
        self._call("nifti_decode", raw, _ptr(raw), _ptr(out), dtype_code(out_dtype), batch, C.byref(layout), self._stream(raw))
        return out


class CentreDraw(NamedTuple):
    """What :meth:`Engine.centre_draw` leaves on the device."""

    centres: Tensor  # int64 (N,): flat index of each centre, -1 where the law holds no positive weight
    corners: Tensor  # int32 (N, 3): min(max(centre - patch // 2, 0), shape - patch); a view of `packed`
    record: Tensor  # int32 (4,): the float64 total (two words) and the invalid flag; a view of `packed`
    packed: Tensor  # corners, padding to 16 bytes, record: ONE copy brings both to the host
    uniforms: Tensor | None  # float64 (N,): the uniforms used, when asked for
    prefix: Tensor  # float64 (segments,): inclusive prefix sums of the segment totals

    def on_host(self) -> tuple[Tensor, float, bool]:
        """``(corners, total, invalid)`` on the host: the one device-to-host copy (and synchronisation) of a draw."""
        host = self.packed.cpu()
        record = host[host.numel() - _abi.CENTRE_RECORD_BYTES // 4 :]
        return host[: self.corners.numel()].view(-1, 3), float(record[:2].view(torch.float64).item()), bool(record[2].item())


_ENGINE: Engine | None = None
_HIP_ENGINE: Engine | None = None


def hip_engine() -> Engine:
    """The engine over ``libtio_hip.so`` whatever `engine()` currently hands out (the tests swap that one for the CPU oracle):
    for callers that are bound to the HIP library themselves — the ``torch.ops.tio_hip`` custom ops' backward passes."""
    global _HIP_ENGINE
    if _HIP_ENGINE is None:
        _, functions = _lib.load()
        _HIP_ENGINE = Engine(functions, "cuda", "hip")
    return _HIP_ENGINE


def engine() -> Engine:
    """The HIP engine (loads ``libtio_hip.so`` on first use; raises if unavailable)."""
    global _ENGINE
    if _ENGINE is None:
        _, functions = _lib.load()
        _ENGINE = Engine(functions, "cuda", "hip")
    return _ENGINE
