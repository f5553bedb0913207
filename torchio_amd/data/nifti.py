"""NIfTI-1 single files (``.nii`` / ``.nii.gz``): header, affine, payload, writer.  No third-party reader is involved.

The layout is the published NIfTI-1 one (``nifti1.h``): a 348-byte header, the magic ``n+1\\0``, the voxels from
``vox_offset`` on with the first axis fastest.  Two rules here are restated from memory of nibabel's behaviour and are
UNVERIFIED against it (nibabel cannot be installed where this was written):

* the affine of a file with neither ``sform_code`` nor ``qform_code`` set (:func:`header_affine`, the last branch) is
  meant to be nibabel's ``get_best_affine`` fallback;
* the values (:func:`decode_host`) are meant to be what ``np.asarray(img.dataobj)`` yields: scaling applies iff
  ``scl_slope`` is finite, non-zero and ``(slope, inter) != (1, 0)``, as ``float64(x) * float64(slope)``, rounded, then
  ``+ float64(inter)``, rounded.

What is written down here is the contract of this package either way.

The payload is decoded on the device by ``tio_nifti_decode`` (``csrc/nifti_codec.hip``, :func:`decode_device`) or on the
host with numpy (:func:`decode_host`: what ``DataLoader`` workers and boxes without a GPU use).
"""
from __future__ import annotations

import gzip
import math
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

HEADER_BYTES = 348
MAGIC = b"n+1\0"

#: NIfTI datatype code -> (numpy type character, bytes, the torch dtype an unscaled read yields)
DATATYPES = {
    2: ("u1", 1, torch.uint8),
    4: ("i2", 2, torch.int16),
    8: ("i4", 4, torch.int32),
    16: ("f4", 4, torch.float32),
    64: ("f8", 8, torch.float64),
    256: ("i1", 1, torch.int8),
    512: ("u2", 2, torch.int32),    # torch has no uint16 ...
    768: ("u4", 4, torch.int64),    # ... uint32 ...
    1024: ("i8", 8, torch.int64),
    1280: ("u8", 8, torch.int64),   # ... or uint64: two's-complement wrap, as ndarray.astype
}
#: torch dtype -> (datatype code written, numpy dtype written)
_WRITE_TYPES = {
    torch.float32: (16, "<f4"), torch.float64: (64, "<f8"), torch.float16: (16, "<f4"), torch.bfloat16: (16, "<f4"),
    torch.uint8: (2, "u1"), torch.int8: (256, "i1"), torch.int16: (4, "<i2"), torch.int32: (8, "<i4"), torch.int64: (1024, "<i8"),
}
SUFFIXES = (".nii", ".nii.gz")


def is_nifti_path(path) -> bool:
    return str(path).lower().endswith(SUFFIXES)


def _is_gz(path) -> bool:
    return str(path).lower().endswith(".gz")


def _inflate(path, limit: int | None = None) -> bytes:
    """The inflated bytes of a ``.nii.gz``: all of them, or no more than the first *limit*."""
    if limit is None:
        with gzip.open(path, "rb") as stream:
            return stream.read()
    inflater = zlib.decompressobj(wbits=31)
    out = b""
    with open(path, "rb") as stream:
        while len(out) < limit and not inflater.eof:
            chunk = stream.read(4096)
            if not chunk:
                break
            out += inflater.decompress(chunk, limit - len(out))
    return out


def _new_staging(nbytes: int, pinned: bool) -> Tensor:
    """The host buffer a payload (or the box of one) is gathered in before it is decoded: pinned when it feeds an H2D copy."""
    return torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=bool(pinned))


@dataclass(frozen=True)
class NiftiHeader:
    """What the reader needs of a NIfTI-1 header."""

    path: str
    big_endian: bool
    datatype: int
    shape: tuple[int, int, int]
    channels: int
    vox_offset: int
    slope: float
    inter: float
    affine: np.ndarray  # float64 (4, 4)

    @property
    def scaled(self) -> bool:
        slope = self.slope
        return math.isfinite(slope) and slope != 0.0 and (slope, self.inter) != (1.0, 0.0)

    @property
    def element_bytes(self) -> int:
        return DATATYPES[self.datatype][1]

    @property
    def disk_dtype(self) -> np.dtype:
        return np.dtype((">" if self.big_endian else "<") + DATATYPES[self.datatype][0])

    @property
    def natural_dtype(self) -> torch.dtype:
        return torch.float64 if self.scaled else DATATYPES[self.datatype][2]

    @property
    def voxels(self) -> int:
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def payload_bytes(self) -> int:
        return self.channels * self.voxels * self.element_bytes

    def group_key(self) -> tuple:
        """Files with equal keys decode in one ``tio_nifti_decode`` launch."""
        scaling = (self.slope, self.inter) if self.scaled else None
        return (self.shape, self.channels, self.datatype, self.big_endian, scaling)


def header_affine(fields: dict) -> np.ndarray:
    """The voxel-to-world matrix of a parsed header: the sform rows, else the qform quaternion, else (UNVERIFIED against
    nibabel, see the module docstring) ``diag(-pixdim1, pixdim2, pixdim3)`` with the volume centre at the world origin."""
    pixdim = [float(v) for v in fields["pixdim"]]
    affine = np.eye(4, dtype=np.float64)
    if fields["sform_code"] > 0:
        affine[:3, :] = np.asarray(fields["srow"], dtype=np.float64).reshape(3, 4)
        return affine
    if fields["qform_code"] > 0:
        b, c, d = (float(v) for v in fields["quatern"])
        a = math.sqrt(max(0.0, 1.0 - b * b - c * c - d * d))
        rotation = np.array([
            [a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
            [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
            [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c],
        ], dtype=np.float64)
        qfac = -1.0 if pixdim[0] == -1.0 else 1.0
        affine[:3, :3] = rotation * np.array([pixdim[1], pixdim[2], pixdim[3] * qfac], dtype=np.float64)
        affine[:3, 3] = [float(v) for v in fields["qoffset"]]
        return affine
    zooms = np.array([-pixdim[1], pixdim[2], pixdim[3]], dtype=np.float64)
    affine[:3, :3] = np.diag(zooms)
    affine[:3, 3] = -zooms * (np.asarray(fields["dim"][1:4], dtype=np.float64) - 1.0) / 2.0
    return affine


def parse_header(raw: bytes, path="<bytes>") -> NiftiHeader:
    """The first 348 bytes of a file as a :class:`NiftiHeader`; ``ValueError`` naming the cause for anything this reader refuses."""
    if len(raw) < HEADER_BYTES:
        raise ValueError(f"{path}: {len(raw)} bytes are too few for a NIfTI-1 header ({HEADER_BYTES})")
    dim0 = struct.unpack_from("<h", raw, 40)[0]
    order = "<" if 1 <= dim0 <= 7 else ">"
    sizeof_hdr = struct.unpack_from(order + "i", raw, 0)[0]
    if sizeof_hdr != HEADER_BYTES:
        raise ValueError(f"{path}: sizeof_hdr is {sizeof_hdr}, not {HEADER_BYTES}: not a NIfTI-1 file (NIfTI-2 and other formats are not read)")
    magic = bytes(raw[344:348])
    if magic != MAGIC:
        raise ValueError(f"{path}: magic {magic!r} is not {MAGIC!r}: only single-file NIfTI-1 is read (no .hdr/.img pairs, no NIfTI-2)")
    dim = struct.unpack_from(order + "8h", raw, 40)
    datatype = struct.unpack_from(order + "h", raw, 70)[0]
    if datatype not in DATATYPES:
        raise ValueError(f"{path}: datatype {datatype} is not supported (supported: {sorted(DATATYPES)}; no complex, RGB or binary data)")
    fields = {
        "dim": dim,
        "pixdim": struct.unpack_from(order + "8f", raw, 76),
        "qform_code": struct.unpack_from(order + "h", raw, 252)[0],
        "sform_code": struct.unpack_from(order + "h", raw, 254)[0],
        "quatern": struct.unpack_from(order + "3f", raw, 256),
        "qoffset": struct.unpack_from(order + "3f", raw, 268),
        "srow": struct.unpack_from(order + "12f", raw, 280),
    }
    ndim = dim[0]
    if ndim == 3:
        channels = 1
    elif ndim == 4:
        channels = dim[4]
    elif ndim == 5 and dim[4] == 1:
        channels = dim[5]
    else:
        raise ValueError(f"{path}: expected 3D, 4D (I, J, K, C) or 5D (I, J, K, 1, C) data, got dim = {tuple(dim[: ndim + 1])}")
    shape = (int(dim[1]), int(dim[2]), int(dim[3]))
    if min(shape) < 1 or channels < 1:
        raise ValueError(f"{path}: every extent must be at least 1, got dim = {tuple(dim[: ndim + 1])}")
    vox_offset, slope, inter = struct.unpack_from(order + "3f", raw, 108)
    return NiftiHeader(
        path=str(path), big_endian=order == ">", datatype=int(datatype), shape=shape, channels=int(channels),
        vox_offset=max(int(vox_offset), HEADER_BYTES), slope=float(slope), inter=float(inter), affine=header_affine(fields),
    )


def read_header(path) -> NiftiHeader:
    """Parse the header of *path*, reading (and, for ``.nii.gz``, inflating) no more than its 348 bytes."""
    path = os.fspath(path)
    if not is_nifti_path(path):
        raise ValueError(f"{path}: only .nii and .nii.gz files are read here")
    if _is_gz(path):
        raw = _inflate(path, HEADER_BYTES)
    else:
        with open(path, "rb") as stream:
            raw = stream.read(HEADER_BYTES)
    return parse_header(raw, path)


# -- payload ---------------------------------------------------------------------------------------------------------------
def _disk_array(header: NiftiHeader) -> np.ndarray:
    """The whole payload as a read-only ``(C, K, J, I)`` array of the disk type: a memory map of a ``.nii``, the inflated
    buffer of a ``.nii.gz``."""
    shape = (header.channels, *reversed(header.shape))
    if _is_gz(header.path):
        raw = _inflate(header.path)
        if len(raw) < header.vox_offset + header.payload_bytes:
            raise ValueError(f"{header.path}: {len(raw)} bytes, the header promises {header.vox_offset + header.payload_bytes}")
        return np.frombuffer(raw, dtype=header.disk_dtype, count=header.channels * header.voxels, offset=header.vox_offset).reshape(shape)
    if os.path.getsize(header.path) < header.vox_offset + header.payload_bytes:
        raise ValueError(f"{header.path}: {os.path.getsize(header.path)} bytes, the header promises {header.vox_offset + header.payload_bytes}")
    return np.memmap(header.path, dtype=header.disk_dtype, mode="r", offset=header.vox_offset, shape=shape)


def _full_box(header: NiftiHeader) -> tuple:
    return ((0, header.channels), (0, header.shape[0]), (0, header.shape[1]), (0, header.shape[2]))


def stage_payload(header: NiftiHeader, staging: Tensor, box=None) -> None:
    """Copy the disk elements of *box* (``((c0, c1), (i0, i1), (j0, j1), (k0, k1))``; default: everything) into the uint8
    host tensor *staging*, dense and in disk order.  Only the box is read from a ``.nii``."""
    (c0, c1), (i0, i1), (j0, j1), (k0, k1) = box or _full_box(header)
    extent = (c1 - c0, k1 - k0, j1 - j0, i1 - i0)
    target = staging.numpy().view(header.disk_dtype).reshape(extent)
    if box is None and not _is_gz(header.path):  # a whole .nii: read straight into the staging buffer
        with open(header.path, "rb") as stream:
            stream.seek(header.vox_offset)
            if stream.readinto(memoryview(staging.numpy())) != header.payload_bytes:
                raise ValueError(f"{header.path}: shorter than the {header.vox_offset + header.payload_bytes} bytes its header promises")
        return
    np.copyto(target, _disk_array(header)[c0:c1, k0:k1, j0:j1, i0:i1])


def _box_layout(header: NiftiHeader, box):
    (c0, c1), (i0, i1), (j0, j1), (k0, k1) = box or _full_box(header)
    return c1 - c0, (i1 - i0, j1 - j0, k1 - k0)


def decode_host(header: NiftiHeader, staging: Tensor, box=None, dtype: torch.dtype | None = None) -> Tensor:
    """The plain numpy decode of staged disk elements: ``(C, I, J, K)`` in the natural dtype (float64 when scaled).  As on
    the device, float32 / float64 are reached in ONE rounding from the exact disk value (a uint64 beyond 2^63 as the unsigned
    number it is) or from the float64 scaled value; any other *dtype* is a cast of the natural result."""
    channels, shape = _box_layout(header, box)
    disk = staging.numpy().view(header.disk_dtype).reshape((channels, *reversed(shape)))
    values = np.ascontiguousarray(disk.transpose(0, 3, 2, 1))
    direct = {torch.float32: np.float32, torch.float64: np.float64}.get(dtype)
    if header.scaled:
        values = values.astype(np.float64) * np.float64(header.slope) + np.float64(header.inter)  # two ufuncs: two roundings
        if direct is not None:
            values = values.astype(direct)
    elif direct is not None:
        values = values.astype(direct)
    else:
        kind = DATATYPES[header.datatype][0]
        values = values.astype(np.dtype({"u2": "i4", "u4": "i8", "u8": "i8"}.get(kind, kind)))
    out = torch.from_numpy(values)
    return out if dtype is None or out.dtype == dtype else out.to(dtype)


def _out_dtype(natural: torch.dtype, dtype: torch.dtype | None) -> torch.dtype:
    """The dtype the decode itself produces: float32 / float64 come out of the kernel in one rounding, others are a cast
    after the natural decode."""
    return dtype if dtype in (torch.float32, torch.float64) else natural


def decode_device(headers, staging: Tensor, device, dtype: torch.dtype | None = None, box=None) -> Tensor:
    """One H2D copy of the staged payloads of *headers* (one group: equal ``group_key``) and ONE ``tio_nifti_decode``:
    the stacked ``(B, C, I, J, K)`` tensor on *device*."""
    from .. import ops  # noqa: PLC0415

    header = headers[0]
    channels, shape = _box_layout(header, box)
    raw = staging.to(device, non_blocking=True)
    out = ops.engine().nifti_decode(
        raw, disk_type=header.datatype, swap_bytes=header.big_endian, shape=shape, channels=channels, batch=len(headers),
        slope=header.slope if header.scaled else None, inter=header.inter, out_dtype=_out_dtype(header.natural_dtype, dtype),
    )
    return out if dtype is None or out.dtype == dtype else out.to(dtype)


def read_tensor(header: NiftiHeader, device=None, dtype: torch.dtype | None = None, box=None) -> Tensor:
    """``(C, I, J, K)`` voxels of one file (or of *box*) on *device* (default: the host)."""
    device = torch.device("cpu" if device is None else device)
    channels, shape = _box_layout(header, box)
    staging = _new_staging(channels * shape[0] * shape[1] * shape[2] * header.element_bytes, device.type == "cuda")
    stage_payload(header, staging, box)
    if device.type == "cuda":
        return decode_device([header], staging, device, dtype, box)[0]
    return decode_host(header, staging, box, dtype).to(device)


def read_stacked(headers, device, dtype: torch.dtype | None = None) -> Tensor:
    """``(B, C, I, J, K)`` voxels of a homogeneous group of files on a cuda *device*: the payloads gathered in ONE pinned
    buffer, one H2D copy, one decode launch writing the stacked tensor."""
    header = headers[0]
    if any(h.group_key() != header.group_key() for h in headers):
        raise ValueError("read_stacked: the files differ in shape, channels, disk type, endianness or scaling")
    size = header.payload_bytes
    staging = _new_staging(size * len(headers), True)
    for index, item in enumerate(headers):
        stage_payload(item, staging[index * size : (index + 1) * size])
    return decode_device(headers, staging, torch.device(device), dtype)


# -- writer ----------------------------------------------------------------------------------------------------------------
def affine_to_quaternion(affine) -> tuple[tuple[float, float, float], float, tuple[float, float, float]]:
    """``((b, c, d), qfac, zooms)`` of the rotation part of *affine* after removing the zooms (``nifti_mat44_to_quatern``):
    the nearest rotation (polar decomposition) when the columns are sheared; ``qfac = -1`` carries a negative determinant."""
    block = np.asarray(affine, dtype=np.float64)[:3, :3].copy()
    zooms = np.sqrt(np.sum(block * block, axis=0))
    zooms[zooms == 0] = 1.0
    block /= zooms
    left, _, right = np.linalg.svd(block)
    rotation = left @ right
    qfac = 1.0
    if np.linalg.det(rotation) < 0:
        rotation[:, 2] *= -1.0
        qfac = -1.0
    (r11, r12, r13), (r21, r22, r23), (r31, r32, r33) = rotation
    a = r11 + r22 + r33 + 1.0
    if a > 0.5:
        a = 0.5 * math.sqrt(a)
        b, c, d = 0.25 * (r32 - r23) / a, 0.25 * (r13 - r31) / a, 0.25 * (r21 - r12) / a
    else:
        xd, yd, zd = 1.0 + r11 - (r22 + r33), 1.0 + r22 - (r11 + r33), 1.0 + r33 - (r11 + r22)
        if xd > 1.0:
            b = 0.5 * math.sqrt(xd)
            c, d, a = 0.25 * (r12 + r21) / b, 0.25 * (r13 + r31) / b, 0.25 * (r32 - r23) / b
        elif yd > 1.0:
            c = 0.5 * math.sqrt(yd)
            b, d, a = 0.25 * (r12 + r21) / c, 0.25 * (r23 + r32) / c, 0.25 * (r13 - r31) / c
        else:
            d = 0.5 * math.sqrt(zd)
            b, c, a = 0.25 * (r13 + r31) / d, 0.25 * (r23 + r32) / d, 0.25 * (r21 - r12) / d
        if a < 0.0:
            b, c, d = -b, -c, -d
    return (float(b), float(c), float(d)), qfac, (float(zooms[0]), float(zooms[1]), float(zooms[2]))


def build_header(shape, channels: int, datatype: int, affine) -> bytes:
    """A little-endian single-file NIfTI-1 header (348 bytes) as :func:`write_nifti` writes it."""
    affine = np.asarray(affine, dtype=np.float64)
    if max(*shape, channels) > 32767:
        raise ValueError(f"NIfTI-1 stores extents as int16: {tuple(shape)} x {channels} channels does not fit")
    quatern, qfac, zooms = affine_to_quaternion(affine)
    raw = bytearray(HEADER_BYTES)
    dim = [3, *shape, 1, 1, 1, 1] if channels == 1 else [5, *shape, 1, channels, 1, 1]
    pixdim = [qfac, *zooms, 1.0, 1.0, 1.0, 1.0]
    struct.pack_into("<i", raw, 0, HEADER_BYTES)
    struct.pack_into("<8h", raw, 40, *dim)
    struct.pack_into("<h", raw, 68, 0 if channels == 1 else 1007)  # NIFTI_INTENT_VECTOR
    struct.pack_into("<h", raw, 70, datatype)
    struct.pack_into("<h", raw, 72, 8 * DATATYPES[datatype][1])
    struct.pack_into("<8f", raw, 76, *pixdim)
    struct.pack_into("<3f", raw, 108, 352.0, 1.0, 0.0)  # vox_offset, scl_slope, scl_inter
    struct.pack_into("<B", raw, 123, 2)  # xyzt_units: mm
    struct.pack_into("<2h", raw, 252, 2, 2)  # qform_code, sform_code: aligned
    struct.pack_into("<3f", raw, 256, *quatern)
    struct.pack_into("<3f", raw, 268, *affine[:3, 3])
    struct.pack_into("<12f", raw, 280, *affine[:3, :].reshape(-1))
    raw[344:348] = MAGIC
    return bytes(raw)


def _disk_order(tensor: Tensor) -> np.ndarray:
    """``(C, I, J, K)`` voxels as a host ``(C, K, J, I)`` array (the file's order).  Device tensors are reversed by
    ``tio_permute3d`` and come over in one D2H copy into pinned memory."""
    if tensor.device.type == "cuda":
        from .. import ops  # noqa: PLC0415

        reversed_axes = ops.engine().permute3d(tensor.detach()[None], (2, 1, 0))[0]
        host = torch.empty(reversed_axes.shape, dtype=reversed_axes.dtype, pin_memory=True)
        host.copy_(reversed_axes)
        return host.numpy()
    return np.ascontiguousarray(tensor.detach().numpy().transpose(0, 3, 2, 1))


def write_nifti(path, tensor, affine=None, *, compresslevel: int = 1) -> None:
    """Write ``(C, I, J, K)`` (or ``(I, J, K)``) voxels as a little-endian single-file NIfTI-1: one channel 3-D, more as 5-D
    ``(I, J, K, 1, C)`` with ``intent_code`` 1007.  float16 / bfloat16 are written as float32, bool raises ``TypeError``."""
    path = os.fspath(path)
    if not is_nifti_path(path):
        raise ValueError(f"{path}: only .nii and .nii.gz can be written here")
    if isinstance(tensor, np.ndarray):
        tensor = torch.as_tensor(tensor)
    if tensor.ndim == 3:
        tensor = tensor[None]
    if tensor.ndim != 4:
        raise ValueError(f"write_nifti: expected (C, I, J, K) or (I, J, K) voxels, got {tuple(tensor.shape)}")
    if tensor.dtype not in _WRITE_TYPES:
        raise TypeError(f"write_nifti: dtype {tensor.dtype} cannot be written (the nine engine dtypes can; cast bool to uint8 first)")
    datatype, disk = _WRITE_TYPES[tensor.dtype]
    if tensor.dtype in (torch.float16, torch.bfloat16):
        tensor = tensor.to(torch.float32)
    if hasattr(affine, "data") and isinstance(affine.data, Tensor):  # AffineMatrix
        affine = affine.data.cpu().numpy()
    elif isinstance(affine, Tensor):
        affine = affine.cpu().numpy()
    affine = np.eye(4) if affine is None else affine
    header = build_header(tuple(int(s) for s in tensor.shape[1:]), int(tensor.shape[0]), datatype, affine)
    payload = _disk_order(tensor).astype(np.dtype(disk), copy=False)
    opener = (lambda: gzip.open(path, "wb", compresslevel=compresslevel)) if _is_gz(path) else (lambda: open(path, "wb"))
    with opener() as stream:
        stream.write(header)
        stream.write(b"\0\0\0\0")  # no extensions; the voxels start at byte 352
        stream.write(memoryview(payload).cast("B"))


__all__ = [
    "NiftiHeader", "affine_to_quaternion", "build_header", "decode_device", "decode_host", "header_affine", "is_nifti_path", "parse_header",
    "read_header", "read_stacked", "read_tensor", "stage_payload", "write_nifti",
]
