"""Shared code of the NIfTI tests: files built by hand and an independent restatement of the value rules.

Files are built with ``struct.pack`` at the field offsets of the published NIfTI-1 header and ``ndarray.tobytes(order="F")``;
the library's writer is never used here.  ``expected_tensor`` restates what a read must yield with numpy alone:
``frombuffer`` with an explicit byte order -> ``reshape(order="F")`` -> channel move -> promotion, or the two-step float64
scaling.  Inputs are seeded integers over the full range of each type (with the extremes, and for the 64-bit types values
near 2^53 and 2^63 where a double rounding through float64 differs from one rounding to float32), and floats including +-0,
denormals, +-inf and NaN.

A plain module (no test collected from it), imported by ``test_nifti_host.py`` and ``test_gpu_nifti.py``.
"""
from __future__ import annotations

import gzip
import struct

import numpy as np
import torch

#: NIfTI datatype code -> numpy type character
DISK_TYPES = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2", 768: "u4", 1024: "i8", 1280: "u8"}
#: what an unscaled read yields (torch has no uint16 / uint32 / uint64)
PROMOTED = {"u1": "u1", "i1": "i1", "i2": "i2", "i4": "i4", "i8": "i8", "f4": "f4", "f8": "f8", "u2": "i4", "u4": "i8", "u8": "i8"}
#: a scaling whose product and sum both round for most inputs (neither factor is a power of two)
SLOPE, INTER = 0.3, -7.1
#: as the float32 header fields hold them
SLOPE32, INTER32 = float(np.float32(SLOPE)), float(np.float32(INTER))

SHEAR_AFFINE = np.array([[2.0, 0.25, 0.0, -10.0], [0.0, 1.5, 0.5, 20.0], [0.125, 0.0, 3.0, -30.0], [0.0, 0.0, 0.0, 1.0]])

# values where float32(float64(x)) != float32(x): x = 2^53 + 2^29 + 1 lies just above the midpoint of two float32 neighbours
# (spacing 2^30 at 2^53); float64 (spacing 2 there) rounds it down ONTO the midpoint, which then ties to even (down), while the
# single rounding goes up.  The same 1-above-a-midpoint construction near 2^62 (float32 spacing 2^39, float64 spacing 2^10)
# and, for uint64, near 2^63 (float32 spacing 2^40, float64 spacing 2^11).
DOUBLE_ROUNDING_I64 = [2**53 + 2**29 + 1, -(2**53 + 2**29 + 1), 2**62 + 2**38 + 1, -(2**62 + 2**38 + 1), 2**53 + 1, 2**63 - 1, -(2**63)]
DOUBLE_ROUNDING_U64 = [2**53 + 2**29 + 1, 2**63 + 2**39 + 1, 2**63 + 1, 2**63, 2**64 - 1, 2**53 + 1]


def values(code: int, count: int, seed: int = 0) -> np.ndarray:
    """*count* native-endian values of disk type *code*: the special values first, seeded draws over the full range after."""
    kind = DISK_TYPES[code]
    rng = np.random.default_rng(1000 * seed + code)
    dtype = np.dtype(kind)
    if kind[0] == "f":
        tiny = np.finfo(dtype).tiny
        special = np.array([0.0, -0.0, tiny / 4, -tiny / 8, np.inf, -np.inf, np.nan, np.finfo(dtype).max, np.finfo(dtype).min, 1.0, -2.5, 1e-3],
                           dtype=dtype)
        # every exponent, not only those of a uniform draw: random bit patterns, NaN patterns replaced by finite draws
        bits = rng.integers(0, 2 ** (8 * dtype.itemsize), size=count, dtype=np.uint64, endpoint=False).astype(f"u{dtype.itemsize}")
        drawn = bits.view(dtype).copy()
        drawn[np.isnan(drawn)] = rng.normal(size=int(np.isnan(drawn).sum())).astype(dtype)
    else:
        info = np.iinfo(dtype)
        extra = {"i8": DOUBLE_ROUNDING_I64, "u8": DOUBLE_ROUNDING_U64}.get(kind, [])
        special = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1, *extra], dtype=dtype)
        drawn = rng.integers(info.min, info.max, size=count, dtype=dtype, endpoint=True)
    out = drawn
    out[: min(count, special.size)] = special[:count]
    return out


def volume(code: int, shape, channels: int = 1, seed: int = 0) -> np.ndarray:
    """Native-endian ``(I, J, K)`` (one channel) or ``(I, J, K, C)`` values of disk type *code*."""
    full = (*shape, channels) if channels > 1 else tuple(shape)
    flat = values(code, int(np.prod(full)), seed)
    # the special values lead the flat array: spread them over the volume, deterministically
    order = np.random.default_rng(seed + 7).permutation(flat.size)
    return flat[order].reshape(full)


def header_bytes(*, dim, datatype: int, big_endian: bool = False, pixdim=(1.0,) * 8, vox_offset: float = 352.0, slope: float = 0.0,
                 inter: float = 0.0, qform_code: int = 0, sform_code: int = 0, quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0),
                 srow=(0.0,) * 12, magic: bytes = b"n+1\0", sizeof_hdr: int = 348, intent_code: int = 0) -> bytes:
    """348 header bytes with the fields at the published offsets; everything else zero."""
    order = ">" if big_endian else "<"
    raw = bytearray(348)
    dims = list(dim) + [1] * (8 - len(dim))
    struct.pack_into(order + "i", raw, 0, sizeof_hdr)
    struct.pack_into(order + "8h", raw, 40, *dims)
    struct.pack_into(order + "h", raw, 68, intent_code)
    struct.pack_into(order + "h", raw, 70, datatype)
    struct.pack_into(order + "h", raw, 72, 8 * np.dtype(DISK_TYPES.get(datatype, "u1")).itemsize)
    struct.pack_into(order + "8f", raw, 76, *pixdim)
    struct.pack_into(order + "f", raw, 108, vox_offset)
    struct.pack_into(order + "f", raw, 112, slope)
    struct.pack_into(order + "f", raw, 116, inter)
    struct.pack_into("B", raw, 123, 2)
    struct.pack_into(order + "h", raw, 252, qform_code)
    struct.pack_into(order + "h", raw, 254, sform_code)
    struct.pack_into(order + "3f", raw, 256, *quatern)
    struct.pack_into(order + "3f", raw, 268, *qoffset)
    struct.pack_into(order + "12f", raw, 280, *srow)
    raw[344:348] = magic
    return bytes(raw)


def payload_bytes(array: np.ndarray, big_endian: bool) -> bytes:
    """The array as it lies on disk: first axis fastest, in the byte order asked for."""
    return array.astype(array.dtype.newbyteorder(">" if big_endian else "<")).tobytes(order="F")


def file_bytes(array: np.ndarray, datatype: int, *, big_endian: bool = False, scaled: bool = False, five_d: bool = False, **header) -> bytes:
    """A whole single-file NIfTI-1: header, four zero bytes, payload.  *array*: ``(I, J, K)`` or ``(I, J, K, C)``; *five_d*
    writes the latter as ``(I, J, K, 1, C)``."""
    if array.ndim == 3:
        dim = [3, *array.shape]
    elif five_d:
        dim = [5, *array.shape[:3], 1, array.shape[3]]
    else:
        dim = [4, *array.shape]
    if scaled:
        header = {"slope": SLOPE, "inter": INTER, **header}
    if "srow" not in header and "qform_code" not in header and "sform_code" not in header:
        header = {"sform_code": 1, "srow": tuple(SHEAR_AFFINE[:3].reshape(-1)), **header}
    return header_bytes(dim=dim, datatype=datatype, big_endian=big_endian, **header) + b"\0\0\0\0" + payload_bytes(array, big_endian)


def write_file(path, content: bytes) -> None:
    """*content* as ``.nii``, or gzipped when the name ends in ``.gz``."""
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as stream:
            stream.write(content)
    else:
        with open(path, "wb") as stream:
            stream.write(content)


def expected_array(payload: bytes, datatype: int, shape, channels: int, *, big_endian: bool, scaling=None, out: str | None = None) -> np.ndarray:
    """What reading *payload* must yield, ``(C, I, J, K)``: the rules of the format restated with numpy alone.  *out*
    (``"f4"`` / ``"f8"``): ONE ``astype`` from the exact disk value (a uint64 beyond 2^63 is converted as the unsigned number it
    is, not as the int64 it wraps to) or from the float64 scaled value."""
    kind = DISK_TYPES[datatype]
    disk = np.frombuffer(payload, dtype=np.dtype((">" if big_endian else "<") + kind))
    disk = disk.reshape((*shape, channels), order="F")
    disk = np.moveaxis(disk, -1, 0)
    if scaling is None:
        return np.ascontiguousarray(disk.astype(np.dtype(PROMOTED[kind] if out is None else out)))
    slope, inter = scaling
    product = disk.astype(np.float64) * np.float64(slope)  # rounded once ...
    value = product + np.float64(inter)  # ... and once more
    return np.ascontiguousarray(value if out is None else value.astype(np.dtype(out)))


def expected_tensor(payload: bytes, datatype: int, shape, channels: int = 1, *, big_endian: bool = False, scaled: bool = False,
                    out: str | None = None) -> torch.Tensor:
    """``expected_array`` as a tensor; *out* (``"f4"`` / ``"f8"``): converted with ONE ``astype`` from the exact value."""
    return torch.from_numpy(expected_array(payload, datatype, shape, channels, big_endian=big_endian, scaling=(SLOPE32, INTER32) if scaled else None, out=out))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal dtype, shape and BITS (NaN payloads and the sign of zero count)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        as_int = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
        return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
    return torch.equal(a, b)


def raw_reparse(content: bytes) -> dict:
    """The fields of a written file read back with ``struct`` alone (little-endian), and the voxels as ``(C, I, J, K)``."""
    dim = struct.unpack_from("<8h", content, 40)
    datatype = struct.unpack_from("<h", content, 70)[0]
    fields = {
        "sizeof_hdr": struct.unpack_from("<i", content, 0)[0], "dim": dim, "intent_code": struct.unpack_from("<h", content, 68)[0],
        "datatype": datatype, "bitpix": struct.unpack_from("<h", content, 72)[0], "pixdim": struct.unpack_from("<8f", content, 76),
        "vox_offset": struct.unpack_from("<f", content, 108)[0], "slope": struct.unpack_from("<f", content, 112)[0],
        "inter": struct.unpack_from("<f", content, 116)[0], "xyzt_units": content[123], "qform_code": struct.unpack_from("<h", content, 252)[0],
        "sform_code": struct.unpack_from("<h", content, 254)[0], "quatern": struct.unpack_from("<3f", content, 256),
        "qoffset": struct.unpack_from("<3f", content, 268), "srow": np.array(struct.unpack_from("<12f", content, 280)).reshape(3, 4),
        "magic": content[344:348], "extension": content[348:352],
    }
    channels = 1 if dim[0] == 3 else dim[5]
    fields["channels"] = channels
    fields["voxels"] = expected_array(content[352:], datatype, dim[1:4], channels, big_endian=False)
    fields["payload_size"] = len(content) - 352
    return fields


def quaternion_rotation(b: float, c: float, d: float) -> np.ndarray:
    """The rotation matrix of a unit quaternion (a, b, c, d) with a >= 0, written out (nifti1.h, "METHOD 2")."""
    a = np.sqrt(max(0.0, 1.0 - b * b - c * c - d * d))
    return np.array([
        [a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
        [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
        [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b],
    ])
