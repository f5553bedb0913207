"""ctypes description of the C ABI, derived from ``include/tio_hip.h`` at import (``_header`` reads it and states the rules).

Only types and prototypes live here — no library is loaded.  ``bind(lib, prefix)``
attaches ``argtypes``/``restype`` to every entry point of a loaded library whose
symbols start with ``prefix`` (``"tio_"`` for ``libtio_hip.so``).

Nothing below restates the header.  A new entry point is declared there and nowhere else; its name is added to
``ORACLE_ENTRY_POINTS`` if the CPU oracle restates it.
"""
from __future__ import annotations

import ctypes as C

from . import _header

_HEADER = _header.load()

# Every enum member and valued #define of the header, under its name without the TIO_ prefix: ABI_VERSION, MAX_IMAGES, OK
# and the ERR_* codes, the dtype / interp / PAD_ / REMAP_ / MAP_ / PRECISION_ / OVERLAP_ / CONV_ codes, GEOM_*, MAX_PATCHES,
# MAX_SEGMENTS, REMAP_MAX_PAIRS, KEEP_LARGEST_MAX_LABELS, CENTRE_*, POINTS_*, PCA_MAX_CHANNELS, HOST_MT_STATE_BYTES.
globals().update({name.removeprefix("TIO_"): value for name, value in _HEADER.constants.items()})
OK = _HEADER.constants["TIO_OK"]
UNSUPPORTED_CONFIG = _HEADER.constants["TIO_ERR_UNSUPPORTED_CONFIG"]  # fused form not available for these arguments; nothing was launched
MULTI_QUANTILE_MAX_FRACTIONS = 32  # not in the header, which states the limit in tio_intensity_multi_quantiles' comment only

# The structs the host fills in and passes by pointer: a parameter that points to one is typed POINTER(class).
_HOST_STRUCTS = {
    "tio_resample_geom": "ResampleGeom",
    "tio_resample_image": "ResampleImage",
    "tio_patch_placement": "PatchPlacement",
    "tio_conv_pass": "ConvPass",
    "tio_nifti_layout": "NiftiLayout",
}
_CLASSES = {tag: _HEADER.struct_class(tag, name) for tag, name in _HOST_STRUCTS.items()}
globals().update({cls.__name__: cls for cls in _CLASSES.values()})
# tio_centre_record lives in device memory: callers pass its address, so its parameters stay c_void_p; the class gives its size
# and layout.  tio_host_mt_state stays opaque: HOST_MT_STATE_BYTES bytes.
CentreRecord = _HEADER.struct_class("tio_centre_record", "CentreRecord")
CENTRE_RECORD_BYTES = C.sizeof(CentreRecord)

#: the entry points oracle/tio_oracle.c restates (as tio_oracle_*); every other one only the HIP library has
ORACLE_ENTRY_POINTS = (
    "resample3d", "channel_min", "separable_conv3d", "separable_conv3d_adjoint", "bias_field_apply", "add_noise", "philox_normal",
    "gamma_pow", "patch_accumulate", "bspline_prefilter", "interpolate3d", "axis_gather_lerp", "flip3d", "pad3d", "unique_labels",
    "kspace_segment_mix", "kspace_mix_table", "abi_version",
)  # fmt: skip

_ALL = _HEADER.prototypes(_CLASSES)
#: name -> (restype, argtypes); names are given without the library prefix.
PROTOTYPES = {name: _ALL[name] for name in ORACLE_ENTRY_POINTS}
#: entry points only the HIP library has (not the CPU restatement)
HIP_ONLY_PROTOTYPES = {name: prototype for name, prototype in _ALL.items() if name not in PROTOTYPES}

#: every symbol include/tio_hip.h declares for libtio_hip.so
HIP_SYMBOLS = tuple("tio_" + n for n in (*PROTOTYPES, *HIP_ONLY_PROTOTYPES))


def bind(lib: C.CDLL, prefix: str, extra: dict | None = None) -> dict:
    """Attach prototypes to ``lib`` and return ``{short_name: function}``.

    Raises ``AttributeError`` naming the first missing symbol.
    """
    table = {}
    protos = dict(PROTOTYPES)
    if extra:
        protos.update(extra)
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, prefix + name)
        fn.restype = restype
        fn.argtypes = argtypes
        table[name] = fn
    return table
