"""``torchio_amd._abi`` is derived from ``include/tio_hip.h``: layouts against the C compiler, prototypes against hand-written
expectations, and the reader's refusal of anything outside the header's grammar.  No GPU."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import pytest

from torchio_amd import _abi
from torchio_amd import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# tag -> (class, the C field names in order), spelled out here so that a field the reader dropped cannot hide
STRUCTS = {
    "tio_resample_geom": (
        _abi.ResampleGeom,
        "batch in_shape out_shape affine_first mapping_dev mapping_batched control_points_dev cp_batched cp_shape cp_skip_dev "
        "passthrough_dev in_spacing out_spacing norm_shape precision plan_dev plan_bytes flags",
    ),
    "tio_resample_image": (_abi.ResampleImage, "in out channels dtype interp fill_dev labels_dev n_labels pad_label out_min_dev"),
    "tio_patch_placement": (_abi.PatchPlacement, "dst_ini src_ini extent"),
    "tio_conv_pass": (
        _abi.ConvPass,
        "axis family radius radius_class radius_k pre_bias post_noise fma grid segments rows_per_segment k_tiles lds_bytes last",
    ),
    "tio_nifti_layout": (_abi.NiftiLayout, "disk_type swap_bytes shape channels scaled slope inter"),
    "tio_centre_record": (_abi.CentreRecord, "total invalid reserved"),
}


def test_struct_layouts_agree_with_the_c_compiler(tmp_path):
    compiler = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if compiler is None:
        pytest.skip("no host C compiler (cc, gcc, clang) on PATH")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "tio_hip.h"', "int main(void) {"]
    for tag, (_, names) in STRUCTS.items():
        lines.append(f'  printf("{tag} %zu\\n", sizeof({tag}));')
        for name in names.split():
            lines.append(f'  printf("{tag}.{name} %zu %zu\\n", offsetof({tag}, {name}), sizeof((({tag}*)0)->{name}));')
    lines += ['  printf("tio_host_mt_state %zu\\n", sizeof(tio_host_mt_state));', "  return 0;", "}"]
    source = tmp_path / "layout.c"
    source.write_text("\n".join(lines) + "\n")
    subprocess.run([compiler, "-std=c99", "-I", INCLUDE, str(source), "-o", str(tmp_path / "layout")], check=True)
    printed = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {key: tuple(int(v) for v in values) for key, *values in (line.split() for line in printed.splitlines())}

    ours = {"tio_host_mt_state": (_abi.HOST_MT_STATE_BYTES,)}
    for tag, (cls, names) in STRUCTS.items():
        assert [name for name, _ in cls._fields_] == [name + "_" * (name == "in") for name in names.split()], tag
        ours[tag] = (C.sizeof(cls),)
        for name, _ in cls._fields_:
            field = getattr(cls, name)
            ours[f"{tag}.{name.rstrip('_')}"] = (field.offset, field.size)
    assert ours == compiled
    assert _abi.CENTRE_RECORD_BYTES == compiled["tio_centre_record"][0] == 16


def test_prototypes_match_hand_written_expectations():
    vp, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
    i32s = C.POINTER(C.c_int32)
    expected = {
        "resample3d": (C.c_int, [C.POINTER(_abi.ResampleGeom), i32, C.POINTER(_abi.ResampleImage), vp]),
        "resample3d_plan_bytes": (i64, [C.POINTER(_abi.ResampleGeom)]),
        "add_noise": (C.c_int, [vp, vp, i32, i32, i64, f32, f32, vp, vp, i32, i32, vp, vp, u64, vp, vp]),
        "blur_fused": (
            C.c_int,
            [vp, vp, vp, i32, i32, i32, i32s, vp, i32, i32, i32s, vp, i32s, i32, f32, f32, vp, vp, i32, u64, vp, i32, vp],
        ),
        "separable_conv3d_passes": (C.c_int, [i32, i32, i32, i32s, i32s, i32, i32, i32, i32, i32, C.POINTER(_abi.ConvPass)]),
        "pad3d": (C.c_int, [vp, vp, i32, i32, i32, i32s, i32s, i32, f64, vp, vp]),
        "kspace_segment_mix": (C.c_int, [vp, i32, vp, vp, vp, i32, i32, i32, i32s, vp, vp]),
        "host_mt19937_plan_prefix": (C.c_int, [vp, i64, vp, i64, vp, vp, vp]),
        "points_warp": (C.c_int, [vp, vp, vp, i64, vp, vp, i32, vp, vp, i64, vp]),
        "channel_scatter_plan": (C.c_int, [i32, i32, i64, i32s]),
        # record_dev points to a tio_centre_record in DEVICE memory: an address, not a POINTER(CentreRecord)
        "centre_law_sums": (C.c_int, [vp, i32, i32, vp, vp, i32, i32s, i32s, vp, vp, vp]),
        "nifti_decode": (C.c_int, [vp, vp, i32, i32, C.POINTER(_abi.NiftiLayout), vp]),
        "intensity_stats_workspace_bytes": (i64, []),
        "last_error": (C.c_char_p, []),
        "reload_env": (None, []),
    }
    table = {**_abi.PROTOTYPES, **_abi.HIP_ONLY_PROTOTYPES}
    for name, prototype in expected.items():
        assert table[name] == prototype, name
    assert not set(_abi.PROTOTYPES) & set(_abi.HIP_ONLY_PROTOTYPES)
    assert tuple(_abi.PROTOTYPES) == _abi.ORACLE_ENTRY_POINTS


def test_constants_come_from_the_header():
    constants = _header.load().constants
    assert constants["TIO_ERR_UNSUPPORTED_CONFIG"] == _abi.UNSUPPORTED_CONFIG == -5
    assert constants["TIO_I64"] == _abi.I64 == 8
    assert constants["TIO_POINTS_TOLERANCE"] == _abi.POINTS_TOLERANCE == 1e-7
    assert _abi.OK == 0 and _abi.ABI_VERSION == constants["TIO_ABI_VERSION"]
    assert "TIO_HIP_H" not in constants and "TIO_BSPLINE_ORDER" not in constants  # the include guard, the function-like macro
    for name, value in constants.items():
        assert getattr(_abi, name.removeprefix("TIO_")) == value


FIELD = "typedef struct tio_patch_placement {"  # a line added after this one is a field
ANYWHERE = "int tio_abi_version(void);"


@pytest.mark.parametrize(
    ("after", "added"),
    [
        (ANYWHERE, "int tio_bad(const void* x, long n, void* stream);"),
        (ANYWHERE, "int tio_bad(unsigned n);"),
        (ANYWHERE, "int tio_bad(unsigned int n);"),
        (ANYWHERE, "int tio_bad(const void* x, void (*done)(int32_t), void* stream);"),
        (FIELD, "int32_t bits : 3;"),
        (ANYWHERE, "int tio_bad(size_t n);"),
        (ANYWHERE, "int tio_bad(tio_dtype dtype);"),
        (ANYWHERE, "long tio_bad(void);"),
        (ANYWHERE, "int tio_bad(int32_t n)"),  # half a prototype: no semicolon
        (ANYWHERE, "int tio_bad();"),
        (ANYWHERE, "int tio_bad(int32_t grid[3][3]);"),
        (ANYWHERE, "int tio_bad(tio_patch_placement by_value);"),
        (ANYWHERE, "int tio_abi_version(void);"),  # declared twice
        ("typedef struct tio_nifti_layout {", "tio_patch_placement inner;"),  # a nested struct
        (ANYWHERE, "typedef struct tio_outer { struct { int32_t x; } inner; } tio_outer;"),
        (ANYWHERE, "typedef enum tio_bad_enum { TIO_BAD_A, TIO_BAD_B } tio_bad_enum;"),
        (ANYWHERE, "typedef int32_t tio_index;"),
        (ANYWHERE, "#define TIO_BAD (1 << 3)"),
        (ANYWHERE, "#define TIO_MAX_IMAGES 9"),
        (ANYWHERE, "#if 0"),
    ],
)
def test_the_reader_refuses_what_it_does_not_know(after, added):
    with open(_header.HEADER_PATH, encoding="utf-8") as file:
        lines = file.read().split("\n")
    at = lines.index(after) + 1
    lines.insert(at, added)
    with pytest.raises(_header.HeaderError) as caught:
        _abi_tables("\n".join(lines))
    assert added in str(caught.value)


def _abi_tables(text):
    header = _header.Header(text)
    return header.prototypes({tag: header.struct_class(tag, cls.__name__) for tag, (cls, _) in STRUCTS.items()})


def test_the_unchanged_text_is_accepted_and_a_missing_header_is_an_import_error(tmp_path):
    with open(_header.HEADER_PATH, encoding="utf-8") as file:
        assert len(_abi_tables(file.read())) == len(_abi.HIP_SYMBOLS)
    with pytest.raises(ImportError, match="no_such_header.h"):
        _header.load(str(tmp_path / "no_such_header.h"))
