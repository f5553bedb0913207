"""Registers and spills of the marching stencil kernels, read from the built library's gfx950 code objects (no GPU).

``conv_march_kernel<R, FUSE_K, PRE_BIAS, POST_NOISE, FMA>`` is built two ways (``torchio_amd/csrc/Makefile``): the fused J + K
instantiations without the SLP vectoriser, the others with it.  What the speed of the fused J + K pass rests on is written in
the code object's metadata, and a later edit that quietly brings the spills back shows here:

* every ``FUSE_K`` instantiation: no spilled scalar or vector register and no private segment, and for ``R <= 6`` at most 128
  vector registers — what its ``__launch_bounds__(256, 4)`` promises;
* every ``PRE_BIAS`` instantiation: no spill, and not more vector registers than before the families were split
  (``PRE_BIAS_VGPRS``: read off the library built from the commit before the split, with the same toolchain).
"""
from __future__ import annotations

import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from torchio_amd import _lib

LLVM_BIN = os.environ.get("TIO_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MARCH = re.compile(r"conv_march_kernelILi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])E")  # <R, FUSE_K, PRE_BIAS, POST_NOISE, FMA>

#: vgpr_count of conv_march_kernel<R, false, true, 0, FMA> before the split: R -> (FMA = false, FMA = true)
PRE_BIAS_VGPRS = {1: (76, 70), 2: (98, 98), 3: (130, 130), 4: (164, 164), 5: (192, 192), 6: (220, 220), 7: (248, 248), 8: (270, 270)}


def _code_object_kernels(path: str) -> dict:
    """``{mangled kernel name: {metadata key: value}}`` of every gfx950 code object bundled in *path*."""
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(path, os.path.join(tmp, "in.bin"))
        subprocess.run([objdump, "--offloading", "in.bin"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for code_object in sorted(glob.glob(os.path.join(tmp, "in.bin.*gfx950*"))):
            notes = subprocess.run([readelf, "--notes", code_object], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:  # one block per kernel: .agpr_count is its first key
                fields = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
                kernels[fields["name"]] = fields
    return kernels


@pytest.fixture(scope="module")
def march_kernels() -> dict:
    """``{(R, FUSE_K, PRE_BIAS, POST_NOISE, FMA): metadata}`` of the library's conv_march_kernel instantiations."""
    for tool in ("llvm-objdump", "llvm-readelf"):
        if not os.path.isfile(os.path.join(LLVM_BIN, tool)):
            pytest.skip(f"{tool} not found under {LLVM_BIN}")
    if not os.path.isfile(_lib.LIBRARY_PATH):
        pytest.skip(f"{_lib.LIBRARY_PATH} is not built")
    found = {}
    for name, fields in _code_object_kernels(_lib.LIBRARY_PATH).items():
        match = MARCH.search(name)
        if match:
            r, fuse_k, pre_bias, post_noise, fma = (int(g) for g in match.groups())
            key = (r, bool(fuse_k), bool(pre_bias), post_noise, bool(fma))
            assert key not in found, f"conv_march_kernel{key} is in the library twice"
            found[key] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return found


def _describe(key, m) -> str:
    return (f"conv_march_kernel<{key[0]}, {str(key[1]).lower()}, {str(key[2]).lower()}, {key[3]}, {str(key[4]).lower()}>: "
            f"{m['vgpr_count']} VGPRs ({m['vgpr_spill_count']} spilled), {m['sgpr_count']} SGPRs ({m['sgpr_spill_count']} spilled), "
            f"{m['private_segment_fixed_size']} B private")


def test_the_library_holds_every_instantiation_the_launcher_names(march_kernels):
    """R = 1 .. 8 and both FMA values of: fused J + K with noise 0 / 1 / 2, bias on load, plain — and nothing else."""
    families = [(True, False, 0), (True, False, 1), (True, False, 2), (False, True, 0), (False, False, 0)]
    expected = {(r, fk, pb, pn, fma) for r in range(1, 9) for fk, pb, pn in families for fma in (False, True)}
    assert set(march_kernels) == expected


def test_fused_k_instantiations_spill_nothing(march_kernels):
    fused = {key: m for key, m in march_kernels.items() if key[1]}
    assert len(fused) == 8 * 3 * 2
    bad = []
    for key, m in sorted(fused.items()):
        print(_describe(key, m))
        if m["sgpr_spill_count"] != 0 or m["vgpr_spill_count"] != 0 or m["private_segment_fixed_size"] != 0:
            bad.append(_describe(key, m))
        elif key[0] <= 6 and m["vgpr_count"] > 128:  # __launch_bounds__(256, 4): four waves per SIMD
            bad.append(_describe(key, m))
    assert not bad, "\n".join(bad)


def test_pre_bias_instantiations_keep_their_registers(march_kernels):
    biased = {key: m for key, m in march_kernels.items() if key[2]}
    assert len(biased) == 8 * 2
    bad = []
    for key, m in sorted(biased.items()):
        print(_describe(key, m))
        limit = PRE_BIAS_VGPRS[key[0]][int(key[4])]
        if m["sgpr_spill_count"] != 0 or m["vgpr_spill_count"] != 0 or m["vgpr_count"] > limit:
            bad.append(f"{_describe(key, m)} (before the split: {limit} VGPRs, no spill)")
    assert not bad, "\n".join(bad)
