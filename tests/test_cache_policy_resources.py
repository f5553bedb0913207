"""Registers, spills and scratch of the streaming kernels against their siblings, read from the built library's gfx950 code objects (no GPU).

The cache policy "stream" (``torchio_amd/csrc/common.hpp``: ``launch_streams``) is a compile-time constant of the kernel: a
marching stencil pass that writes more than the Infinity Cache holds takes the kernel whose once-touched rows are loaded and
stored nontemporal.  The policy adds a modifier to memory instructions and nothing else, so every streaming instantiation the
launchers can name — ``conv_stream_march_kernel<R, FUSE_K, PRE_BIAS, POST_NOISE, FMA>`` (``stencil_march.hpp``), sibling
``conv_march_kernel<...>`` —

must have its sibling's ``vgpr_count``, ``sgpr_count``, spill counts and private segment size; and every sibling must have
what it had before the policy existed (``tests/golden/cache_policy_sibling_resources.json``: read off the library built from
the commit before, with the same toolchain, by ``python tests/test_cache_policy_resources.py LIBRARY > that file``).  An
instantiation that spills or leaves its occupancy class is a bug in the change, not a trade.
"""
from __future__ import annotations

import json
import os
import re
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_stencil_kernel_resources import LLVM_BIN
from test_stencil_kernel_resources import _code_object_kernels

from torchio_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_policy_sibling_resources.json")
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")

B, I = r"ELb([01])", r"ELi(\d+)"
#: kernel family -> pattern of its mangled name, one group per template argument <R, FUSE_K, PRE_BIAS, POST_NOISE, FMA>
FAMILIES = {
    "conv_march_kernel": re.compile(r"conv_march_kernelILi(\d+)" + B + B + I + B + "E"),
    "conv_stream_march_kernel": re.compile(r"conv_stream_march_kernelILi(\d+)" + B + B + I + B + "E"),
}


def kernel_key(name: str):
    """``(sibling family, template arguments, streams)`` of a mangled kernel name, or None for every other kernel."""
    for family, pattern in FAMILIES.items():
        match = pattern.search(name)
        if match is not None:
            return "conv_march_kernel", tuple(int(g) for g in match.groups()), family == "conv_stream_march_kernel"
    return None


def kernel_table(library: str) -> dict:
    """``{kernel_key: {field: value}}`` of *library*'s kernels of the families above."""
    table = {}
    for name, fields in _code_object_kernels(library).items():
        key = kernel_key(name)
        if key is not None:
            assert key not in table, f"{key} is in the library twice"
            table[key] = {field: int(fields[field]) for field in FIELDS}
    return table


def _tag(family: str, args: tuple) -> str:
    return f"{family}<{','.join(str(a) for a in args)}>"


@pytest.fixture(scope="module")
def kernels() -> dict:
    for tool in ("llvm-objdump", "llvm-readelf"):
        if not os.path.isfile(os.path.join(LLVM_BIN, tool)):
            pytest.skip(f"{tool} not found under {LLVM_BIN}")
    if not os.path.isfile(_lib.LIBRARY_PATH):
        pytest.skip(f"{_lib.LIBRARY_PATH} is not built")
    return kernel_table(_lib.LIBRARY_PATH)


def _expected_keys() -> set:
    """Every (family, arguments) the launchers can name: launch_conv and launch_conv_march_fused."""
    march = [(True, False, 0), (True, False, 1), (True, False, 2), (False, True, 0), (False, False, 0)]
    return {("conv_march_kernel", (r, int(fk), int(pb), pn, fma)) for r in range(1, 9) for fk, pb, pn in march for fma in (0, 1)}


def test_every_kernel_the_launchers_name_has_both_forms(kernels):
    assert {(family, args) for family, args, streams in kernels if streams} == _expected_keys()
    assert {(family, args) for family, args, streams in kernels if not streams} == _expected_keys()


def test_streaming_instantiations_have_their_siblings_resources(kernels):
    bad = []
    for family, args in sorted(_expected_keys()):
        stream, sibling = kernels[(family, args, True)], kernels[(family, args, False)]
        print(_tag(family, args), "stream", stream, "sibling", sibling)
        if stream != sibling:
            bad.append(f"{_tag(family, args)}: streaming {stream}, sibling {sibling}")
    assert not bad, "\n".join(bad)


def test_siblings_are_what_they_were_before_the_policy(kernels):
    with open(GOLDEN, encoding="utf-8") as file:
        before = json.load(file)
    assert set(before) == {_tag(family, args) for family, args in _expected_keys()}
    bad = []
    for family, args in sorted(_expected_keys()):
        now = kernels[(family, args, False)]
        if now != before[_tag(family, args)]:
            bad.append(f"{_tag(family, args)}: {now}, before the policy {before[_tag(family, args)]}")
    assert not bad, "\n".join(bad)


def _stores_by_kernel(library: str) -> dict:
    """``{kernel_key: [every global_store instruction with its operands, register numbers blanked]}`` of the families above."""
    import glob
    import shutil
    import subprocess
    import tempfile

    objdump = os.path.join(LLVM_BIN, "llvm-objdump")
    stores: dict = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(library, os.path.join(tmp, "in.bin"))
        subprocess.run([objdump, "--offloading", "in.bin"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for code_object in sorted(glob.glob(os.path.join(tmp, "in.bin.*gfx950*"))):
            text = subprocess.run([objdump, "-d", code_object], check=True, capture_output=True, text=True).stdout
            current = None
            for line in text.split("\n"):
                label = re.match(r"[0-9a-f]+ <(\w+)>:", line)
                if label:
                    current = kernel_key(label.group(1))
                    if current is not None:
                        stores[current] = []
                elif current is not None and "global_store_" in line:
                    instruction = " ".join(line.split("//")[0].split())
                    stores[current].append(re.sub(r"\[\d+:\d+\]", "[:]", re.sub(r"\bv\d+", "v", instruction)))
    return stores


def test_streaming_stores_carry_nt_in_their_siblings_addressing_form(kernels):
    """Instruction for instruction a streaming kernel has its sibling's global stores, the row stores of the marching loop with
    the ``nt`` modifier (whole rows: ``global_store_dwordx4 ... nt``), and a sibling has none with it."""
    stores = _stores_by_kernel(_lib.LIBRARY_PATH)
    for family, args in sorted(_expected_keys()):
        streamed, plain = stores[(family, args, True)], stores[(family, args, False)]
        what = _tag(family, args)
        assert not [op for op in plain if op.endswith(" nt")], what
        assert [op.removesuffix(" nt") for op in streamed] == plain, what
        nt = [op for op in streamed if op.endswith(" nt")]
        print(what, f"{len(nt)} of {len(streamed)} global stores with nt")
        assert nt and all(op.startswith("global_store_dwordx4 ") for op in nt), (what, nt)


if __name__ == "__main__":  # the recorded table: python tests/test_cache_policy_resources.py LIBRARY_OF_THE_COMMIT_BEFORE > GOLDEN
    recorded = {_tag(family, args): fields for (family, args, streams), fields in sorted(kernel_table(sys.argv[1]).items()) if not streams}
    json.dump(recorded, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
