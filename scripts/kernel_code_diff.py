#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel (no GPU).

    python scripts/kernel_code_diff.py BEFORE AFTER

BEFORE and AFTER are each a ``libtio_hip.so``, an object file, or a directory (its ``*.o`` files are the set).  Every bundled
gfx950 code object is unbundled (``llvm-objdump --offloading``) and disassembled; the instructions are keyed by mangled
symbol, without the ``//`` address comments and without the padding behind a symbol's last real instruction (``s_nop``,
``s_code_end`` and objdump's ``...`` for a zero fill: that fill depends on what the linker lays out next).  Each kernel's
metadata note (registers, spills, segment sizes, workgroup size) is compared as well.  Prints the symbols of one side only,
the symbols whose instructions or metadata differ, and a line of totals; exits 1 when anything differs.
"""
from __future__ import annotations

import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("TIO_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
METADATA = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
            "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")
PADDING = re.compile(r"s_nop\b|s_code_end\b|\.\.\.$")


def _tool(name: str) -> str:
    return os.path.join(LLVM_BIN, name)


def _inputs(path: str) -> list:
    return sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]


def read_side(path: str) -> tuple:
    """``({symbol: [instruction, ...]}, {kernel: {metadata key: value}})`` of every gfx950 code object under *path*."""
    code, meta = {}, {}
    for binary in _inputs(path):
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(binary, os.path.join(tmp, "in.bin"))
            subprocess.run([_tool("llvm-objdump"), "--offloading", "in.bin"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
            for code_object in sorted(glob.glob(os.path.join(tmp, "in.bin.*gfx950*"))):
                text = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", code_object],
                                      check=True, capture_output=True, text=True).stdout
                symbol = None
                for line in text.splitlines():
                    header = re.fullmatch(r"<(.+)>:", line.strip())
                    if header:
                        symbol = header.group(1)
                        assert symbol not in code, f"{symbol} is in {path} twice"
                        code[symbol] = []
                    elif symbol is not None and line.strip():
                        code[symbol].append(line.split("//")[0].strip())
                notes = subprocess.run([_tool("llvm-readelf"), "--notes", code_object], check=True, capture_output=True, text=True).stdout
                for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:  # one block per kernel: .agpr_count is its first key
                    fields = dict(re.findall(r"\.(\w+):\s+(\S+)", block), agpr_count=block.split()[0])
                    meta[fields["name"]] = {key: fields.get(key) for key in METADATA}
    for lines in code.values():
        while lines and PADDING.match(lines[-1]):
            lines.pop()
    return code, meta


def main(argv: list) -> int:
    if len(argv) != 3:
        print(__doc__)
        return 2
    (code_a, meta_a), (code_b, meta_b) = read_side(argv[1]), read_side(argv[2])
    version = subprocess.run([_tool("llvm-objdump"), "--version"], check=True, capture_output=True, text=True).stdout
    print("toolchain:", next((line.strip() for line in version.splitlines() if "version" in line), "unknown"))
    only_a, only_b = sorted(set(code_a) - set(code_b)), sorted(set(code_b) - set(code_a))
    for name in only_a:
        print(f"only in {argv[1]}: {name}")
    for name in only_b:
        print(f"only in {argv[2]}: {name}")
    common = sorted(set(code_a) & set(code_b))
    text_differs = [name for name in common if code_a[name] != code_b[name]]
    for name in text_differs:
        a, b = code_a[name], code_b[name]
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"instructions differ: {name}: {len(a)} -> {len(b)} lines, first difference at line {first}: "
              f"{a[first] if first < len(a) else '<end>'!r} -> {b[first] if first < len(b) else '<end>'!r}")
    meta_differs = [name for name in sorted(set(meta_a) & set(meta_b)) if meta_a[name] != meta_b[name]]
    for name in meta_differs:
        changed = {key: (meta_a[name][key], meta_b[name][key]) for key in METADATA if meta_a[name][key] != meta_b[name][key]}
        print(f"metadata differs: {name}: {changed}")
    meta_only = sorted(set(meta_a) ^ set(meta_b))
    print(f"totals: {len(code_a)} / {len(code_b)} symbols, {len(meta_a)} / {len(meta_b)} kernels with metadata, "
          f"{sum(len(v) for v in code_a.values())} / {sum(len(v) for v in code_b.values())} instructions; "
          f"{len(only_a) + len(only_b)} symbols on one side only, {len(text_differs)} with different instructions, "
          f"{len(meta_differs) + len(meta_only)} with different metadata")
    return 1 if only_a or only_b or text_differs or meta_differs or meta_only else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
