#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 disassembly of two builds of libglrtx.so: which kernels are new, gone, or changed.

    python tools/isa_diff.py OTHER/libglrtx.so [THIS/libglrtx.so]      # exit 1 if a kernel present in both differs

A pull request that adds kernels to the translation unit shows with it that every kernel it did not mean to touch still compiles to the same
instructions.  Compared per symbol: mnemonics and operands of every instruction in order; addresses and encodings are dropped (a kernel moves when
another is added in front of it), as are the pc-relative literals that follow s_getpc_b64 (distances to other symbols).
Works without a GPU (tools/isa_report.py's extraction, llvm-objdump from /opt/rocm).
"""
from __future__ import annotations

import pathlib
import re
import subprocess
import sys
import tempfile

import isa_report


def functions(lib: pathlib.Path) -> dict[str, list[str]]:
    with tempfile.TemporaryDirectory() as td:
        co = isa_report.extract(lib, pathlib.Path(td))
        text = subprocess.run([str(isa_report.LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
    out, cur, pcrel = {}, None, 0
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not ln.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", ln).strip()
        ins = re.sub(r"\s*<[^>]+>", "", ins)
        if ins.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_add(c)?_u32 ", ins):  # the two halves of a pc-relative address
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "PCREL", ins)
            pcrel -= 1
        cur.append(ins)
    return out


def main() -> int:
    if len(sys.argv) < 2:
        print(__doc__)
        return 2
    a = functions(pathlib.Path(sys.argv[1]))
    b = functions(pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else isa_report.LIB)
    names = isa_report.demangle(sorted(set(a) | set(b)))
    same = changed = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
        else:
            changed += 1
            print(f"CHANGED  {names[n]}  ({len(a[n])} -> {len(b[n])} instructions)")
    for n in sorted(set(a) - set(b)):
        print(f"GONE     {names[n]}")
    for n in sorted(set(b) - set(a)):
        print(f"NEW      {names[n]}  ({len(b[n])} instructions)")
    print(f"{same} symbols identical, {changed} changed, {len(set(a) - set(b))} gone, {len(set(b) - set(a))} new")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
