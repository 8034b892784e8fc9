#!/usr/bin/env python3
r"""Per-kernel comparison of the gfx950 disassembly of two builds of libglrtx.so: which kernels are new, gone, or changed.

    python tools/isa_diff.py [--rename REGEX=REPLACEMENT ...] OTHER/libglrtx.so [THIS/libglrtx.so]      # exit 1 if a kernel present in both differs

A pull request that adds kernels to the translation unit shows with it that every kernel it did not mean to touch still compiles to the same
instructions.  Compared per symbol, by demangled name: mnemonics and operands of every instruction in order; addresses and encodings are dropped (a kernel
moves when another is added in front of it), as are the pc-relative literals that follow s_getpc_b64 (distances to other symbols).
--rename (repeatable, applied in order with re.sub to the demangled names of OTHER) compares a renamed kernel against its successor instead of
listing it as GONE and NEW.  From the commit before pt_render_persistent and features_tree became one template each (9558ec0) to its successor:

    --rename 'pt_render_persistent<(\w+), (\w+), (\w+)>(.*)glrtx::VolArgs\)=pt_render_persistent<\1, \2, \3, false, false, false>\4std::conditional<false, glrtx::EnvArgs, glrtx::VolArgs>::type)'
    --rename 'pt_render_persistent_tex<(\w+), (\w+), (\w+)>(.*)glrtx::VolArgs\)=pt_render_persistent<\1, true, \2, true, false, \3>\4std::conditional<false, glrtx::EnvArgs, glrtx::VolArgs>::type)'
    --rename 'pt_render_persistent_env<(\w+), (\w+), (\w+)>(.*)glrtx::EnvArgs\)=pt_render_persistent<\1, true, false, \2, true, \3>\4std::conditional<true, glrtx::EnvArgs, glrtx::VolArgs>::type)'
    --rename 'features_tree<(\w+)>=features_tree<\1, glrtx::features::Args>'
    --rename 'features_tree_\w+<(\w+)>\(glrtx::features::(\w+)\)=features_tree<\1, glrtx::features::\2>(glrtx::features::\2)'

From the commit before pt_render_persistent gained its CUT argument (66f6c1f) to its successor (608 symbols identical, 9 new):

    --rename 'pt_render_persistent<(\w+), (\w+), (\w+), (\w+), (\w+), (\w+)>(.*)std::conditional<(\w+), glrtx::EnvArgs, glrtx::VolArgs>::type\)=pt_render_persistent<\1, \2, \3, \4, \5, \6, false>\7std::conditional<false, glrtx::CutTail<std::conditional<\8, glrtx::EnvArgs, glrtx::VolArgs>::type>, std::conditional<\8, glrtx::EnvArgs, glrtx::VolArgs>::type>::type)'

From the commit before pt_render_persistent gained its EMIT argument (b9c727a) to its successor (625 symbols identical, 21 new; the kernel's name keeps
its seven arguments, the type of its last parameter is spelled anew):

    --rename '(pt_render_persistent<.*)std::conditional<(\w+), glrtx::CutTail<std::conditional<(\w+), glrtx::EnvArgs, glrtx::VolArgs>::type>, std::conditional<\w+, glrtx::EnvArgs, glrtx::VolArgs>::type>::type\)=\1std::conditional<((0)>(0)), glrtx::EmitTail<std::conditional<\3, glrtx::EnvArgs, glrtx::VolArgs>::type>, std::conditional<\2, glrtx::CutTail<std::conditional<\3, glrtx::EnvArgs, glrtx::VolArgs>::type>, std::conditional<\3, glrtx::EnvArgs, glrtx::VolArgs>::type>::type>::type)'

Works without a GPU (tools/isa_report.py's extraction, llvm-objdump from /opt/rocm).
"""
from __future__ import annotations

import argparse
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


def by_name(lib: pathlib.Path, renames=()) -> dict[str, list[str]]:
    fs = functions(lib)
    names = isa_report.demangle(sorted(fs))
    out = {}
    for sym, ins in fs.items():
        n = names[sym]
        for rx, to in renames:
            n = re.sub(rx, to, n)
        assert n not in out, f"{lib}: two symbols named {n}"
        out[n] = ins
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("this", nargs="?", default=str(isa_report.LIB))
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT")
    args = ap.parse_args()
    a = by_name(pathlib.Path(args.other), [r.split("=", 1) for r in args.rename])
    b = by_name(pathlib.Path(args.this))
    same = changed = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
        else:
            changed += 1
            print(f"CHANGED  {n}  ({len(a[n])} -> {len(b[n])} instructions)")
    for n in sorted(set(a) - set(b)):
        print(f"GONE     {n}")
    for n in sorted(set(b) - set(a)):
        print(f"NEW      {n}  ({len(b[n])} instructions)")
    print(f"{same} symbols identical, {changed} changed, {len(set(a) - set(b))} gone, {len(set(b) - set(a))} new")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
