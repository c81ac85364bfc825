#!/usr/bin/env python3
"""Compares two assembly listings of one translation unit kernel by kernel.

    hipcc <the library's flags> --cuda-device-only -S crt_mega3.hip -o a.s      (cudaraytracing_amd/build.py: COMMON + DEVICE)
    python tools/isa_diff.py parent.s this.s [--markdown] [--show SYMBOL]

A listing is split by kernel symbol (.amdhsa_kernel names them); of each kernel's text only the instructions and labels count:
directives, comments and blank lines are dropped, and the .LBB<function>_<block> labels are renumbered by first appearance within
the kernel, because the function index changes with the order in which the templates are instantiated.  Per symbol: equal / differs,
instruction count, VGPRs, SGPRs, private segment bytes (scratch), group segment bytes (LDS).  Exit status 1 when the symbol sets or
any stream differ.
"""
import argparse
import difflib
import re
import sys

LABEL = re.compile(r"\.LBB\d+_\d+")
DESC = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "scratch": "private_segment_fixed_size", "lds": "group_segment_fixed_size"}


def strip_comment(line):
    """The line without its ';' or '//' comment (no string literal of a kernel's text holds either)."""
    for mark in (";", "//"):
        k = line.find(mark)
        if k >= 0:
            line = line[:k]
    return line.strip()


def parse(path):
    """{symbol: {"code": [lines], "vgpr": .., "sgpr": .., "scratch": .., "lds": ..}} of the kernels of a listing."""
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        lines = f.read().split("\n")
    kernels, bodies = {}, {}
    n = len(lines)
    for i in range(n):  # the kernel descriptors (they sit between a kernel's last instruction and its .Lfunc_end)
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", lines[i].strip())
        if not m:
            continue
        d, j = {}, i + 1
        while j < n and not lines[j].strip().startswith(".end_amdhsa_kernel"):
            t = lines[j].split()
            for k, name in DESC.items():
                if len(t) == 2 and t[0] == ".amdhsa_" + name:
                    d[k] = int(t[1], 0)
            j += 1
        kernels[m.group(1)] = d
    i = 0
    while i < n:  # a function's text runs from its entry label to .Lfunc_end
        s = lines[i].strip()
        m = re.match(r"([A-Za-z_$][\w$.]*):", s)
        if m and not s.startswith(".L") and m.group(1) not in bodies:
            j = i + 1
            while j < n and not lines[j].strip().startswith(".Lfunc_end"):
                j += 1
            if j < n:
                bodies[m.group(1)] = lines[i + 1:j]
                i = j
        i += 1
    for sym, d in kernels.items():
        names, code = {}, []
        for raw in bodies.get(sym, []):
            s = strip_comment(raw)
            if not s or (s.startswith(".") and not LABEL.match(s)):  # blank, comment or directive
                continue
            code.append(LABEL.sub(lambda mm: names.setdefault(mm.group(0), ".L%d" % len(names)), s))
        d["code"] = code
        d["insts"] = sum(1 for c in code if not c.endswith(":"))
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--markdown", action="store_true", help="print the table as a markdown table")
    ap.add_argument("--show", metavar="SYMBOL", help="print the unified diff of that kernel's streams")
    o = ap.parse_args()
    A, B = parse(o.a), parse(o.b)
    bad = 0
    for sym in sorted(set(A) - set(B)):
        print("only in %s: %s" % (o.a, sym)); bad += 1
    for sym in sorted(set(B) - set(A)):
        print("only in %s: %s" % (o.b, sym)); bad += 1
    cols = ("insts", "vgpr", "sgpr", "scratch", "lds")
    if o.markdown:
        print("| kernel | streams | instructions | VGPRs | SGPRs | scratch B | LDS B |")
        print("|---|---|---|---|---|---|---|")
    for sym in sorted(set(A) & set(B)):
        a, b = A[sym], B[sym]
        same = a["code"] == b["code"] and len(a["code"]) > 0
        bad += 0 if same else 1
        cells = [str(a.get(c)) if a.get(c) == b.get(c) else "%s -> %s" % (a.get(c), b.get(c)) for c in cols]
        if o.markdown:
            print("| `%s` | %s | %s |" % (sym, "equal" if same else "**differs**", " | ".join(cells)))
        else:
            print("%-7s %s  insts %s  vgpr %s  sgpr %s  scratch %s  lds %s" % (("equal" if same else "DIFFERS", sym) + tuple(cells)))
        if o.show == sym and not same:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a["code"], b["code"], o.a, o.b, lineterm="", n=2))
    n_same = len(set(A) & set(B)) - sum(1 for s in set(A) & set(B) if A[s]["code"] != B[s]["code"] or not A[s]["code"])
    print("%d kernels in %s, %d in %s; %d streams equal, %d differ or are missing" % (len(A), o.a, len(B), o.b, n_same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
