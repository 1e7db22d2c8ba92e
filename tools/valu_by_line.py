#!/usr/bin/env python3
"""The static instruction count of tools/valu_mix.py, attributed to source lines.

    hipcc <the Makefile's FLAGS> -gline-tables-only -c -o /tmp/fused_g.o qldpc_amd/csrc/qbp_tu_fused.hip
    python tools/valu_by_line.py --obj /tmp/fused_g.o [--kernel SUBSTR] [--per-trip N]

The object (or library) must carry line tables; they do not change the machine code, which the tool checks
against --so (the library the benchmark loads) when given: same loop length, same counts per class.  Every
vector-ALU instruction that valu_mix.loop_mix counts (main loop, minus once-per-syndrome and marked cold regions)
is listed under the innermost source line `llvm-objdump -l` names for it, by issue class.  --per-trip: iterations
per trip of the loop (2 for the one-barrier forced build), printed counts are per trip; the per-iteration total is
the sum divided by it.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valu_mix  # noqa: E402


def lines_of(co_bytes):
    """{address: 'file:line'} of one code object"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co_bytes)
        f.flush()
        txt = subprocess.check_output([os.path.join(valu_mix.LLVM, "llvm-objdump"), "-d", "-l", f.name], text=True)
    where, cur = {}, "?"
    loc = re.compile(r"^; (\S+):(\d+)\s*$")
    ins = re.compile(r"//\s*([0-9A-Fa-f]+):")
    for ln in txt.splitlines():
        m = loc.match(ln)
        if m:
            cur = f"{os.path.basename(m.group(1))}:{m.group(2)}"
            continue
        m = ins.search(ln)
        if m:
            where[int(m.group(1), 16)] = cur
    return where


def source_text(csrc, where):
    name, _, line = where.partition(":")
    try:
        return open(os.path.join(csrc, name)).read().splitlines()[int(line) - 1].strip()
    except Exception:
        return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", required=True, help="object or library built with -gline-tables-only")
    ap.add_argument("--so", default=None, help="library to check the counts against")
    ap.add_argument("--kernel", default="bp_fused_kernel<6, 3, 0, false, true, 1024, 1, true>")
    ap.add_argument("--per-trip", type=int, default=2)
    ap.add_argument("--src", default=os.path.join(valu_mix.ROOT, "qldpc_amd", "csrc"),
                    help="directory of the sources the object was built from (for the text of the lines)")
    args = ap.parse_args()
    funcs = valu_mix.disassemble(args.obj)
    sym = [s for s in funcs if args.kernel in valu_mix.demangle(s) or args.kernel in s]
    if len(sym) != 1:
        sys.exit(f"{len(sym)} kernels match {args.kernel!r}")
    counted = []
    mix = valu_mix.loop_mix(funcs[sym[0]], counted)
    where = {}
    for co in valu_mix.extract_code_objects(args.obj):
        w = lines_of(co)
        if all(a in w for a, _, _ in counted):
            where = w
            break
    if args.so:
        ref = valu_mix.analyse(args.so, [args.kernel])
        ref = next(iter(ref.values()))
        if ref["valu_by_class"] != mix["valu_by_class"]:
            sys.exit(f"line-table build differs from {args.so}: {mix['valu_by_class']} != {ref['valu_by_class']}")
    csrc = args.src
    classes = [c for c, _ in valu_mix.CLASSES]
    by_line = collections.defaultdict(collections.Counter)
    mnem = collections.defaultdict(collections.Counter)
    for a, m, c in counted:
        by_line[where.get(a, "?")][c] += 1
        mnem[where.get(a, "?")][m] += 1

    def key(w):
        name, _, line = w.partition(":")
        return (name, int(line) if line.isdigit() else 0)
    print(f"kernel: {valu_mix.demangle(sym[0])}")
    print(f"loop {mix['loop'][0]} .. {mix['loop'][1]}: {mix['valu_total']} vector-ALU instructions per trip "
          f"({args.per_trip} iterations: {mix['valu_total'] / args.per_trip:g} per wave-iteration); "
          f"{mix['valu_in_cold_regions']} more in cold regions")
    print("per trip, by class: " + ", ".join(f"{c} {mix['valu_by_class'].get(c, 0)}" for c in classes))
    print()
    print(f"{'source line':24s} {'all':>4s} " + " ".join(f"{c[:9]:>9s}" for c in classes) + "  text / 32-bit mnemonics")
    for w in sorted(by_line, key=key):
        row = by_line[w]
        ints = ", ".join(f"{n} {m}" for m, n in mnem[w].most_common() if "_f64" not in m)
        print(f"{w:24s} {sum(row.values()):4d} " + " ".join(f"{row.get(c, 0) or '.':>9}" for c in classes) +
              f"  {source_text(csrc, w)[:70]}" + (f"   [{ints}]" if ints else ""))
    tot = collections.Counter()
    for row in by_line.values():
        tot.update(row)
    print(f"{'total':24s} {sum(tot.values()):4d} " + " ".join(f"{tot.get(c, 0):>9}" for c in classes))


if __name__ == "__main__":
    main()
