#!/usr/bin/env python3
"""Compare two device assemblies of one .hip file (hipcc -S --cuda-device-only, the product's flags) function body by function
body: the proof that a refactoring left existing kernels instruction for instruction what they were.  Labels are renumbered and
comments dropped (both carry the function's index in the file, which moves when kernels are added); everything else must match.

    python tools/kernel_asm_diff.py before.s after.s [--match REGEX]

Prints one line per function of `before` (lines, differing lines) and exits 1 when a body differs or is missing in `after`."""
import argparse
import difflib
import re
import sys


def bodies(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = []
        for ln in m.group(2).splitlines():
            ln = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?", ".L", ln.split(";")[0]).rstrip()
            if ln and not ln.lstrip().startswith((".loc", ".file", ".cfi")):
                lines.append(ln)
        out[m.group(1)] = lines
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--match", default="", help="only functions whose mangled name matches this regular expression")
    a = ap.parse_args()
    old, new = bodies(a.before), bodies(a.after)
    bad = 0
    for name, body in old.items():
        if a.match and not re.search(a.match, name):
            continue
        if name not in new:
            print(f"MISSING {name}")
            bad += 1
            continue
        d = sum(1 for ln in difflib.unified_diff(body, new[name], lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
        print(f"{'same   ' if d == 0 else 'DIFFERS'} {len(body):6d} lines {d:6d} differ  {name[:72]}")
        bad += d != 0
    for name in new:
        if name not in old and (not a.match or re.search(a.match, name)):
            print(f"new     {len(new[name]):6d} lines                {name[:72]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
