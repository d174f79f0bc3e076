#!/usr/bin/env python3
"""Function-by-function comparison of two device assembly listings of one translation unit, the check behind "the existing kernels
are byte-identical" (DESIGN.md section 11).  Needs no GPU:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S dusk_blindbidproof_amd/csrc/prover.hip -o before.s   # parent commit
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S dusk_blindbidproof_amd/csrc/prover.hip -o after.s
    python tools/asm_functions_diff.py before.s after.s

A function is the text between its label and its .Lfunc_end.  Basic-block labels carry the function's ordinal in the file
(.LBB59_5), which moves when functions are added ahead of it: they are compared with the ordinal removed.  Exit status 1 when a
function present in both listings differs.
"""
import re
import sys


def functions(path):
    out, cur, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L") and cur is None:
            cur, buf = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                out[cur], cur = buf, None
            else:
                buf.append(re.sub(r"BB\d+_", "BB_", line))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    changed = sorted(f for f in a if f in b and a[f] != b[f])
    print("functions: %d before, %d after, %d identical" % (len(a), len(b), sum(1 for f in a if f in b and a[f] == b[f])))
    print("changed:", changed)
    print("removed:", sorted(f for f in a if f not in b))
    print("new:", sorted(f for f in b if f not in a))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
