#!/usr/bin/env python3
"""Function-by-function comparison of device assembly listings, the check behind "the existing kernels are byte-identical"
(DESIGN.md section 11).  Needs no GPU:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S dusk_blindbidproof_amd/csrc/prover.hip -o before.s   # parent commit
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S dusk_blindbidproof_amd/csrc/prover.hip -o after.s
    python tools/asm_functions_diff.py before.s after.s

Either side may be several listings, the sides separated by "--": a translation unit that was split is compared against the union
of the units it became, and a function that appears in more than one listing of a side is reported.

    python tools/asm_functions_diff.py capi_prove.before.s -- capi_prove.s capi_best.s capi_bests.s capi_verify.s capi_ctx.s

A function is the text between its label and its .Lfunc_end.  Basic-block labels carry the function's ordinal in the file
(.LBB59_5), which moves when functions are added ahead of it or move to another unit: they are compared with the ordinal removed
(and with it the padding in front of a label's comment, which follows the ordinal's width).  Exit status 1 when a
function present on both sides differs, or when a side holds a function twice.
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
                line = re.sub(r"BB\d+_", "BB_", line)
                # a label's comment is padded to a column: the padding moves with the ordinal's width
                buf.append(re.sub(r"^(\.LBB_\d+:)\s+;", r"\1 ;", line))
    return out


def side(paths):
    """the functions of all listings of one side, and the names that more than one listing holds"""
    out, doubled = {}, set()
    for p in paths:
        for name, text in functions(p).items():
            if name in out:
                doubled.add(name)
            out[name] = text
    return out, sorted(doubled)


def main():
    args = sys.argv[1:]
    if "--" in args:
        before, after = args[:args.index("--")], args[args.index("--") + 1:]
    else:
        before, after = args[:1], args[1:]
    if not before or not after:
        sys.exit(__doc__)
    (a, a_doubled), (b, b_doubled) = side(before), side(after)
    changed = sorted(f for f in a if f in b and a[f] != b[f])
    print("functions: %d before, %d after, %d identical" % (len(a), len(b), sum(1 for f in a if f in b and a[f] == b[f])))
    print("changed:", changed)
    print("removed:", sorted(f for f in a if f not in b))
    print("new:", sorted(f for f in b if f not in a))
    print("doubled:", a_doubled + b_doubled)
    return 1 if changed or a_doubled or b_doubled else 0


if __name__ == "__main__":
    sys.exit(main())
