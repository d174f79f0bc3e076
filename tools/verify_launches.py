#!/usr/bin/env python3
"""Launch table of ONE host-pointer verify call, from the engine's own per-launch events (bbp_set_profiling / bbp_last_timings); the
sibling of tools/prove_launches.py:

    python tools/verify_launches.py [--mixed | --round | --rounds] [--aggregated] profiles/r13_verify_launches_uniform_plain_after.csv [B] [N]

no flag: bbp_verify_batch at list length N; --mixed: bbp_verify_batch_mixed over N = 1, 8, 202 in turn; --round: bbp_verify_rounds
with one round of length N; --rounds: with three rounds of 1, 8, 202.  --aggregated: the aggregated form of the same call, groups
of 8.

One row per kernel tag (context.h TAG_*) with the number of launches the call made, then the tags in the order the host enqueued
them.  The file holds no timings, so two builds that enqueue the same work give byte-identical files: how "the verify call's launch
sequence did not change" is checked (DESIGN.md "The plan of a verify call").  Rows and tables are all zero -- every row is refused
as malformed -- since the launch sequence does not depend on the data: the aggregated engine's fallback launches size themselves
on the device.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.prove_launches import TAGS  # noqa: E402

MIX = (1, 8, 202)
G = 8


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = {a for a in sys.argv[1:] if a.startswith("--")}
    assert flags <= {"--mixed", "--round", "--rounds", "--aggregated"} and len(flags - {"--aggregated"}) <= 1, flags
    out = args[0]
    B = int(args[1]) if len(args) > 1 else 64
    N = int(args[2]) if len(args) > 2 else 8
    agg = "--aggregated" in flags
    import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
    import dusk_blindbidproof_amd as bbp
    ctx = bbp.Context(0)
    Ns = [MIX[i % len(MIX)] for i in range(B)]
    if "--mixed" in flags:
        name, shape, blob = "bbp_verify_batch_mixed", "1+8+202", bytes(sum(bbp.verify_row_size(n) for n in Ns))
        call = (lambda: ctx.verify_batch_mixed_aggregated(Ns, blob, G)[0]) if agg else (lambda: ctx.verify_batch_mixed(Ns, blob))
    elif "--rounds" in flags:
        name, shape, blob = "bbp_verify_rounds", "1+8+202", bytes(sum(bbp.round_row_size(n) for n in Ns))
        table, of = bytes(sum(32 * (1 + n) for n in MIX)), [i % len(MIX) for i in range(B)]
        call = (lambda: ctx.verify_rounds_aggregated(list(MIX), table, of, blob, G)[0]) if agg else (lambda: ctx.verify_rounds(list(MIX), table, of, blob))
    elif "--round" in flags:
        name, shape, blob, table = "bbp_verify_rounds one round", str(N), bytes(bbp.round_row_size(N) * B), bytes(32 * (1 + N))
        call = (lambda: ctx.verify_rounds_aggregated([N], table, None, blob, G)[0]) if agg else (lambda: ctx.verify_rounds([N], table, None, blob))
    else:
        name, shape, blob = "bbp_verify_batch", str(N), bytes(bbp.verify_row_size(N) * B)
        call = (lambda: ctx.verify_batch_aggregated(B, N, blob, G)[0]) if agg else (lambda: ctx.verify_batch(B, N, blob))
    call()  # buffers and circuits exist afterwards
    ctx.set_profiling(True)
    ctx.last_timings()
    st = call()
    assert len(st) == B and 0 not in st, st  # no zero row is a proof
    tags = [t for t, _ in ctx.last_timings()]
    ctx.set_profiling(False)
    with open(out, "w") as f:
        f.write("call,B,N\n%s%s,%d,%s\ntag,name,launches\n" % (name, " aggregated" if agg else "", B, shape))
        for t in sorted(set(tags)):
            f.write("%d,%s,%d\n" % (t, TAGS.get(t, "?"), tags.count(t)))
        f.write("order,%s\n" % " ".join(str(t) for t in tags))
    print("%d launches -> %s" % (len(tags), out))
    ctx.close()


if __name__ == "__main__":
    main()
