#!/usr/bin/env python3
"""Launch table of ONE host-pointer prove call, from the engine's own per-launch events (bbp_set_profiling / bbp_last_timings):

    python tools/prove_launches.py [--checked | --round] profiles/r10_prove_round_launches_after.csv [B] [N]

--checked: the call is made with checked proving on (bbp_set_prove_check); --round: the call is bbp_prove_round.  Both take honest
bids (tests/prove_round_cases.py), since a zero row does not satisfy the circuit and a zero bid is in no list.

One row per kernel tag (context.h TAG_*) with the number of launches the call made, then the tags in the order the host enqueued
them.  The file holds no timings, so two builds that enqueue the same work give byte-identical files: how "bbp_prove_batch's launch
sequence did not change" is checked ("Proving a round from raw bids").  Rows are all-zero dummy rows with all-zero
entropy (what bbp_reserve proves): the launch sequence does not depend on the data.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAGS = {1: "msm_acc", 2: "encode", 3: "witness", 4: "rng", 5: "poly", 6: "ipa_scalars", 7: "commit", 8: "transcript", 9: "verify_scalars",
        10: "varbase", 11: "msm_sort", 12: "msm_fold"}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    checked, as_round = "--checked" in sys.argv, "--round" in sys.argv
    out = args[0]
    B = int(args[1]) if len(args) > 1 else 64
    N = int(args[2]) if len(args) > 2 else 8
    import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
    import dusk_blindbidproof_amd as bbp
    ctx = bbp.Context(0)
    rows, ent = bytes((7 * 32 + 32 * N + 8) * B), bytes(bbp.entropy_size(N) * B)
    if checked or as_round:
        from tests import prove_round_cases as rc
        r = rc.honest(N, B, tag=8)
        rows = r.in_rows()
    ctx.set_prove_check(checked)
    call = (lambda: ctx.prove_round(N, r.table, r.bid_bytes, ent)[2]) if as_round else (lambda: ctx.prove_batch(B, N, rows, ent)[1])
    call()  # buffers and circuit exist afterwards
    ctx.set_profiling(True)
    ctx.last_timings()
    st = call()
    assert st == [0] * B, st
    tags = [t for t, _ in ctx.last_timings()]
    ctx.set_profiling(False)
    with open(out, "w") as f:
        f.write("call,B,N\n%s%s,%d,%d\ntag,name,launches\n" % ("bbp_prove_round" if as_round else "bbp_prove_batch", " checked" if checked else "", B, N))
        for t in sorted(set(tags)):
            f.write("%d,%s,%d\n" % (t, TAGS.get(t, "?"), tags.count(t)))
        f.write("order,%s\n" % " ".join(str(t) for t in tags))
    print("%d launches -> %s" % (len(tags), out))
    ctx.close()


if __name__ == "__main__":
    main()
