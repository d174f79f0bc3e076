#!/usr/bin/env python3
"""Launch table of ONE host-pointer prove call, from the engine's own per-launch events (bbp_set_profiling / bbp_last_timings):

    python tools/prove_launches.py [--checked | --round] profiles/r10_prove_round_launches_after.csv [B] [N]

--checked: the call is made with checked proving on (bbp_set_prove_check); --round: the call is bbp_prove_round.  Both take honest
bids (tests/prove_round_cases.py), since a zero row does not satisfy the circuit and a zero bid is in no list.

One row per kernel tag (context.h TAG_*) with the number of launches the call made, then the tags in the order the host enqueued
them.  The file holds no timings, so two builds that enqueue the same work give byte-identical files: how "bbp_prove_batch's launch
sequence did not change" is checked ("Proving a round from raw bids").  Rows are all-zero dummy rows with all-zero
entropy (what bbp_reserve proves): the launch sequence does not depend on the data.

With BBP_OPEN_ON_CHAIN=1 in the environment every row ends in one more column, the chain stream the call's launches ran on (side,
lane[1] or lane[2]: internal stream 1 + call % 3 of the engine's own BBP_TRACE_PROVE line; `none`: the call did not rotate).  Without it
the file is what it always was.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAGS = {1: "msm_acc", 2: "encode", 3: "witness", 4: "rng", 5: "poly", 6: "ipa_scalars", 7: "commit", 8: "transcript", 9: "verify_scalars",
        10: "varbase", 11: "msm_sort", 12: "msm_fold", 13: "wipe"}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    checked, as_round = "--checked" in sys.argv, "--round" in sys.argv
    out = args[0]
    B = int(args[1]) if len(args) > 1 else 64
    N = int(args[2]) if len(args) > 2 else 8
    chain_column = os.environ.get("BBP_OPEN_ON_CHAIN") == "1"
    if chain_column:
        os.environ["BBP_TRACE_PROVE"] = "1"  # read by bbp_init
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
    if chain_column:  # the engine writes its trace lines to the C stderr: into a file for this call
        import tempfile
        sys.stderr.flush()
        keep, tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(tmp.fileno(), 2)
    try:
        st = call()
    finally:
        if chain_column:
            os.dup2(keep, 2)
            os.close(keep)
    assert st == [0] * B, st
    tags = [t for t, _ in ctx.last_timings()]
    ctx.set_profiling(False)
    chain = ""
    if chain_column:
        tmp.seek(0)
        plans = re.findall(r"prove call (\d+): .* rotate (\d) ", tmp.read().decode())
        chain = "," + "+".join(sorted({("lane[1]", "lane[2]", "side")[int(k) % 3] if r == "1" else "none" for k, r in plans}))
    with open(out, "w") as f:
        f.write("call,B,N\n%s%s,%d,%d\ntag,name,launches%s\n" % ("bbp_prove_round" if as_round else "bbp_prove_batch", " checked" if checked else "", B, N,
                                                                 ",chain_stream" if chain else ""))
        for t in sorted(set(tags)):
            f.write("%d,%s,%d%s\n" % (t, TAGS.get(t, "?"), tags.count(t), chain))
        f.write("order,%s\n" % " ".join(str(t) for t in tags))
    print("%d launches -> %s" % (len(tags), out))
    ctx.close()


if __name__ == "__main__":
    main()
