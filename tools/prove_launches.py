#!/usr/bin/env python3
"""Launch table of ONE bbp_prove_batch call, from the engine's own per-launch events (bbp_set_profiling / bbp_last_timings):

    python tools/prove_launches.py profiles/r10_prove_round_launches_after.csv [B] [N]

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
    out = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
    import dusk_blindbidproof_amd as bbp
    ctx = bbp.Context(0)
    rows, ent = bytes((7 * 32 + 32 * N + 8) * B), bytes(bbp.entropy_size(N) * B)
    ctx.prove_batch(B, N, rows, ent)  # buffers and circuit exist afterwards
    ctx.set_profiling(True)
    ctx.last_timings()
    _, st = ctx.prove_batch(B, N, rows, ent)
    assert st == [0] * B, st
    tags = [t for t, _ in ctx.last_timings()]
    ctx.set_profiling(False)
    with open(out, "w") as f:
        f.write("call,B,N\nbbp_prove_batch,%d,%d\ntag,name,launches\n" % (B, N))
        for t in sorted(set(tags)):
            f.write("%d,%s,%d\n" % (t, TAGS.get(t, "?"), tags.count(t)))
        f.write("order,%s\n" % " ".join(str(t) for t in tags))
    print("%d launches -> %s" % (len(tags), out))
    ctx.close()


if __name__ == "__main__":
    main()
