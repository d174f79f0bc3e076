#!/usr/bin/env python3
"""bbp_prove_round against the path it replaces, and its device pass against bbp_prepare_bids_dev's kernel:

    python tools/prove_round.py profiles/r10_prove_round.jsonl

One process, one context, the two arms alternated; a run is the best of 5 calls after 2 warm-ups, 5 runs per arm, reported as
median and range (the project's within_margin rule: (b) may not be slower than (a) by more than (a)'s own range).
  (a) bbp_witness_batch + host toggle search + host row assembly + bbp_prove_batch + host assembly of the verify-rounds rows
  (b) bbp_prove_round
Cases N in {8, 202} x B in {64, 1024}, explicit entropy (the same rows for both arms), with the bytes each arm uploads.  Then, per
case, the device time (bbp_set_profiling, TAG_WITNESS) of k_round_bids + k_round_expand against k_prepare_bids for the same (B, N).
"""
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = 2 ** 252 + 27742317777372353535851937790883648493


def b32(x):
    return x.to_bytes(32, "little")


def make_case(ctx, N, B, rnd):
    """A round whose list holds the x of min(N, B) distinct bids; bid i is distinct bid i mod that count."""
    seed = b32(rnd.randrange(L))
    n = min(N, B)
    distinct = [(b32(rnd.getrandbits(64)), b32(rnd.randrange(L))) for _ in range(n)]
    w = ctx.witness_batch(b"".join(d + k + seed for d, k in distinct))
    items = [b32(rnd.randrange(L)) for _ in range(N)]
    for j, at in enumerate(rnd.sample(range(N), n)):
        items[at] = w[192 * j + 32:192 * j + 64]
    bids = [distinct[i % n] for i in range(B)]
    ent = b"".join(b"".join(os.urandom(31) + b"\0" for _ in range(4 + N)) + os.urandom(32) for _ in range(B))
    return seed, items, bids, ent


def arm_a(ctx, bbp, N, seed, items, bids, ent):
    B = len(bids)
    w = ctx.witness_batch(b"".join(d + k + seed for d, k in bids))
    where = {}
    for i in range(N - 1, -1, -1):  # lowest index wins; items as Scalar::from_bits values
        where[(int.from_bytes(items[i], "little") & ((1 << 255) - 1)) % L] = i
    lst = b"".join(items)
    rows, tails = [], []
    for i, (d, k) in enumerate(bids):
        m, x, y, yi, q, z = (w[192 * i + 32 * j:192 * i + 32 * j + 32] for j in range(6))
        rows.append(d + k + y + yi + q + z + seed + lst + where[int.from_bytes(x, "little")].to_bytes(8, "little"))
        tails.append(q + z)
    out, st = ctx.prove_batch(B, N, b"".join(rows), ent)
    rs_ = bbp.record_size(N)
    return b"".join(out[rs_ * i:rs_ * (i + 1)] + tails[i] for i in range(B)), st


def arm_b(ctx, bbp, N, seed, items, bids, ent):
    rows, _, st = ctx.prove_round(N, seed + b"".join(items), b"".join(d + k for d, k in bids), ent)
    return rows, st


def best_of(f, calls=5, warm=2):
    for _ in range(warm):
        f()
    best = None
    for _ in range(calls):
        t = time.perf_counter()
        f()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best * 1e3


def kernel_times(ctx, bbp, torch, N, seed, items, bids):
    """microseconds of the TAG_WITNESS launch of each pass (best of 5 after 2), same (B, N)"""
    B = len(bids)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    tab, rb = dev(seed + b"".join(items)), dev(b"".join(d + k for d, k in bids))
    pb, lists = dev(b"".join(d + k + seed for d, k in bids)), dev(b"".join(items) * B)
    tog = torch.zeros(B, dtype=torch.int64, device="cuda")
    pin = torch.zeros((7 * 32 + 32 * N + 8) * B, dtype=torch.uint8, device="cuda")
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {}
    for name, call in (("k_round_bids+k_round_expand", lambda: ctx.prepare_round_dev(N, tab.data_ptr(), B, rb.data_ptr(), pin.data_ptr(), st.data_ptr())),
                       ("k_prepare_bids", lambda: ctx.prepare_bids_dev(B, N, pb.data_ptr(), lists.data_ptr(), tog.data_ptr(), pin.data_ptr()))):
        ts = []
        for it in range(7):
            ctx.set_profiling(True)
            ctx.last_timings()
            call()
            t = [us for tag, us in ctx.last_timings() if tag == 3]
            ctx.set_profiling(False)
            assert len(t) == 1, t
            if it >= 2:
                ts.append(t[0])
        res[name] = round(min(ts), 1)
    return res


def main():
    out = sys.argv[1]
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    ctx = bbp.Context(0)
    rnd = random.Random(10)
    with open(out, "w") as f:
        for N in (8, 202):
            for B in (64, 1024):
                case = make_case(ctx, N, B, rnd)
                ra, sa = arm_a(ctx, bbp, N, *case)
                rb_, sb = arm_b(ctx, bbp, N, *case)
                assert sa == sb == [0] * B and ra == rb_, "the two arms disagree"
                runs = {"a": [], "b": []}
                for _ in range(5):
                    for arm, fn in (("a", arm_a), ("b", arm_b)):
                        runs[arm].append(best_of(lambda: fn(ctx, bbp, N, *case)))
                es = bbp.entropy_size(N)
                rec = {"N": N, "B": B, "unit": "ms per call, best of 5 after 2 warm-ups, 5 runs",
                       "upload_bytes": {"a": 96 * B + (7 * 32 + 32 * N + 8) * B + es * B, "b": 64 * B + 32 * (1 + N) + es * B}}
                for arm in ("a", "b"):
                    v = runs[arm]
                    rec[arm] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                rec["b_minus_a_ms"] = round(rec["b"]["median"] - rec["a"]["median"], 3)
                rec["within_margin"] = rec["b"]["median"] - rec["a"]["median"] <= rec["a"]["max"] - rec["a"]["min"]
                rec["kernel_us"] = kernel_times(ctx, bbp, torch, N, case[0], case[1], case[2])
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
