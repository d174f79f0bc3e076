#!/usr/bin/env python3
"""Rounds (bbp_verify_rounds*) against the existing calls on the expanded rows, in one process on one context.

    one round    R = 1, N in {8, 202}, B in {1024, 8192}: bbp_verify_rounds[_aggregated][_dev] against
                 bbp_verify_batch[_aggregated][_dev] on rows that carry seed || pub_list each
    catch-up     8192 rows over 202 rounds with N = 1..202: against bbp_verify_batch_mixed[_aggregated][_dev]

One JSON line per case (plain / aggregated, host / device-resident on one verifier lane).  A figure is the best of `--steps` wall
times after `--warmup` calls; `--runs` such figures per call, taken in turn (existing, rounds, existing, ...), give the median and
the range.  bytes_*: what the call uploads (rows, plus the round table once) -- the host forms copy them, the device forms read them.

    python tools/verify_rounds.py --out profiles/r08_verify_rounds.jsonl
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)
import dusk_blindbidproof_amd as bbp  # noqa: E402

L = 2 ** 252 + 27742317777372353535851937790883648493


def sc(r):
    return (r.getrandbits(256) % L).to_bytes(32, "little")


def make_round(ctx, N, count, r):
    """(seed, pub_list, [record || score || z_img]) with `count` <= N valid proofs of one round, proved by the engine."""
    seed = sc(r)
    dks = b"".join(r.getrandbits(64).to_bytes(8, "little") + bytes(24) + sc(r) + seed for _ in range(count))
    w = ctx.witness_batch(dks)
    wit = [[w[192 * i + 32 * j:192 * i + 32 * j + 32] for j in range(6)] for i in range(count)]
    pub = [sc(r) for _ in range(N)]
    for i in range(count):
        pub[i] = wit[i][1]
    pub = b"".join(pub)
    ins = b"".join(dks[96 * i:96 * i + 64] + wit[i][2] + wit[i][3] + wit[i][4] + wit[i][5] + seed + pub + i.to_bytes(8, "little") for i in range(count))
    out, st = ctx.prove_batch(count, N, ins)
    assert st == [0] * count
    rs_ = bbp.record_size(N)
    return seed, pub, [out[i * rs_:(i + 1) * rs_] + wit[i][4] + wit[i][5] for i in range(count)]


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def cbuf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(b)


def measure(ctx, lane, name, round_Ns, table, round_of, rows, a):
    """every mode and path of one case: round_of None = one round against the uniform calls, else against the mixed calls"""
    dev = torch.device("cuda", 0)
    lib, h = bbp.lib, ctx.handle
    R = len(round_Ns)
    Ns, blob = bbp.expand_round_rows(round_Ns, table, round_of, rows)
    B = len(Ns)
    u32 = ctypes.c_uint32
    c_rns, c_of, c_ns = (u32 * R)(*round_Ns), (None if round_of is None else (u32 * B)(*round_of)), (u32 * B)(*Ns)
    c_tab, c_rows, c_blob = cbuf(table), cbuf(rows), cbuf(blob)
    st = (ctypes.c_int32 * B)()
    put = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_tab, d_rows, d_blob, d_ent = put(table), put(rows), put(blob), put(os.urandom(32 * B))
    d_st = torch.empty(B, dtype=torch.int32, device=dev)
    p_tab, p_rows, p_blob, p_ent, p_st = (t.data_ptr() for t in (d_tab, d_rows, d_blob, d_ent, d_st))
    lines = []
    for mode in ("plain", "aggregated"):
        agg = mode == "aggregated"
        for path in ("host", "dev"):
            if path == "host":
                def rounds_call():
                    rc = (lib.bbp_verify_rounds_aggregated(h, R, c_rns, c_tab, B, c_of, c_rows, st, 0, None) if agg else
                          lib.bbp_verify_rounds(h, R, c_rns, c_tab, B, c_of, c_rows, st))
                    assert rc == 0

                def existing_call():
                    if round_of is None:
                        rc = (lib.bbp_verify_batch_aggregated(h, B, Ns[0], c_blob, st, 0, None) if agg else lib.bbp_verify_batch(h, B, Ns[0], c_blob, st))
                    else:
                        rc = (lib.bbp_verify_batch_mixed_aggregated(h, B, c_ns, c_blob, st, 0, None) if agg else
                              lib.bbp_verify_batch_mixed(h, B, c_ns, c_blob, st))
                    assert rc == 0
            else:
                def rounds_call():
                    rc = (lib.bbp_verify_rounds_aggregated_dev(h, R, c_rns, p_tab, B, c_of, p_rows, p_ent, p_st, 0, None, lane) if agg else
                          lib.bbp_verify_rounds_dev(h, R, c_rns, p_tab, B, c_of, p_rows, p_ent, p_st, lane))
                    assert rc == 0

                def existing_call():
                    if round_of is None:
                        rc = (lib.bbp_verify_batch_aggregated_dev(h, B, Ns[0], p_blob, p_ent, p_st, 0, None, lane) if agg else
                              lib.bbp_verify_batch_dev(h, B, Ns[0], p_blob, p_ent, p_st, lane))
                    else:
                        rc = (lib.bbp_verify_batch_mixed_aggregated_dev(h, B, c_ns, p_blob, p_ent, p_st, 0, None, lane) if agg else
                              lib.bbp_verify_batch_mixed_dev(h, B, c_ns, p_blob, p_ent, p_st, lane))
                    assert rc == 0

            def check():
                torch.cuda.synchronize()
                assert (list(st) if path == "host" else d_st.cpu().tolist()) == [0] * B
            te, tr = [], []
            for _ in range(a.runs):
                te.append(timed(existing_call, a.warmup, a.steps) * 1e3)
                check()
                tr.append(timed(rounds_call, a.warmup, a.steps) * 1e3)
                check()
            me, mr = statistics.median(te), statistics.median(tr)
            line = {"case": name, "B": B, "R": R, "N": round_Ns[0] if R == 1 else "1..%d" % max(round_Ns), "mode": mode, "path": path,
                    "existing": "verify_batch" if round_of is None else "verify_batch_mixed",
                    "existing_ms": round(me, 3), "existing_range_ms": [round(min(te), 3), round(max(te), 3)],
                    "rounds_ms": round(mr, 3), "rounds_range_ms": [round(min(tr), 3), round(max(tr), 3)],
                    "speedup": round(me / mr, 3), "margin_ms": round(max(te) - min(te), 3), "within_margin": mr <= me + (max(te) - min(te)),
                    "bytes_existing": len(blob), "bytes_rounds": len(rows) + len(table), "bytes_share": round((len(rows) + len(table)) / len(blob), 3),
                    "runs": a.runs, "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r08_verify_rounds.jsonl")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--items", default="8,202")
    ap.add_argument("--catchup", type=int, default=8192, help="rows of the catch-up case (0 = skip it)")
    ap.add_argument("--catchup-rounds", type=int, default=202, help="its rounds: N = 1..this")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = bbp.Context(0)
    lane = ctx.verify_stream(0)
    r = random.Random(808)
    lines = []
    for N in (int(n) for n in a.items.split(",")):
        seed, pub, proofs = make_round(ctx, N, min(N, 8), r)
        for B in (int(b) for b in a.batches.split(",")):
            rows = b"".join(proofs[i % len(proofs)] for i in range(B))
            lines += measure(ctx, lane, "one_round", [N], seed + pub, None, rows, a)
    if a.catchup:
        made = [make_round(ctx, n, min(n, 2), r) for n in range(1, a.catchup_rounds + 1)]
        round_Ns, table = bbp.pack_rounds([(m[0], m[1]) for m in made])
        round_of = [i % len(made) for i in range(a.catchup)]
        r.shuffle(round_of)
        used = [0] * len(made)
        parts = []
        for ro in round_of:
            parts.append(made[ro][2][used[ro] % len(made[ro][2])])
            used[ro] += 1
        lines += measure(ctx, lane, "catch_up", round_Ns, table, round_of, b"".join(parts), a)
    assert ctx.health() == 0
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
