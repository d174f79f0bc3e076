#!/usr/bin/env python3
"""Mixed-N verification (bbp_verify_batch_mixed*) against what a caller does without it: sort the rows by N and make one
uniform call per distinct N.  One JSON line per case (B, N distribution, plain / aggregated, host / device-resident on one
verifier lane): best-of-`--steps` wall time of the mixed call and of the grouped calls, after `--warmup` runs of each.

    python tools/verify_mixed.py --out profiles/r06_verify_mixed.jsonl
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py)
import dusk_blindbidproof_amd as bbp  # noqa: E402

L = 2 ** 252 + 27742317777372353535851937790883648493
DISTS = {"uniform_1_202": lambda r: r.randint(1, 202), "four_values": lambda r: r.choice((8, 50, 120, 202))}


def sc(r):
    return (r.getrandbits(256) % L).to_bytes(32, "little")


def proofs_for(ctx, N, count, r):
    """`count` valid verify rows of list length N, proved by the engine."""
    dks = b"".join(r.getrandbits(64).to_bytes(8, "little") + bytes(24) + sc(r) + sc(r) for _ in range(count))
    w = ctx.witness_batch(dks)
    ins, tails = [], []
    for i in range(count):
        m, x, y, yi, q, z = (w[192 * i + 32 * j:192 * i + 32 * j + 32] for j in range(6))
        d, k, sd = dks[96 * i:96 * i + 32], dks[96 * i + 32:96 * i + 64], dks[96 * i + 64:96 * i + 96]
        pub = [sc(r) for _ in range(N)]
        pub[i % N] = x
        ins.append(d + k + y + yi + q + z + sd + b"".join(pub) + (i % N).to_bytes(8, "little"))
        tails.append(q + z + sd + b"".join(pub))
    out, st = ctx.prove_batch(count, N, b"".join(ins))
    assert st == [0] * count
    rs_ = bbp.record_size(N)
    return [out[i * rs_:(i + 1) * rs_] + tails[i] for i in range(count)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r06_verify_mixed.jsonl")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--per-n", type=int, default=16, help="distinct proofs per N; rows of the same N reuse them in turn")
    a = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    ctx = bbp.Context(0)
    lane = ctx.verify_stream(0)
    r = random.Random(606)
    lines = []
    for dist, draw in DISTS.items():
        Bmax = max(int(b) for b in a.batches.split(","))
        Ns_all = [draw(r) for _ in range(Bmax)]
        pool = {n: proofs_for(ctx, n, min(a.per_n, Ns_all.count(n)), r) for n in sorted(set(Ns_all))}
        used = {n: 0 for n in pool}
        rows_all = []
        for n in Ns_all:
            rows_all.append(pool[n][used[n] % len(pool[n])])
            used[n] += 1
        for B in (int(b) for b in a.batches.split(",")):
            Ns, rows = Ns_all[:B], rows_all[:B]
            blob = b"".join(rows)
            groups = {}
            for i, n in enumerate(Ns):
                groups.setdefault(n, []).append(i)
            gblobs = [(n, len(ix), b"".join(rows[i] for i in ix)) for n, ix in sorted(groups.items())]
            # device-resident copies: the mixed rows, and the same rows sorted into contiguous groups
            d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
            d_g = torch.frombuffer(bytearray(b"".join(g[2] for g in gblobs)), dtype=torch.uint8).to(dev)
            d_ent = torch.frombuffer(bytearray(os.urandom(32 * B)), dtype=torch.uint8).to(dev)
            d_st = torch.empty(B, dtype=torch.int32, device=dev)
            goff, o = [], 0
            for n, cnt, gb in gblobs:
                goff.append(o)
                o += len(gb)
            for mode in ("plain", "aggregated"):
                agg = mode == "aggregated"
                for path in ("host", "dev"):
                    if path == "host":
                        def mixed():
                            st = ctx.verify_batch_mixed_aggregated(Ns, blob)[0] if agg else ctx.verify_batch_mixed(Ns, blob)
                            assert st == [0] * B

                        def grouped():
                            for n, cnt, gb in gblobs:
                                st = ctx.verify_batch_aggregated(cnt, n, gb)[0] if agg else ctx.verify_batch(cnt, n, gb)
                                assert st == [0] * cnt
                    else:
                        def mixed():
                            if agg:
                                ctx.verify_batch_mixed_aggregated_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), d_st.data_ptr(), stream=lane,
                                                                      want_count=False)
                            else:
                                ctx.verify_batch_mixed_dev(Ns, d_in.data_ptr(), d_ent.data_ptr(), d_st.data_ptr(), stream=lane)

                        def grouped():
                            first = 0
                            for (n, cnt, gb), go in zip(gblobs, goff):
                                args = (cnt, n, d_g.data_ptr() + go, d_ent.data_ptr() + 32 * first, d_st.data_ptr() + 4 * first)
                                if agg:
                                    ctx.verify_batch_aggregated_dev(*args, stream=lane, want_count=False)
                                else:
                                    ctx.verify_batch_dev(*args, stream=lane)
                                first += cnt
                    tm = timed(mixed, a.warmup, a.steps)
                    if path == "dev":
                        assert d_st.cpu().tolist() == [0] * B
                    tg = timed(grouped, a.warmup, a.steps)
                    if path == "dev":
                        assert d_st.cpu().tolist() == [0] * B
                    line = {"B": B, "dist": dist, "distinct_n": len(groups), "mode": mode, "path": path, "mixed_ms": round(tm * 1e3, 3),
                            "grouped_ms": round(tg * 1e3, 3), "mixed_per_s": round(B / tm), "grouped_per_s": round(B / tg),
                            "speedup": round(tg / tm, 3), "steps": a.steps, "warmup": a.warmup}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
    assert ctx.health() == 0
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
