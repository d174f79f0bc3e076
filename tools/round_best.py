"""What finding a round's best valid proof costs on one MI355X (include/bbp.h "Best valid proofs of a round"; DESIGN.md has the figures).
One JSON line per cell, to stdout and to --out (default profiles/r19_round_best.jsonl) with the box id and --commit.

  cells   shapes (N, B) = (8, 8192), (202, 8192), (8, 65536); traffic: every row honest / the top 1 % by claimed score forged / the top
          25 % forged / every row forged (a forged row is a valid row with one record byte flipped: it keeps its claim and fails).
          Arm A: bbp_verify_round_best with K = 1 and the default tranche, and its _dev form on resident rows.  Arm B, the route a caller
          had before: bbp_verify_rounds_aggregated (or its _dev form, in calls of at most 32 768 rows) over all rows, then the pick on the
          host.  Per cell: ms per call for the four arms, rows examined and tranches (asserted equal to what the rules predict), bytes
          uploaded by the host forms, A / B.
  sweep   tranche in {16, 64, 256, 1024} on the honest and the 25 % traffic at B = 8192, host form: what picks BBP_BEST_TRANCHE_DEFAULT.

  --distinct OUT   instead of the above: bbp_verify_round_best_distinct ("Best proofs of a round, one per bidder") at N = 8 / 202,
          B = 8192, K = 4, default tranche, into OUT (profiles/r20_round_best_distinct.jsonl).  Traffic: (a) every bidder once at the top,
          the rest of the rows claiming scores below them; (b) a flood: the top bidder's row 8000 times (byte-equal), the others once;
          (c) the flood with the top 1 % by claimed score forged.  Arms: the new call (host, dev), the existing call (host, dev: under a
          flood its answer holds one bidder K times -- here for cost only), bbp_verify_rounds_aggregated over everything with a
          de-duplicating pick on the host.  Rows examined and dropped are asserted equal to the model of
          tests/round_best_distinct_cases.py on the verdicts of the third arm; the tranche count is the model's.  Also traffic (a)
          with K = 1, new call against existing call in the same run.

  --rounds OUT   instead of the above: bbp_verify_rounds_best ("Best valid proofs of many rounds") on 8192 rows over 202 rounds (row i in
          round i mod 202), every round at N = 8, and rounds cycling through N = 8, 50, 120, 202; K = 1, tranche 16, into OUT
          (profiles/r22_rounds_best.jsonl).  Traffic: honest / the top 1 % of each round (at least one row) forged / all forged.  Arms:
          A the new call (host, dev); B a loop of bbp_verify_round_best calls, one per round (host, dev); C
          bbp_verify_rounds_aggregated over everything, then the pick per round on the host.  Rows examined and steps are asserted
          equal to what the rules predict; the three arms must name the same winners.  Rounds of one length reuse one proved table.

  --rounds-distinct OUT   instead of the above: bbp_verify_rounds_best_distinct ("Best proofs of many rounds, one per bidder") on 8192
          rows over 202 rounds (the --rounds shape: row i in round i mod 202), K = 3, tranche 16, into OUT
          (profiles/r23_rounds_best_distinct.jsonl).  Every round holds 40 or 41 bidders, so every round is at N = 50: a list of 8 items
          holds 8 bids.  Traffic: no duplicates / a flood: each round's best bidder resent eight times (byte-equal, in place
          of the round's eight lowest claims) / a forged flood: those eight copies claim a raised score and fail.  Arms: the new call
          (host, dev); one bbp_verify_round_best_distinct per round; the plain bbp_verify_rounds_best (under a flood its answer holds
          the copies: here for cost); bbp_verify_rounds_aggregated over everything with a de-duplicating pick per round on the host.
          The new call's outputs are asserted equal to the model of tests/rounds_best_distinct_cases.py on the verdicts of the last
          arm, and to the loop's; without duplicates it must examine exactly the rows the plain call examines.

  --standing [OUT]   instead of the above: a standing ("Standing of a round") of one round at N = 50, K = 3, default tranche; 8192 rows
          arrive as 32 offers of 256, into OUT (profiles/r24_round_standing.jsonl).  Traffic: every valid row sent once / the second half of
          every offer resends earlier rows / a forged flood on top (16 rows per offer under the best bidder's z_img and a forged score).
          Arms: offers to a standing; bbp_verify_round_best_distinct over all rows so far after each burst; the same call on each burst
          alone.  Per arm ms per burst, bytes uploaded, rows verified; every output of every offer is asserted equal to the model of
          tests/round_standing_cases.py.

  --standings [OUT]   instead of the above: one offer to many standings ("Standings of many rounds"): 64 standings at N = 50, K = 3,
          default tranche; 8192 rows arrive as 32 bursts of 256, every burst carrying 4 rows of each of the 64 rounds, interleaved, the
          second half of a round's rows of a burst resending earlier ones, into OUT (profiles/r25_standings.jsonl).  Arms: (a) one
          bbp_standings_offer per burst; (b) one bbp_standing_offer per standing per burst.  Per arm ms per burst, rows verified, bytes
          uploaded; every output of arm (a) is asserted equal to the model of tests/standings_cases.py, and the two arms must leave equal
          standings.

Rows are 64 proved bids of the round repeated (byte-equal rows do occur in the protocol too); arms alternate in one process; every figure
is the best of --calls calls, taken --runs times after a warm-up: median and range."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab import box_id  # noqa: E402

T_X = 257  # byte offset of t_x in a record
DEV_CALL_ROWS = 32768
TRAFFIC = (("honest", 0.0), ("top_1pct_forged", 0.01), ("top_25pct_forged", 0.25), ("all_forged", 1.0))


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def predict(n_candidates, forged, K, tranche):
    """(rows examined, tranches) by the rules when the first `forged` candidates in the candidate order fail and the rest hold"""
    T, at, t = max(tranche, K), 0, 0
    while at < n_candidates:
        at, T, t = min(at + T, n_candidates), 2 * T, t + 1
        if at - min(at, forged) >= K:
            break
    return at, t


class Cell:
    """one shape and traffic: the rows on the host (a ctypes buffer) and on the device, what every arm must answer"""

    def __init__(self, torch, bbp, np, N, B, base_rows, table, frac):
        row = bbp.round_row_size(N)
        n_base = len(base_rows) // row
        rows = bytearray(base_rows * (B // n_base))
        key_off = bbp.record_size(N)
        keys = np.frombuffer(bytes(rows), dtype=np.uint8).reshape(B, row)[:, key_off:key_off + 32].copy().view("<u8")  # B x 4 words
        idx = np.arange(B)
        self.order = np.lexsort((idx, ~keys[:, 0], ~keys[:, 1], ~keys[:, 2], ~keys[:, 3]))  # key descending, index ascending
        self.forged = int(round(frac * B))
        for i in self.order[:self.forged].tolist():
            rows[row * i + T_X] ^= 0x01
        self.N, self.B, self.row, self.keys = N, B, row, keys
        self.best = int(self.order[self.forged]) if self.forged < B else None
        self.host = (ctypes.c_uint8 * len(rows)).from_buffer(rows)
        self.table = (ctypes.c_uint8 * len(table)).from_buffer_copy(table)
        self.d_rows = torch.frombuffer(rows, dtype=torch.uint8).cuda()
        self.d_table = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
        self.d_ent = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, device="cuda")
        self.d_status = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
        self.status = (ctypes.c_int32 * B)()
        self.floor = (ctypes.c_uint8 * 32)()


def make_arms(ctx, bbp, torch, np, c, tranche):
    lib, h = bbp.lib, ctx.handle
    best, n = (ctypes.c_uint32 * 1)(), [ctypes.c_uint32() for _ in range(3)]
    nfb = ctypes.c_uint32()
    Ns = (ctypes.c_uint32 * 1)(c.N)
    stream = torch.cuda.Stream()

    def answer():
        return (best[0] if n[0].value else None, n[0].value, n[1].value, n[2].value)

    def a_host():
        rc = lib.bbp_verify_round_best(h, c.N, c.table, c.B, c.host, c.floor, 1, tranche, 1, best, ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]),
                                       c.status)
        assert rc == 0, (rc, lib.bbp_last_error(h))
        return answer()

    def a_dev():
        rc = lib.bbp_verify_round_best_dev(h, c.N, c.d_table.data_ptr(), c.B, c.d_rows.data_ptr(), c.d_ent.data_ptr(), c.floor, 1, tranche, 1, best,
                                           ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]), c.d_status.data_ptr(), stream.cuda_stream)
        assert rc == 0, (rc, lib.bbp_last_error(h))
        stream.synchronize()
        return answer()

    def pick(status):
        ok = np.nonzero(status == 0)[0]
        if not len(ok):
            return None
        k = c.keys[ok]
        return int(ok[np.lexsort((ok, ~k[:, 0], ~k[:, 1], ~k[:, 2], ~k[:, 3]))[0]])

    def b_host():
        rc = lib.bbp_verify_rounds_aggregated(h, 1, Ns, c.table, c.B, None, c.host, c.status, 0, ctypes.byref(nfb))
        assert rc == 0, (rc, lib.bbp_last_error(h))
        return (pick(np.frombuffer(c.status, dtype="<i4")),)

    def b_dev():  # in calls of at most 32 768 rows, the size of a host-pointer call's engine calls (BBP_HOST_CHUNK_VERIFY)
        for first in range(0, c.B, DEV_CALL_ROWS):
            m = min(DEV_CALL_ROWS, c.B - first)
            rc = lib.bbp_verify_rounds_aggregated_dev(h, 1, Ns, c.d_table.data_ptr(), m, None, c.d_rows.data_ptr() + c.row * first,
                                                      c.d_ent.data_ptr() + 32 * first, c.d_status.data_ptr() + 4 * first, 0, None, stream.cuda_stream)
            assert rc == 0, (rc, lib.bbp_last_error(h))
        stream.synchronize()
        return (pick(c.d_status.cpu().numpy().view("<i4")),)
    return {"best_host": a_host, "best_dev": a_dev, "all_then_pick_host": b_host, "all_then_pick_dev": b_dev}


def timed(arms, names, args):
    for name in names:  # the warm-up, and the answers
        arms[name]()
    runs = {name: [] for name in names}
    for _ in range(args.runs):
        for name in names:
            best = None
            for _c in range(args.calls):
                t = time.perf_counter()
                arms[name]()
                dt = (time.perf_counter() - t) * 1e3
                best = dt if best is None else min(best, dt)
            runs[name].append(best)
    return {name: stats(v) for name, v in runs.items()}


def model_tranches(dc, keys, ids, verdicts, K, tranche):
    """the number of tranches the model of tests/round_best_distinct_cases.py runs (its loop, counting)"""
    live = sorted(range(len(keys)), key=lambda i: (-keys[i], i))
    T, settled, t = (max(tranche or 16, K) if K else len(live)), set(), 0
    while live:
        batch, live, T, t = live[:T], live[T:], 2 * T, t + 1
        settled |= {ids[i] for i in batch if verdicts[i] == 0}
        if K and len(settled) >= K:
            break
        live = [i for i in live if ids[i] not in settled]
    return t


def distinct_traffic(bbp, N, B, base_rows, kind):
    """B rows as a bytearray: one row per bidder of base_rows (by z_img), then what `kind` says, then rows that claim scores below all"""
    row = bbp.round_row_size(N)
    key_off = bbp.record_size(N)
    seen, uniq = set(), []
    for i in range(len(base_rows) // row):
        r = base_rows[row * i:row * (i + 1)]
        if r[-32:] not in seen:
            seen.add(r[-32:])
            uniq.append(r)
    uniq.sort(key=lambda r: -int.from_bytes(r[key_off:key_off + 32], "little"))
    rows = list(uniq)
    if kind != "no_duplicates":
        rows += [uniq[0]] * (8000 - 1)
    n_real = len(rows)
    for i in range(B - n_real):  # the rest: a bidder's row under a claimed score below every real one (fails if it is ever verified)
        r = uniq[i % len(uniq)]
        rows.append(r[:key_off] + (i + 1).to_bytes(32, "little") + r[key_off + 32:])
    if kind == "flood_top_1pct_forged":
        order = sorted(range(B), key=lambda i: (-int.from_bytes(rows[i][key_off:key_off + 32], "little"), i))
        for i in order[:B // 100]:
            b = bytearray(rows[i])
            b[T_X] ^= 0x01
            rows[i] = bytes(b)
    keys = [int.from_bytes(r[key_off:key_off + 32], "little") for r in rows]
    ids = [r[-32:] for r in rows]
    return bytearray(b"".join(rows)), keys, ids


def distinct_main(args):
    import numpy as np
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    from tests import round_best_distinct_cases as dc
    box = box_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.distinct)), exist_ok=True)
    B = 8192
    unit = "ms of host time per call, best of %d, %d runs after a warm-up" % (args.calls, args.runs)
    with open(args.distinct, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        lib, h = bbp.lib, ctx.handle
        try:
            for N in (8, 202):
                r = rc.honest(N, 64, tag=20)
                base_rows, _t, st = ctx.prove_round(N, r.table, r.bid_bytes)
                assert st == [0] * 64
                row = bbp.round_row_size(N)
                table = (ctypes.c_uint8 * len(r.table)).from_buffer_copy(r.table)
                d_table = torch.frombuffer(bytearray(r.table), dtype=torch.uint8).cuda()
                Ns = (ctypes.c_uint32 * 1)(N)
                floor = (ctypes.c_uint8 * 32)()
                stream = torch.cuda.Stream()
                for kind, Ks in (("no_duplicates", (4, 1)), ("flood", (4,)), ("flood_top_1pct_forged", (4,))):
                    rows, keys, ids = distinct_traffic(bbp, N, B, base_rows, kind)
                    host = (ctypes.c_uint8 * len(rows)).from_buffer(rows)
                    d_rows = torch.frombuffer(rows, dtype=torch.uint8).cuda()
                    d_ent = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, device="cuda")
                    d_status = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
                    status = (ctypes.c_int32 * B)()
                    nfb = ctypes.c_uint32()
                    rc_ = lib.bbp_verify_rounds_aggregated(h, 1, Ns, table, B, None, host, status, 0, ctypes.byref(nfb))
                    assert rc_ == 0
                    verdicts = list(status)
                    for K in Ks:
                        best = (ctypes.c_uint32 * K)()
                        n = [ctypes.c_uint32() for _ in range(4)]
                        p = [ctypes.byref(x) for x in n]

                        def new_host():
                            assert lib.bbp_verify_round_best_distinct(h, N, table, B, host, floor, K, 0, K, best, p[0], p[1], p[2], p[3], status) == 0
                            return list(best)[:n[0].value], n[0].value, n[1].value, n[2].value, n[3].value

                        def new_dev():
                            assert lib.bbp_verify_round_best_distinct_dev(h, N, d_table.data_ptr(), B, d_rows.data_ptr(), d_ent.data_ptr(), floor, K, 0, K, best,
                                                                          p[0], p[1], p[2], p[3], d_status.data_ptr(), stream.cuda_stream) == 0
                            stream.synchronize()
                            return list(best)[:n[0].value], n[0].value, n[1].value, n[2].value, n[3].value

                        def old_host():
                            assert lib.bbp_verify_round_best(h, N, table, B, host, floor, K, 0, K, best, p[0], p[1], p[2], status) == 0
                            return list(best)[:n[0].value]

                        def old_dev():
                            assert lib.bbp_verify_round_best_dev(h, N, d_table.data_ptr(), B, d_rows.data_ptr(), d_ent.data_ptr(), floor, K, 0, K, best, p[0], p[1],
                                                                 p[2], d_status.data_ptr(), stream.cuda_stream) == 0
                            stream.synchronize()
                            return list(best)[:n[0].value]

                        def all_then_pick():
                            assert lib.bbp_verify_rounds_aggregated(h, 1, Ns, table, B, None, host, status, 0, ctypes.byref(nfb)) == 0
                            ok = np.nonzero(np.frombuffer(status, dtype="<i4") == 0)[0].tolist()
                            ok.sort(key=lambda i: (-keys[i], i))
                            seen, out = set(), []
                            for i in ok:
                                if ids[i] not in seen:
                                    seen.add(ids[i])
                                    out.append(i)
                                    if len(out) == K:
                                        break
                            return out
                        arms = {"distinct_host": new_host, "distinct_dev": new_dev, "existing_host": old_host, "existing_dev": old_dev,
                                "all_then_dedup_pick_host": all_then_pick}
                        want = dc.model(keys, ids, verdicts, 0, K, 0)
                        assert new_host() == want[:5] and new_dev() == want[:5], (new_host(), want[:5])  # nothing here is tuned: the model predicts it
                        assert all_then_pick() == want[0]
                        old = old_host()
                        rec = {"section": "distinct", "N": N, "B": B, "traffic": kind, "K": K, "tranche": bbp.BEST_TRANCHE_DEFAULT, "bidders": len(set(ids)),
                               "rows_examined": want[3], "rows_dropped": want[4], "tranches": model_tranches(dc, keys, ids, verdicts, K, 0),
                               "existing_call_distinct_bidders_in_best": len({ids[i] for i in old}), "unit": unit}
                        rec.update(timed(arms, list(arms), args))
                        for form in ("host", "dev"):
                            a, b = rec["distinct_" + form], rec["existing_" + form]
                            rec["distinct_over_existing_" + form] = round(a["median"] / b["median"], 4)
                            rec["distinct_above_existing_range_by_ms_" + form] = round(max(0.0, a["median"] - b["max"]), 3)
                        emit(rec)
            assert ctx.health() == 0
        finally:
            ctx.close()


FOUR_LENGTHS = (8, 50, 120, 202)  # tools/verify_combine.py's four_values


def rounds_main(args):
    """--rounds: bbp_verify_rounds_best against the two routes a caller had before, 8192 rows over 202 rounds"""
    import numpy as np
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    box = box_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.rounds)), exist_ok=True)
    B, R, K, tranche, n_base = 8192, 202, 1, 16, 16
    unit = "ms of host time per call, best of %d, %d runs after a warm-up" % (args.calls, args.runs)
    with open(args.rounds, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        lib, h = bbp.lib, ctx.handle
        try:
            base = {}
            for N in sorted(set(FOUR_LENGTHS)):
                r = rc.honest(N, n_base, tag=22)
                rows, _t, st = ctx.prove_round(N, r.table, r.bid_bytes)
                assert st == [0] * n_base
                size = bbp.round_row_size(N)
                base[N] = ([rows[size * i:size * (i + 1)] for i in range(n_base)], r.table)
            stream = torch.cuda.Stream()
            for mix, lengths in (("n8", (8,)), ("four_lengths", FOUR_LENGTHS)):
                Ns = [lengths[r % len(lengths)] for r in range(R)]  # (rounds of one length share the table's bytes: the cost is the same)
                table = b"".join(base[N][1] for N in Ns)
                round_of = [i % R for i in range(B)]
                members = [[i for i in range(B) if i % R == r] for r in range(R)]
                for tname, frac in (("honest", 0.0), ("top_1pct_of_each_round_forged", 0.01), ("all_forged", 1.0)):
                    row_list = [base[Ns[i % R]][0][(i // R) % n_base] for i in range(B)]
                    key_off = [bbp.record_size(Ns[i % R]) for i in range(B)]
                    keys = [int.from_bytes(row_list[i][key_off[i]:key_off[i] + 32], "little") for i in range(B)]
                    order = [sorted(m, key=lambda i: (-keys[i], i)) for m in members]
                    forged = [0 if frac == 0 else max(1, int(round(frac * len(m)))) for m in members]
                    for r in range(R):
                        for i in order[r][:forged[r]]:
                            b = bytearray(row_list[i])
                            b[T_X] ^= 0x01
                            row_list[i] = bytes(b)
                    want_best = [order[r][forged[r]] if forged[r] < len(order[r]) else None for r in range(R)]
                    pred = [predict(len(members[r]), forged[r], K, tranche) for r in range(R)]
                    rows = bytearray(b"".join(row_list))
                    c_rows = (ctypes.c_uint8 * len(rows)).from_buffer(rows)
                    c_table = (ctypes.c_uint8 * len(table)).from_buffer_copy(table)
                    c_ns, c_ro = (ctypes.c_uint32 * R)(*Ns), (ctypes.c_uint32 * B)(*round_of)
                    d_rows = torch.frombuffer(rows, dtype=torch.uint8).cuda()
                    d_table = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
                    d_ent = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, device="cuda")
                    d_status = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
                    status = (ctypes.c_int32 * B)()
                    best, nb, nc, ne = ((ctypes.c_uint32 * R)() for _ in range(4))
                    steps, nfb = ctypes.c_uint32(), ctypes.c_uint32()
                    floor = (ctypes.c_uint8 * 32)()
                    # arm B's inputs: every round's rows and table on their own, host and device
                    per = []
                    for r in range(R):
                        blob = bytearray(b"".join(row_list[i] for i in members[r]))
                        tab = base[Ns[r]][1]
                        per.append(((ctypes.c_uint8 * len(blob)).from_buffer(blob), (ctypes.c_uint8 * len(tab)).from_buffer_copy(tab),
                                    torch.frombuffer(blob, dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda(),
                                    (ctypes.c_int32 * len(members[r]))()))
                    one, n3 = (ctypes.c_uint32 * 1)(), [ctypes.c_uint32() for _ in range(3)]
                    p3 = [ctypes.byref(x) for x in n3]

                    def answer():
                        return [best[r] if nb[r] else None for r in range(R)], list(ne), steps.value

                    def a_host():
                        rc_ = lib.bbp_verify_rounds_best(h, R, c_ns, c_table, B, c_ro, c_rows, None, K, tranche, 1, best, nb, nc, ne, ctypes.byref(steps), status)
                        assert rc_ == 0, (rc_, lib.bbp_last_error(h))
                        return answer()

                    def a_dev():
                        rc_ = lib.bbp_verify_rounds_best_dev(h, R, c_ns, d_table.data_ptr(), B, c_ro, d_rows.data_ptr(), d_ent.data_ptr(), None, K, tranche, 1, best,
                                                             nb, nc, ne, ctypes.byref(steps), d_status.data_ptr(), stream.cuda_stream)
                        assert rc_ == 0, (rc_, lib.bbp_last_error(h))
                        stream.synchronize()
                        return answer()

                    def b_host():
                        out, exam = [], []
                        for r in range(R):
                            hb, ht, _db, _dt, st_ = per[r]
                            assert lib.bbp_verify_round_best(h, Ns[r], ht, len(members[r]), hb, floor, K, tranche, 1, one, p3[0], p3[1], p3[2], st_) == 0
                            out.append(members[r][one[0]] if n3[0].value else None)
                            exam.append(n3[2].value)
                        return out, exam

                    def b_dev():
                        out, exam = [], []
                        for r in range(R):
                            _hb, _ht, db, dt, _st = per[r]
                            assert lib.bbp_verify_round_best_dev(h, Ns[r], dt.data_ptr(), len(members[r]), db.data_ptr(), d_ent.data_ptr(), floor, K, tranche, 1, one,
                                                                 p3[0], p3[1], p3[2], d_status.data_ptr(), stream.cuda_stream) == 0
                            out.append(members[r][one[0]] if n3[0].value else None)
                            exam.append(n3[2].value)
                        stream.synchronize()
                        return out, exam

                    def c_host():
                        assert lib.bbp_verify_rounds_aggregated(h, R, c_ns, c_table, B, c_ro, c_rows, status, 0, ctypes.byref(nfb)) == 0
                        st_ = np.frombuffer(status, dtype="<i4")
                        return [next((i for i in order[r] if st_[i] == 0), None) for r in range(R)]
                    arms = {"rounds_best_host": a_host, "rounds_best_dev": a_dev, "loop_of_round_best_host": b_host, "loop_of_round_best_dev": b_dev,
                            "all_then_pick_host": c_host}
                    want = (want_best, [p[0] for p in pred], max(p[1] for p in pred))
                    assert a_host() == want and a_dev() == want, (a_host()[1:], want[1:])  # nothing here is tuned: the rules predict it
                    assert b_host() == want[:2] and b_dev() == want[:2] and c_host() == want_best
                    examined = sum(want[1])
                    row_bytes = [len(x) for x in row_list]
                    up_rows = sum(row_bytes[i] + 32 + 4 for r in range(R) for i in order[r][:pred[r][0]])
                    rec = {"section": "rounds", "mix": mix, "B": B, "R": R, "traffic": tname, "K": K, "tranche": tranche, "rows_examined": examined,
                           "steps": want[2], "tranches_of_the_loop": sum(p[1] for p in pred), "unit": unit}
                    rec.update(timed(arms, list(arms), args))
                    rec["bytes_uploaded"] = {"rounds_best_host": 32 * B + 4 * B + up_rows + want[2] * len(table),
                                             "loop_of_round_best_host": 32 * B + up_rows + sum(pred[r][1] * 32 * (1 + Ns[r]) for r in range(R)),
                                             "all_then_pick_host": sum(row_bytes) + 32 * B + len(table)}
                    for form in ("host", "dev"):
                        a, b = rec["rounds_best_" + form], rec["loop_of_round_best_" + form]
                        rec["A_over_B_" + form] = round(a["median"] / b["median"], 4)
                        rec["A_beats_B_by_more_than_B_range_" + form] = b["median"] - a["median"] > b["max"] - b["min"]
                    a, cc = rec["rounds_best_host"], rec["all_then_pick_host"]
                    rec["A_over_C_host"] = round(a["median"] / cc["median"], 4)
                    rec["A_beats_C_by_more_than_C_range_host"] = cc["median"] - a["median"] > cc["max"] - cc["min"]
                    emit(rec)
            assert ctx.health() == 0
        finally:
            ctx.close()


def rounds_distinct_main(args):
    """--rounds-distinct: bbp_verify_rounds_best_distinct against the three routes a caller had before, 8192 rows over 202 rounds"""
    import numpy as np
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    from tests import rounds_best_distinct_cases as mdc
    box = box_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.rounds_distinct)), exist_ok=True)
    B, R, K, tranche, N, n_base, copies = 8192, 202, 3, 16, 50, 41, 8
    L = mdc.L
    unit = "ms of host time per call, best of %d, %d runs after a warm-up" % (args.calls, args.runs)
    with open(args.rounds_distinct, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        lib, h = bbp.lib, ctx.handle
        try:
            r0 = rc.honest(N, n_base, tag=23)
            proved, _t, st = ctx.prove_round(N, r0.table, r0.bid_bytes)
            assert st == [0] * n_base
            size, key_off = bbp.round_row_size(N), bbp.record_size(N)
            base = [proved[size * i:size * (i + 1)] for i in range(n_base)]
            assert len({x[-32:] for x in base}) == n_base  # every bid a bidder of its own
            score = lambda x: int.from_bytes(x[key_off:key_off + 32], "little")
            Ns, table = [N] * R, r0.table * R  # (the rounds share the table's bytes: identities belong to a round all the same)
            round_of = [i % R for i in range(B)]
            members = [[i for i in range(B) if i % R == r] for r in range(R)]
            stream = torch.cuda.Stream()
            for tname in ("no_duplicates", "flood", "forged_flood"):
                row_list = [base[i // R] for i in range(B)]
                for r in range(R):
                    order = sorted(members[r], key=lambda i: (-score(row_list[i]), i))
                    if tname != "no_duplicates":
                        top = row_list[order[0]]
                        if tname == "forged_flood":
                            top = top[:key_off] + (L - 1).to_bytes(32, "little") + top[key_off + 32:]
                        for i in order[-copies:]:
                            row_list[i] = top
                keys, ids = [score(x) for x in row_list], [x[-32:] for x in row_list]
                rows = bytearray(b"".join(row_list))
                c_rows = (ctypes.c_uint8 * len(rows)).from_buffer(rows)
                c_table = (ctypes.c_uint8 * len(table)).from_buffer_copy(table)
                c_ns, c_ro = (ctypes.c_uint32 * R)(*Ns), (ctypes.c_uint32 * B)(*round_of)
                d_rows = torch.frombuffer(rows, dtype=torch.uint8).cuda()
                d_table = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
                d_ent = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, device="cuda")
                d_status = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
                status = (ctypes.c_int32 * B)()
                best = (ctypes.c_uint32 * (R * K))()
                nb, nc, ne, nd = ((ctypes.c_uint32 * R)() for _ in range(4))
                steps, nfb = ctypes.c_uint32(), ctypes.c_uint32()
                floor = (ctypes.c_uint8 * 32)()
                per = []
                for r in range(R):
                    blob = bytearray(b"".join(row_list[i] for i in members[r]))
                    per.append(((ctypes.c_uint8 * len(blob)).from_buffer(blob), (ctypes.c_uint8 * len(r0.table)).from_buffer_copy(r0.table),
                                (ctypes.c_int32 * len(members[r]))()))
                k3, n4 = (ctypes.c_uint32 * K)(), [ctypes.c_uint32() for _ in range(4)]
                p4 = [ctypes.byref(x) for x in n4]

                def answer(dups=True):
                    return [list(best[r * K:r * K + min(nb[r], K)]) for r in range(R)], list(ne), list(nd) if dups else None, steps.value

                def new_host():
                    rc_ = lib.bbp_verify_rounds_best_distinct(h, R, c_ns, c_table, B, c_ro, c_rows, None, K, tranche, K, best, nb, nc, ne, nd, ctypes.byref(steps),
                                                              status)
                    assert rc_ == 0, (rc_, lib.bbp_last_error(h))
                    return answer()

                def new_dev():
                    rc_ = lib.bbp_verify_rounds_best_distinct_dev(h, R, c_ns, d_table.data_ptr(), B, c_ro, d_rows.data_ptr(), d_ent.data_ptr(), None, K, tranche,
                                                                  K, best, nb, nc, ne, nd, ctypes.byref(steps), d_status.data_ptr(), stream.cuda_stream)
                    assert rc_ == 0, (rc_, lib.bbp_last_error(h))
                    stream.synchronize()
                    return answer()

                def loop_host():
                    out, exam, dups = [], [], []
                    for r in range(R):
                        hb, ht, st_ = per[r]
                        assert lib.bbp_verify_round_best_distinct(h, N, ht, len(members[r]), hb, floor, K, tranche, K, k3, p4[0], p4[1], p4[2], p4[3], st_) == 0
                        out.append([members[r][k3[j]] for j in range(min(n4[0].value, K))])
                        exam.append(n4[2].value), dups.append(n4[3].value)
                    return out, exam, dups

                def plain_host():
                    rc_ = lib.bbp_verify_rounds_best(h, R, c_ns, c_table, B, c_ro, c_rows, None, K, tranche, K, best, nb, nc, ne, ctypes.byref(steps), status)
                    assert rc_ == 0, (rc_, lib.bbp_last_error(h))
                    return answer(dups=False)

                def all_host():
                    assert lib.bbp_verify_rounds_aggregated(h, R, c_ns, c_table, B, c_ro, c_rows, status, 0, ctypes.byref(nfb)) == 0
                    st_ = np.frombuffer(status, dtype="<i4")
                    out = []
                    for r in range(R):
                        seen, mine = set(), []
                        for i in sorted(members[r], key=lambda i: (-keys[i], i)):
                            if st_[i] == 0 and ids[i] not in seen:
                                seen.add(ids[i]), mine.append(i)
                        out.append(mine[:K])
                    return out
                picked = all_host()
                verdicts = [int(v) for v in np.frombuffer(status, dtype="<i4")]
                w_best, _nb, _nc, w_exam, w_dups, w_steps, _st, ran = mdc.model(R, round_of, keys, ids, verdicts, None, K, tranche)
                want = (w_best, w_exam, w_dups, w_steps)
                assert new_host() == want and new_dev() == want, (new_host()[1:], want[1:])  # nothing here is tuned: the rules predict it
                assert loop_host() == want[:3] and picked == w_best
                p_best, p_exam, _none, p_steps = plain_host()
                if tname == "no_duplicates":
                    assert p_exam == w_exam and p_best == w_best and p_steps == w_steps  # exactly the rows the plain call examines
                copies_in_plain = sum(len({ids[i] for i in b}) < len(b) for b in p_best)
                arms = {"rounds_best_distinct_host": new_host, "rounds_best_distinct_dev": new_dev, "loop_of_round_best_distinct_host": loop_host,
                        "rounds_best_host": plain_host, "all_then_pick_host": all_host}
                rec = {"section": "rounds_distinct", "B": B, "R": R, "N": N, "traffic": tname, "K": K, "tranche": tranche, "rows_examined": sum(w_exam),
                       "rows_dropped": sum(w_dups), "steps": w_steps, "tranches_of_the_loop": sum(ran), "rows_examined_by_rounds_best": sum(p_exam),
                       "rounds_where_rounds_best_returns_copies": copies_in_plain, "unit": unit}
                rec.update(timed(arms, list(arms), args))
                tab = 32 * (1 + N)
                rec["bytes_uploaded"] = {"rounds_best_distinct_host": 64 * B + 4 * B + sum(w_exam) * (size + 32 + 4) + w_steps * len(table),
                                         "loop_of_round_best_distinct_host": 64 * B + sum(w_exam) * (size + 32 + 4) + sum(ran) * tab,
                                         "rounds_best_host": 32 * B + 4 * B + sum(p_exam) * (size + 32 + 4) + p_steps * len(table),
                                         "all_then_pick_host": B * (size + 32) + len(table)}
                a = rec["rounds_best_distinct_host"]
                for other in ("loop_of_round_best_distinct_host", "rounds_best_host", "all_then_pick_host"):
                    o = rec[other]
                    rec["new_over_" + other] = round(a["median"] / o["median"], 4)
                rec["extra_ms_over_rounds_best_host"] = round(a["median"] - rec["rounds_best_host"]["median"], 3)
                emit(rec)
            assert ctx.health() == 0
        finally:
            ctx.close()


def standing_traffic(bbp, N, base_rows, kind, n_offers, per_offer):
    """n_offers x per_offer rows of one round as a list: every bidder of base_rows once, in ascending score (so the standing keeps
    changing), spread evenly over the first half of the stream; the other rows claim scores below every real one.  half_resent: the
    second half of every offer resends rows of earlier offers (offer 0: of its own first half), byte-equal.  forged_flood: on top of that
    16 rows of every offer carry the best bidder's row under a forged score near l, each a different one."""
    import random
    row, key_off = bbp.round_row_size(N), bbp.record_size(N)
    score = lambda r: int.from_bytes(r[key_off:key_off + 32], "little")
    uniq = sorted({base_rows[row * i:row * (i + 1)][-32:]: base_rows[row * i:row * (i + 1)] for i in range(len(base_rows) // row)}.values(), key=score)
    B = n_offers * per_offer
    step = (B // 2) // len(uniq)
    L = (1 << 252) + 27742317777372353535851937790883648493
    rnd = random.Random(24)
    rows = []
    for i in range(B):
        o, j = divmod(i, per_offer)
        if kind != "no_resends" and j >= per_offer // 2:
            rows.append(rows[rnd.randrange(per_offer // 2)] if o == 0 else rows[rnd.randrange(o * per_offer)])
        elif kind == "forged_flood" and j < 16:
            rows.append(uniq[-1][:key_off] + (L - 1 - i).to_bytes(32, "little") + uniq[-1][key_off + 32:])
        elif i % step == 0 and i // step < len(uniq):
            rows.append(uniq[i // step])
        else:
            r = uniq[i % len(uniq)]
            rows.append(r[:key_off] + (i + 1).to_bytes(32, "little") + r[key_off + 32:])
    return rows, [score(r) for r in rows], [r[-32:] for r in rows]


def standing_main(args):
    """--standing: one round at N = 50, K = 3; 8192 rows arrive as 32 offers of 256.  Arms, alternated: (a) offers to a standing; (b)
    bbp_verify_round_best_distinct over all rows so far after each burst; (c) the same call on each burst alone, floor 0 (its answers
    would still have to be merged by hand: here for cost).  Per arm ms per burst, bytes uploaded and rows verified; arm (a)'s rows
    verified are asserted equal to the model's of tests/round_standing_cases.py on the verdicts of bbp_verify_rounds_aggregated."""
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    from tests import round_standing_cases as sc
    box = box_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.standing)), exist_ok=True)
    N, K, tranche, n_offers, per, n_base = 50, 3, 0, 32, 256, 41
    B = n_offers * per
    unit = "ms of host time per burst (a run is the %d bursts of the round in order), %d runs after a warm-up, arms alternated" % (n_offers, args.runs)
    with open(args.standing, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        lib, h = bbp.lib, ctx.handle
        try:
            r0 = rc.honest(N, n_base, tag=24)
            proved, _t, st = ctx.prove_round(N, r0.table, r0.bid_bytes)
            assert st == [0] * n_base
            size, tab = bbp.round_row_size(N), 32 * (1 + N)
            table = (ctypes.c_uint8 * len(r0.table)).from_buffer_copy(r0.table)
            Ns, floor, nfb = (ctypes.c_uint32 * 1)(N), (ctypes.c_uint8 * 32)(), ctypes.c_uint32()
            for kind in ("no_resends", "half_resent", "forged_flood"):
                row_list, keys, ids = standing_traffic(bbp, N, proved, kind, n_offers, per)
                blob = bytearray(b"".join(row_list))
                host = (ctypes.c_uint8 * len(blob)).from_buffer(blob)
                status = (ctypes.c_int32 * B)()
                assert lib.bbp_verify_rounds_aggregated(h, 1, Ns, table, B, None, host, status, 0, ctypes.byref(nfb)) == 0
                verdicts = list(status)
                model, want, m_bytes = sc.Standing(0, K), [], 0
                for o in range(n_offers):
                    sl = slice(o * per, (o + 1) * per)
                    want.append(model.offer(keys[sl], ids[sl], verdicts[sl], tranche))
                    m_bytes += 64 * per + want[-1][3] * (size + 32 + 4) + model.tranches * tab
                assert [(k, i) for k, i, _ in model.entries] == [(k, i) for k, i, _ in sc.truth(keys, ids, verdicts, 0, K)]
                ent = (ctypes.c_uint32 * K)()
                n = [ctypes.c_uint32() for _ in range(4)]
                p = [ctypes.byref(x) for x in n]
                at = lambda first: ctypes.byref(host, size * first)
                seen = {}

                def a_standing():
                    hs = ctx.standing_open(N, r0.table, 0, K)
                    got = []
                    for o in range(n_offers):
                        assert lib.bbp_standing_offer(h, hs, per, at(o * per), tranche, K, ent, p[0], p[1], p[2], p[3], status) == 0, lib.bbp_last_error(h)
                        got.append((list(ent)[:n[0].value], n[0].value, n[1].value, n[2].value, n[3].value, list(status)[:per]))
                    seen["entries"] = ctx.standing_read(hs)
                    ctx.standing_close(hs)
                    return got

                def one_shot(first, rows):
                    assert lib.bbp_verify_round_best_distinct(h, N, table, rows, at(first), floor, K, tranche, K, ent, p[0], p[1], p[2], p[3], status) == 0
                    return n[2].value, 64 * rows + n[2].value * (size + 32 + 4)

                def b_all_so_far():
                    return [one_shot(0, (o + 1) * per) for o in range(n_offers)]

                def c_burst_alone():
                    return [one_shot(o * per, per) for o in range(n_offers)]
                got = a_standing()
                assert got == want, "an offer differs from the model"  # nothing here is tuned: the rules predict every output
                examined = sum(g[3] for g in got)
                assert examined == sum(w[3] for w in want)
                assert list(zip(seen["entries"].scores, seen["entries"].z_imgs)) == [(k.to_bytes(32, "little"), i) for k, i, _ in model.entries]
                arms = {"standing_offers": a_standing, "best_distinct_over_all_so_far": b_all_so_far, "best_distinct_on_each_burst_alone": c_burst_alone}
                b_out, c_out = b_all_so_far(), c_burst_alone()
                args.calls = 1
                rec = {"section": "standing", "N": N, "K": K, "tranche": "default", "rows": B, "offers": n_offers, "rows_per_offer": per, "traffic": kind,
                       "valid_rows": verdicts.count(0), "unit": unit}
                for name, v in timed(arms, list(arms), args).items():
                    rec[name] = {k: round(x / n_offers, 4) for k, x in v.items()}
                rec["rows_verified"] = {"standing_offers": examined, "best_distinct_over_all_so_far": sum(x for x, _ in b_out),
                                        "best_distinct_on_each_burst_alone": sum(x for x, _ in c_out)}
                # score || z_img of every row handed over, the examined rows with their entropy and status words, a round table per tranche
                # (arms b and c: the table counted once per call -- a lower bound)
                rec["bytes_uploaded"] = {"standing_offers": m_bytes, "best_distinct_over_all_so_far": sum(y for _, y in b_out) + n_offers * tab,
                                         "best_distinct_on_each_burst_alone": sum(y for _, y in c_out) + n_offers * tab}
                rec["duplicates_left_unverified_by_standing"] = sum(g[4] for g in got)
                emit(rec)
            assert ctx.health() == 0
        finally:
            ctx.close()


def standings_main(args):
    """--standings: 64 rounds at N = 50, K = 3, one standing each; 8192 rows arrive as 32 bursts of 256, 4 rows of every round in every
    burst.  Arms, alternated: (a) one bbp_standings_offer per burst; (b) one bbp_standing_offer per standing per burst."""
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    from tests import round_standing_cases as sc
    from tests import standings_cases as mc
    box = box_id()
    os.makedirs(os.path.dirname(os.path.abspath(args.standings)), exist_ok=True)
    N, K, tranche, S, n_bursts, per_round, n_base = 50, 3, 0, 64, 32, 4, 8
    per = S * per_round
    B = n_bursts * per
    unit = "ms of host time per burst (a run is the %d bursts in order, the standings opened before and read and closed after), %d runs after a warm-up, arms alternated" % (n_bursts, args.runs)
    with open(args.standings, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        lib, h = bbp.lib, ctx.handle
        try:
            size, tab = bbp.round_row_size(N), 32 * (1 + N)
            tables, rows, keys, ids, verdicts = [], [], [], [], []
            for r in range(S):  # every round: its own seed and list, eight proved bidders, a stream of 128 rows with resends
                r0 = rc.honest(N, n_base, tag=250 + r)
                proved, _t, st = ctx.prove_round(N, r0.table, r0.bid_bytes)
                assert st == [0] * n_base
                rl, k, i = standing_traffic(bbp, N, proved, "half_resent", n_bursts, per_round)
                tables.append(r0.table), rows.append(rl), keys.append(k), ids.append(i)
                verdicts.append(ctx.verify_rounds([N], r0.table, None, b"".join(rl)))
            # burst o: row j of every round, then row j + 1: a wavefront holds rows of all rounds
            idx = [[(r, o * per_round + j) for j in range(per_round) for r in range(S)] for o in range(n_bursts)]
            so = (ctypes.c_uint32 * per)(*[r for r, _ in idx[0]])
            mixed = [(ctypes.c_uint8 * (size * per)).from_buffer_copy(b"".join(rows[r][x] for r, x in burst)) for burst in idx]
            alone = [[(ctypes.c_uint8 * (size * per_round)).from_buffer_copy(b"".join(rows[r][o * per_round:(o + 1) * per_round])) for r in range(S)]
                     for o in range(n_bursts)]
            models, want, bytes_a, bytes_b = [sc.Standing(0, K) for _ in range(S)], [], 0, 0
            for burst in idx:
                w = mc.offer(models, [r for r, _ in burst], [keys[r][x] for r, x in burst], [ids[r][x] for r, x in burst], [verdicts[r][x] for r, x in burst],
                             tranche)
                want.append(w)
                examined = sum(p[3] for p in w[0])
                # score || z_img of every row handed over, the examined rows with their entropy and status words, and the round tables: arm
                # (a) one table of S rounds per step, arm (b) one round per tranche of every standing
                bytes_a += 64 * per + examined * (size + 32 + 4) + w[1] * S * tab
                bytes_b += 64 * per + examined * (size + 32 + 4) + sum(m.tranches for m in models) * tab
            for r in range(S):
                assert [(k, i) for k, i, _ in models[r].entries] == [(k, i) for k, i, _ in sc.truth(keys[r], ids[r], verdicts[r], 0, K)]
            ent, status = (ctypes.c_uint32 * (S * K))(), (ctypes.c_int32 * per)()
            cnt = [(ctypes.c_uint32 * S)() for _ in range(4)]
            steps = ctypes.c_uint32()
            one = [ctypes.c_uint32() for _ in range(4)]
            p1 = [ctypes.byref(x) for x in one]
            seen = {}

            def opened():
                return [ctx.standing_open(N, tables[r], 0, K) for r in range(S)]

            def closed(hs, arm):
                seen[arm] = [ctx.standing_read(x) for x in hs]
                for x in hs:
                    ctx.standing_close(x)

            def a_one_call_per_burst():
                hs = opened()
                handles = (ctypes.c_uint32 * S)(*hs)
                got = []
                for o in range(n_bursts):
                    assert lib.bbp_standings_offer(h, S, handles, per, so, mixed[o], tranche, K, ent, cnt[0], cnt[1], cnt[2], cnt[3], ctypes.byref(steps),
                                                   status) == 0, lib.bbp_last_error(h)
                    e = list(ent)
                    got.append(([[e[K * r:K * r + min(cnt[0][r], K)], cnt[0][r], cnt[1][r], cnt[2][r], cnt[3][r]] for r in range(S)], steps.value,
                                list(status)))
                closed(hs, "a")
                return got

            def b_one_call_per_standing():
                hs = opened()
                examined = 0
                for o in range(n_bursts):
                    for r in range(S):
                        assert lib.bbp_standing_offer(h, hs[r], per_round, alone[o][r], tranche, K, ent, p1[0], p1[1], p1[2], p1[3], status) == 0
                        examined += one[2].value
                closed(hs, "b")
                return examined
            got = a_one_call_per_burst()
            assert got == [(w[0], w[1], w[2]) for w in want], "an offer differs from the model"  # nothing here is tuned: the rules predict every output
            examined_a = sum(p[3] for g in got for p in g[0])
            examined_b = b_one_call_per_standing()
            assert seen["a"] == seen["b"], "the two arms leave different standings"
            assert examined_a == examined_b
            arms = {"one_standings_offer_per_burst": a_one_call_per_burst, "one_standing_offer_per_standing_per_burst": b_one_call_per_standing}
            args.calls = 1
            rec = {"section": "standings", "N": N, "K": K, "tranche": "default", "standings": S, "rows": B, "bursts": n_bursts, "rows_per_burst": per,
                   "rows_per_standing_per_burst": per_round, "traffic": "half_resent", "valid_rows": sum(v.count(0) for v in verdicts), "unit": unit}
            for name, v in timed(arms, list(arms), args).items():
                rec[name] = {k: round(x / n_bursts, 4) for k, x in v.items()}
            assert seen["a"] == seen["b"]
            rec["rows_verified"] = {"one_standings_offer_per_burst": examined_a, "one_standing_offer_per_standing_per_burst": examined_b}
            rec["bytes_uploaded"] = {"one_standings_offer_per_burst": bytes_a, "one_standing_offer_per_standing_per_burst": bytes_b}
            rec["steps"] = sum(g[1] for g in got)
            rec["engine_calls"] = {"one_standings_offer_per_burst": sum(g[1] for g in got), "one_standing_offer_per_standing_per_burst": "one per tranche of every standing"}
            emit(rec)
            assert ctx.health() == 0
        finally:
            ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--standings", nargs="?", const=os.path.join(ROOT, "profiles", "r25_standings.jsonl"), default="", metavar="OUT",
                    help="measure one offer to many standings instead, into OUT (default profiles/r25_standings.jsonl)")
    ap.add_argument("--standing", nargs="?", const=os.path.join(ROOT, "profiles", "r24_round_standing.jsonl"), default="", metavar="OUT",
                    help="measure offers to a standing instead, into OUT (default profiles/r24_round_standing.jsonl)")
    ap.add_argument("--rounds-distinct", default="", metavar="OUT",
                    help="measure bbp_verify_rounds_best_distinct instead, into OUT (profiles/r23_rounds_best_distinct.jsonl)")
    ap.add_argument("--rounds", default="", metavar="OUT", help="measure bbp_verify_rounds_best instead, into OUT (profiles/r22_rounds_best.jsonl)")
    ap.add_argument("--distinct", default="", metavar="OUT", help="measure bbp_verify_round_best_distinct instead, into OUT")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_round_best.jsonl"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--sections", default="cells,sweep")
    args = ap.parse_args()
    if args.standings:
        return standings_main(args)
    if args.standing:
        return standing_main(args)
    if args.rounds_distinct:
        return rounds_distinct_main(args)
    if args.rounds:
        return rounds_main(args)
    if args.distinct:
        return distinct_main(args)
    import numpy as np
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    box = box_id()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T_DEFAULT = bbp.BEST_TRANCHE_DEFAULT
    with open(args.out, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        try:
            base = {}
            for N in (8, 202):
                r = rc.honest(N, 64, tag=19)
                rows, _t, st = ctx.prove_round(N, r.table, r.bid_bytes)
                assert st == [0] * 64
                base[N] = (rows, r.table)
            unit = "ms of host time per call, best of %d, %d runs after a warm-up" % (args.calls, args.runs)
            if "cells" in args.sections:
                for N, B in ((8, 8192), (202, 8192), (8, 65536)):
                    for tname, frac in TRAFFIC:
                        c = Cell(torch, bbp, np, N, B, base[N][0], base[N][1], frac)
                        arms = make_arms(ctx, bbp, torch, np, c, 0)
                        examined, tranches = predict(B, c.forged, 1, T_DEFAULT)
                        want = (c.best, 1 if c.best is not None else 0, B, examined)
                        assert arms["best_host"]() == want and arms["best_dev"]() == want, (arms["best_host"](), want)  # nothing here is tuned: the rules predict it
                        assert arms["all_then_pick_host"]() == (c.best,) and arms["all_then_pick_dev"]() == (c.best,)
                        rec = {"section": "cells", "N": N, "B": B, "traffic": tname, "K": 1, "tranche": T_DEFAULT, "rows_examined": examined,
                               "tranches": tranches, "unit": unit}
                        rec.update(timed(arms, list(arms), args))
                        tab = 32 * (1 + N)
                        rec["bytes_uploaded"] = {"best_host": 32 * B + examined * (c.row + 32 + 4) + tranches * tab, "all_then_pick_host": B * (c.row + 32) + tab}
                        rec["ratio_A_over_B"] = {"host": round(rec["best_host"]["median"] / rec["all_then_pick_host"]["median"], 4),
                                                 "dev": round(rec["best_dev"]["median"] / rec["all_then_pick_dev"]["median"], 4)}
                        for form in ("host", "dev"):
                            a, b = rec["best_" + form], rec["all_then_pick_" + form]
                            rec["A_loses_by_more_than_B_range_" + form] = a["median"] - b["median"] > b["max"] - b["min"]
                        emit(rec)
                        del c, arms
            if "sweep" in args.sections:
                for N in (8, 202):
                    for tname, frac in (TRAFFIC[0], TRAFFIC[2]):
                        c = Cell(torch, bbp, np, N, 8192, base[N][0], base[N][1], frac)
                        rec = {"section": "sweep", "N": N, "B": 8192, "traffic": tname, "K": 1, "unit": unit}
                        sweep = {}
                        for tranche in (16, 64, 256, 1024):
                            sweep[tranche] = make_arms(ctx, bbp, torch, np, c, tranche)["best_host"]
                            examined, tranches = predict(8192, c.forged, 1, tranche)
                            assert sweep[tranche]() == (c.best, 1, 8192, examined)
                            rec["rows_examined_%d" % tranche] = examined
                        for k, v in timed(sweep, list(sweep), args).items():
                            rec["tranche_%d" % k] = v
                        emit(rec)
                        del c
            assert ctx.health() == 0
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
