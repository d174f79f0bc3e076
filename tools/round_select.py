"""What selecting a round's bids costs on one MI355X (include/bbp.h "Selecting a round's bids"; DESIGN.md has the figures).  Three
sections, one JSON line each per case, to stdout and to --out (default profiles/r18_round_select.jsonl) with the box id and --commit:

  scoring     device time (events on the call's stream) of one bbp_select_round_dev with the all-ones floor -- table reduction,
              k_round_scores, k_round_select, nothing expanded -- at B in {4096, 65536, 1048576}, N in {8, 202}; beside it, at B in
              {4096, 65536}, the pass a caller had before: bbp_prepare_round_dev with tails over all bids.  ms and bids/s.
  selection   device time of the selection launches k_round_select_* alone (their profiling tag) at B = 2^20 through bbp_debug_round_select: uniform 252-bit
              scores (what honest scores look like) for K in {1, 64, 4096}, and one adversarial input, all scores equal on their top 31
              bytes, K = 64; each as a share of the scoring time at the same B.
  end_to_end  host time of a whole call at B = 65536, N in {8, 202}, K in {1, 64}, floor 0: bbp_prove_round_select against the route a
              caller had before (bbp_prepare_round_dev over all bids, tails and statuses fetched, the pick on the host, bbp_prove_round
              on the gathered bids); bytes over PCIe and device bytes the pass writes, both from the shapes.

Arms alternate in one process; every figure is the best of --calls calls after a warm-up, taken --runs times: median and range."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab import box_id  # noqa: E402

TAG_SELECT = 14  # csrc/context.h
ALL_ONES = (1 << 256) - 1


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def tiled_round(rc, N, B):
    """B accepted bids of one round: a block of honest bids (the big-int oracle builds at most 4096 witnesses) repeated"""
    base = rc.honest(N, min(B, 4096), tag=18)
    return base, base.bid_bytes * (B // base.B)


class Dev:
    """device copies of one round's inputs and room for every output of both passes"""

    def __init__(self, torch, bbp, N, table, bids, B, rows):
        u8 = dict(dtype=torch.uint8, device="cuda")
        self.tab = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
        self.bids = torch.frombuffer(bytearray(bids), dtype=torch.uint8).cuda()
        self.sel, self.counts = torch.zeros(4, **u8), torch.zeros(8, **u8)
        self.status, self.scores = torch.zeros(4 * B, **u8), torch.zeros(32 * B, **u8)
        self.rows = torch.zeros(bbp.prove_row_size(N) * B, **u8) if rows else None
        self.tails = torch.zeros(64 * B, **u8) if rows else None


def device_ms(torch, stream, call, calls):
    """best of `calls` after one warm-up: events around the call on its stream"""
    best = None
    for it in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        if it:
            best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    return best


def scoring(ctx, bbp, torch, rc, args, emit):
    stream = torch.cuda.Stream()
    score_ms = {}
    for N in (8, 202):
        for B in (4096, 65536, 1 << 20):
            base, bids = tiled_round(rc, N, B)
            parent = B <= 65536
            d = Dev(torch, bbp, N, base.table, bids, B, parent)
            torch.cuda.synchronize()

            def new():
                ctx.select_round_dev(N, d.tab.data_ptr(), B, d.bids.data_ptr(), ALL_ONES, 0, 0, None, d.counts.data_ptr(), d.status.data_ptr(),
                                     d.scores.data_ptr(), stream=stream.cuda_stream)

            def old():
                ctx.prepare_round_dev(N, d.tab.data_ptr(), B, d.bids.data_ptr(), d.rows.data_ptr(), d.status.data_ptr(), d.tails.data_ptr(),
                                      stream=stream.cuda_stream)
            runs = {"select_pass": [], "prepare_pass": []}
            for _ in range(args.runs):
                runs["select_pass"].append(device_ms(torch, stream, new, args.calls))
                if parent:
                    runs["prepare_pass"].append(device_ms(torch, stream, old, args.calls))
            assert d.status.view(torch.int32).count_nonzero().item() == 0  # every bid accepted
            rec = {"section": "scoring", "N": N, "B": B, "unit": "ms of device time per pass, best of %d after a warm-up, %d runs" % (args.calls, args.runs)}
            for name, v in runs.items():
                if v:
                    rec[name] = stats(v)
                    rec[name]["bids_per_s"] = round(B / (statistics.median(v) * 1e-3))
            if parent:
                rec["select_not_slower_per_bid"] = rec["select_pass"]["median"] <= rec["prepare_pass"]["median"]
            score_ms[(N, B)] = rec["select_pass"]["median"]
            emit(rec)
            del d
    return score_ms


def selection(ctx, bbp, torch, args, emit, score_ms):
    import numpy as np
    B = 1 << 20
    rng = np.random.RandomState(18)
    uniform = rng.randint(0, 256, size=(B, 32), dtype=np.uint8)
    uniform[:, 31] &= 0x0f                                  # below 2^252 < l
    shared = np.tile(uniform[:1], (B, 1))
    shared[:, 0] = rng.randint(0, 256, size=B, dtype=np.uint8)  # equal on their top 31 bytes
    statuses = [0] * B
    for name, scores, K in (("uniform", uniform, 1), ("uniform", uniform, 64), ("uniform", uniform, 4096), ("top31_shared", shared, 64)):
        raw = scores.tobytes()
        ts = []
        for it in range(args.runs + 1):
            ctx.set_profiling(True)
            ctx.last_timings()
            _sel, n_sel, n_q = ctx.debug_round_select(raw, statuses, 0, K, cap=K)
            t = [us for tag, us in ctx.last_timings() if tag == TAG_SELECT]
            ctx.set_profiling(False)
            assert len(t) == 1 and (n_sel, n_q) == (K, B)
            if it:
                ts.append(t[0] * 1e-3)
        rec = {"section": "selection", "B": B, "K": K, "scores": name, "unit": "ms of device time of k_round_select_*, %d runs" % args.runs, "select": stats(ts)}
        rec["share_of_scoring"] = {"N%d" % N: round(statistics.median(ts) / score_ms[(N, B)], 4) for N in (8, 202) if (N, B) in score_ms}
        emit(rec)


def host_pick(np, tails, statuses, B, K):
    """the K best accepted bids by (score descending, index ascending), in index order: what a caller does with fetched tails"""
    w = np.frombuffer(tails, dtype="<u8").reshape(B, 8)[:, :4]
    ok = np.nonzero(np.frombuffer(statuses, dtype="<i4") == 0)[0]
    order = np.lexsort((ok, ~w[ok, 0], ~w[ok, 1], ~w[ok, 2], ~w[ok, 3]))
    return sorted(ok[order[:K]].tolist())


def end_to_end(ctx, bbp, torch, rc, args, emit):
    import numpy as np
    B = 65536
    for N in (8, 202):
        base, bids = tiled_round(rc, N, B)
        table = base.table
        row, pin = bbp.round_row_size(N), bbp.prove_row_size(N)
        for K in (1, 64):
            ctx.reserve(K, N)

            def new():
                got = ctx.prove_round_select(N, table, bids, 0, K)
                assert got.n_sel == K
                return got.sel

            def old():
                d = Dev(torch, bbp, N, table, bids, B, True)
                ctx.prepare_round_dev(N, d.tab.data_ptr(), B, d.bids.data_ptr(), d.rows.data_ptr(), d.status.data_ptr(), d.tails.data_ptr())
                torch.cuda.synchronize()
                sel = host_pick(np, d.tails.cpu().numpy().tobytes(), d.status.cpu().numpy().tobytes(), B, K)
                _rows, _t, st = ctx.prove_round(N, table, b"".join(bids[64 * i:64 * i + 64] for i in sel))
                assert st == [0] * K
                return sel
            assert new() == old()
            runs = {"prove_round_select": [], "prepare_fetch_pick_prove": []}
            for _ in range(args.runs):
                for name, f in (("prove_round_select", new), ("prepare_fetch_pick_prove", old)):
                    best = None
                    for _c in range(args.calls):
                        t = time.perf_counter()
                        f()
                        dt = (time.perf_counter() - t) * 1e3
                        best = dt if best is None else min(best, dt)
                    runs[name].append(best)
            tab = 32 * (1 + N)
            prove_io = 64 * K + tab + K * row + 12 * K  # phase B / bbp_prove_round: bids and table up; rows, toggles, statuses down (entropy drawn on the host: up too)
            prove_io += K * bbp.entropy_size(N)
            rec = {"section": "end_to_end", "N": N, "B": B, "K": K, "unit": "ms of host time per call, best of %d, %d runs" % (args.calls, args.runs)}
            for name, v in runs.items():
                rec[name] = stats(v)
            rec["pcie_bytes"] = {"prove_round_select": 64 * B + tab + 8 + 4 * K + 4 * B + prove_io, "prepare_fetch_pick_prove": 64 * B + tab + 64 * B + 4 * B + prove_io}
            rec["pass_device_bytes_written_per_bid"] = {"prove_round_select": 40 + 4, "prepare_fetch_pick_prove": 4 * 36 + pin + 64 + 8 + 4}
            a, b = rec["prove_round_select"], rec["prepare_fetch_pick_prove"]
            rec["select_loses_by_more_than_the_other_route_s_range"] = a["median"] - b["median"] > b["max"] - b["min"]
            emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_round_select.jsonl"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sections", default="scoring,selection,end_to_end")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests import prove_round_cases as rc
    box = box_id()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            rec.update(box=box, commit=args.commit)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        ctx = bbp.Context(0)
        try:
            score_ms = scoring(ctx, bbp, torch, rc, args, emit) if "scoring" in args.sections else {}
            if "selection" in args.sections:
                selection(ctx, bbp, torch, args, emit, score_ms)
            if "end_to_end" in args.sections:
                end_to_end(ctx, bbp, torch, rc, args, emit)
            assert ctx.health() == 0
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
