#!/usr/bin/env python3
"""Concurrent single-proof verify callers (bbp_verify_async) with verify mixing off and on (bbp_set_verify_mixing): one process, one
context, valid rows prepared once.  A case is a burst of M requests; its time runs from the first submit to the last callback.
Best of `--steps` after `--warmup` bursts per arm, the bbp_batching_stats deltas of the best burst beside it.  Cases: M from
`--ms`; N drawn from 1..202, from {8, 50, 120, 202}, and one N (8).  `--repeat R` runs every one-N and four-value case R times over
(the run-to-run spread that any difference between the arms has to exceed).  The combiner is configured as the UDS server configures
it by default (`--window-us 200 --max-batch 4096`).  On a library without bbp_set_verify_mixing (an older build) the one arm
is that build's own grouping, reported as "parent".

`--server`: one more case through bbp-uds-server, a verify-only closed loop over four N with `--verify-mixing off` and `on`.
bbp-uds-loadgen's operation is prove-then-verify of one N, so this loop is driven from Python speaking tests/uds_client.py's
protocol: `--client-procs` fresh client processes (no GPU in them) of `--connections` threads each, one connection per thread,
every connection with one of the four N.  The arms alternate `--server-rounds` times, each with a server of its own.  Ahead
of it, what one small device call costs for each of the four N and for a mixed call over them (the closed loop is bound by it).

    python tools/verify_combine.py --out profiles/r07_verify_combine.jsonl --server

`--rounds`: round sharing instead (bbp_set_verify_round_sharing): the same bursts with sharing off and on, mixing left on.  Cases: one
round at N = 8 and N = 202 (M from `--ms`), eight rounds of four list lengths (largest M), and rounds that are all distinct (smallest M:
the fallback, which must come out level).  The arms alternate over `--runs` runs, each run the best of `--steps` after `--warmup`
bursts per arm; a line reports every arm's median and range over the runs, the bytes each arm hands to the engine (expanded rows
against short rows plus tables, from bbp_verify_round_sharing_stats), and `within_margin`: the on arm's median is not above the off
arm's by more than the off arm's own range.  With `--server`: a verify-only closed loop of one round at N = 202 through
bbp-uds-server `--verify-rounds off` and `on`.

    python tools/verify_combine.py --rounds --server --out profiles/r11_verify_round_sharing.jsonl
"""
import argparse
import ctypes
import json
import os
import random
import signal
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bbp = None  # the engine binding: imported by main(), not by the socket clients (they are plain processes without a GPU)

L = 2 ** 252 + 27742317777372353535851937790883648493
DISTS = {"uniform_1_202": lambda r: r.randint(1, 202), "four_values": lambda r: r.choice((8, 50, 120, 202)), "one_n": lambda r: 8}


def sc(r):
    return (r.getrandbits(256) % L).to_bytes(32, "little")


def requests_for(ctx, N, count, r):
    """`count` valid (record, score, z_img, seed, pub_list) of list length N, proved by the engine."""
    dks = b"".join(r.getrandbits(64).to_bytes(8, "little") + bytes(24) + sc(r) + sc(r) for _ in range(count))
    w = ctx.witness_batch(dks)
    ins, tails = [], []
    for i in range(count):
        m, x, y, yi, q, z = (w[192 * i + 32 * j:192 * i + 32 * j + 32] for j in range(6))
        d, k, sd = dks[96 * i:96 * i + 32], dks[96 * i + 32:96 * i + 64], dks[96 * i + 64:96 * i + 96]
        pub = [sc(r) for _ in range(N)]
        pub[i % N] = x
        ins.append(d + k + y + yi + q + z + sd + b"".join(pub) + (i % N).to_bytes(8, "little"))
        tails.append((q, z, sd, b"".join(pub)))
    out, st = ctx.prove_batch(count, N, b"".join(ins))
    assert st == [0] * count
    rs_ = bbp.record_size(N)
    return [(out[i * rs_:(i + 1) * rs_],) + tails[i] for i in range(count)]


def round_requests(ctx, N, count, r):
    """`count` valid requests (at most N) of ONE round: one seed, one list, the bids at list positions 0..count-1."""
    count = min(count, N)
    sd = sc(r)
    dks = b"".join(r.getrandbits(64).to_bytes(8, "little") + bytes(24) + sc(r) + sd for _ in range(count))
    w = ctx.witness_batch(dks)
    wit = [[w[192 * i + 32 * j:192 * i + 32 * j + 32] for j in range(6)] for i in range(count)]
    pub = [sc(r) for _ in range(N)]
    for i in range(count):
        pub[i] = wit[i][1]
    pub = b"".join(pub)
    ins = b"".join(dks[96 * i:96 * i + 64] + wit[i][2] + wit[i][3] + wit[i][4] + wit[i][5] + sd + pub + i.to_bytes(8, "little") for i in range(count))
    out, st = ctx.prove_batch(count, N, ins)
    assert st == [0] * count
    rs_ = bbp.record_size(N)
    return [(out[i * rs_:(i + 1) * rs_], wit[i][4], wit[i][5], sd, pub) for i in range(count)]


class Burst:
    """M prepared bbp_verify_async calls: ctypes arguments built once, one shared callback that counts down."""

    def __init__(self, ctx, reqs):
        self.h = ctx.handle() if callable(getattr(ctx, "handle", None)) else ctx._h
        self.fn = bbp._native.lib.bbp_verify_async
        self.args = [(ctypes.c_char_p(r[0]), len(r[0]), ctypes.c_char_p(r[1]), ctypes.c_char_p(r[2]), ctypes.c_char_p(r[3]), ctypes.c_char_p(r[4]),
                      len(r[4]) // 32) for r in reqs]
        self.keep = reqs
        self.lock, self.done = threading.Lock(), threading.Event()
        self.left, self.bad = 0, 0
        self.cb = bbp._native.DONE_FN(self._on_done)

    def _on_done(self, _user, status):
        with self.lock:
            self.bad += status != 0
            self.left -= 1
            if self.left == 0:
                self.done.set()

    def run(self):
        self.left, self.bad = len(self.args), 0
        self.done.clear()
        fn, h, cb = self.fn, self.h, self.cb
        t = time.perf_counter()
        for a in self.args:
            rc = fn(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], cb, None)
            assert rc == 0, rc
        t_sub = time.perf_counter() - t
        assert self.done.wait(600), "callbacks missing"
        dt = time.perf_counter() - t
        assert self.bad == 0, "%d valid proofs were refused" % self.bad
        return dt, t_sub


def measure(ctx, b, warmup, steps):
    for _ in range(warmup):
        b.run()
    best = None
    for _ in range(steps):
        c0 = ctx.batching_stats()
        dt, t_sub = b.run()
        c1 = ctx.batching_stats()
        if best is None or dt < best["ms"] / 1e3:
            best = {"ms": round(dt * 1e3, 3), "submit_ms": round(t_sub * 1e3, 3), "calls": c1[0] - c0[0], "requests": c1[1] - c0[1]}
    return best


def measure_rounds(ctx, b, warmup, steps):
    """measure() with the round-sharing counters of the best burst beside it"""
    for _ in range(warmup):
        b.run()
    best = None
    for _ in range(steps):
        c0, s0 = ctx.batching_stats(), ctx.verify_round_sharing_stats()
        dt, t_sub = b.run()
        c1, s1 = ctx.batching_stats(), ctx.verify_round_sharing_stats()
        if best is None or dt < best["ms"] / 1e3:
            best = {"ms": round(dt * 1e3, 3), "submit_ms": round(t_sub * 1e3, 3), "calls": c1[0] - c0[0], "round_calls": s1[0] - s0[0],
                    "round_rows": s1[1] - s0[1], "round_tables": s1[2] - s0[2]}
    return best


def summarise(runs):
    ms = sorted(x["ms"] for x in runs)
    return {"median_ms": ms[len(ms) // 2], "range_ms": round(ms[-1] - ms[0], 3), "min_ms": ms[0], "max_ms": ms[-1]}


def engine_bytes(reqs, n_rounds_case, best):
    """Bytes the best burst handed to the engine: every request's expanded row, less what the rounds calls saved.  Exact when every
    request left in a rounds call that held every round of the case (or when none did); else in proportion."""
    expanded = sum(len(x) for q in reqs for x in q)
    tails = sum(len(q[3]) + len(q[4]) for q in reqs)
    distinct = {q[3] + q[4] for q in reqs}
    tables = sum(len(t) for t in distinct)
    M, rows, calls, held = len(reqs), best["round_rows"], best["round_calls"], best["round_tables"]
    if calls == 0:
        return expanded, True
    exact = rows == M and held == calls * n_rounds_case
    return int(expanded - tails * rows / M + tables * held / max(1, len(distinct))), exact


def rounds_cases(a, ctx, r):
    Ms = sorted(int(x) for x in a.ms.split(","))
    cases, pool = [], {}
    for n in (8, 202):
        pool[n] = round_requests(ctx, n, a.per_n, r)
        for M in Ms:
            cases.append(("one_round_n%d" % n, 1, [pool[n][i % len(pool[n])] for i in range(M)]))
    eight = [round_requests(ctx, n, a.per_n, r) for n in (8, 50, 120, 202) for _ in range(2)]
    cases.append(("eight_rounds_four_lengths", 8, [eight[i % 8][(i // 8) % len(eight[i % 8])] for i in range(Ms[-1])]))
    cases.append(("all_distinct_rounds_n8", Ms[0], requests_for(ctx, 8, Ms[0], r)))
    return cases, pool


def rounds_main(a):
    ctx = bbp.Context(0)
    ctx.set_batching(a.window_us, a.max_batch)
    r = random.Random(1111)
    cases, pool = rounds_cases(a, ctx, r)
    lines = []
    for name, n_rounds_case, reqs in cases:
        b = Burst(ctx, reqs)
        runs = {"off": [], "on": []}
        for run in range(a.runs):
            for arm in (("off", "on") if run % 2 == 0 else ("on", "off")):  # alternated: neither arm always runs on the warmer device
                ctx.set_verify_round_sharing(arm == "on")
                runs[arm].append(measure_rounds(ctx, b, a.warmup, a.steps))
        ctx.set_verify_round_sharing(False)
        line = {"case": name, "M": len(reqs), "rounds": n_rounds_case, "window_us": a.window_us, "max_batch": a.max_batch, "steps": a.steps,
                "warmup": a.warmup, "runs": a.runs}
        if a.label:
            line["label"] = a.label
        for arm in ("off", "on"):
            best = min(runs[arm], key=lambda x: x["ms"])
            nbytes, exact = engine_bytes(reqs, n_rounds_case, best)
            line[arm] = dict(summarise(runs[arm]), best=best, engine_bytes=nbytes, engine_bytes_exact=exact)
        line["off_over_on"] = round(line["off"]["median_ms"] / line["on"]["median_ms"], 3)
        line["within_margin"] = line["on"]["median_ms"] <= line["off"]["median_ms"] + line["off"]["range_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    assert ctx.health() == 0
    ctx.close()
    if a.server:
        server_case(a, {202: pool[202]}, lines, flag="--verify-rounds", case="server_closed_loop_one_round_n202", reserve="202")
        mine = [l for l in lines if l.get("case") == "server_closed_loop_one_round_n202"]
        off = sorted(l["ops_per_s"] for l in mine if l["verify_rounds"] == "off")
        on = sorted(l["ops_per_s"] for l in mine if l["verify_rounds"] == "on")
        line = {"case": "server_closed_loop_one_round_n202_summary", "off_median_ops_per_s": off[len(off) // 2], "off_range": round(off[-1] - off[0], 1),
                "on_median_ops_per_s": on[len(on) // 2], "on_range": round(on[-1] - on[0], 1)}
        line["within_margin"] = line["on_median_ops_per_s"] >= line["off_median_ops_per_s"] - line["off_range"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def latency_case(ctx, pool, lines):
    """What one small device call costs by list length, and a mixed call over the four: best of 20 bbp_verify_batch /
    bbp_verify_batch_mixed calls of B rows.  A mixed call takes as long as a uniform call of its largest N."""
    ns = (8, 50, 120, 202)

    def best(fn):
        for _ in range(3):
            fn()
        b = float("inf")
        for _ in range(20):
            t = time.perf_counter()
            fn()
            b = min(b, time.perf_counter() - t)
        return round(b * 1e3, 3)
    for B in (8, 32, 128):
        line = {"case": "small_call_latency_ms", "B": B}
        for n in ns:
            blob = b"".join(b"".join(pool[n][i % len(pool[n])]) for i in range(B))
            line["uniform_n%d" % n] = best(lambda: ctx.verify_batch(B, n, blob))
        Ns = [ns[i % 4] for i in range(B)]
        blob = b"".join(b"".join(pool[n][i % len(pool[n])]) for i, n in enumerate(Ns))
        line["mixed_four_values"] = best(lambda: ctx.verify_batch_mixed(Ns, blob))
        print(json.dumps(line), flush=True)
        lines.append(line)


def client_main(path, frames_file, n_threads, seconds, index):
    """A client process of the server case: n_threads connections in a closed loop for 2 s of warm-up plus `seconds`."""
    import pickle
    from tests import uds_client as uc
    frames = pickle.load(open(frames_file, "rb"))
    ns = sorted(frames)
    stop_at = time.perf_counter() + seconds + 2.0
    counts, lat, errors = [0] * n_threads, [[] for _ in range(n_threads)], []

    def worker(i):
        try:
            c = uc.Conn(path, timeout=120.0)
            fr = frames[ns[(index + i) % len(ns)]]
            k = 0
            while time.perf_counter() < stop_at:
                t = time.perf_counter()
                c.send(fr[k % len(fr)])
                assert c.recv_frame() == b"\x01"
                if t >= stop_at - seconds:  # (after the warm-up part)
                    lat[i].append(time.perf_counter() - t)
                    counts[i] += 1
                k += 1
            c.close()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(n_threads)]
    for t in th:
        t.start()
    for t in th:
        t.join(seconds + 180)
    print(json.dumps({"ops": sum(counts), "lat_ms": [round(x * 1e3, 3) for l in lat for x in l][::7], "errors": errors[:3]}))


def server_case(a, pool, lines, flag="--verify-mixing", case="server_closed_loop_four_values", reserve="202"):
    import pickle
    from tests import uds_client as uc
    frames = {}
    for n in sorted(pool):
        frames[n] = []
        for r in pool[n]:
            body = r[0][1121:]
            pts = [body[32 * i:32 * i + 32] for i in range(4 + n)]
            blob = uc.tlv(r[0][:1121]) + uc.tlv_list(pts[:4]) + uc.tlv_list(pts[4:])
            frames[n].append(uc.verify_request(blob, r[1], r[2], r[3], r[4]))
    d0 = tempfile.mkdtemp(prefix="bbp-vc-")
    frames_file = os.path.join(d0, "frames.pkl")
    pickle.dump(frames, open(frames_file, "wb"))
    server = os.path.join(ROOT, "dusk_blindbidproof_amd", "server", "bbp-uds-server")
    for rnd in range(a.server_rounds):
        for arm in ("off", "on"):
            d = tempfile.mkdtemp(prefix="bbp-vc-")
            path, blog = os.path.join(d, "sock"), os.path.join(d, "batches")
            p = subprocess.Popen([server, "-b", path, "-l", "warn", "--engine", bbp.lib_path, "--device", "0", flag, arm, "--reserve", reserve,
                                  "--max-batch", "1024"], env=dict(os.environ, BBP_BATCH_LOG=blog))
            try:
                for _ in range(6000):
                    if os.path.exists(path) or p.poll() is not None:
                        break
                    time.sleep(0.02)
                assert os.path.exists(path), "server did not bind"
                cl = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--client", path, frames_file, str(a.connections), str(a.seconds), str(k)],
                                       stdout=subprocess.PIPE, text=True) for k in range(a.client_procs)]
                outs = [json.loads(c.communicate(timeout=a.seconds + 240)[0]) for c in cl]
            finally:
                if p.poll() is None:
                    p.send_signal(signal.SIGTERM)
                    p.wait(timeout=60)
            assert not any(o["errors"] for o in outs), [o["errors"] for o in outs]
            rows = [l.split() for l in open(blog) if l.strip()]
            v = [r for r in rows if r[2] == "verify"]
            all_lat = sorted(x for o in outs for x in o["lat_ms"])
            line = {"case": case, flag[2:].replace("-", "_"): arm, "round": rnd, "connections": a.connections * a.client_procs,
                    "seconds": a.seconds, "client": "%d python processes x %d threads" % (a.client_procs, a.connections),
                    "ops_per_s": round(sum(o["ops"] for o in outs) / a.seconds, 1), "p50_ms": all_lat[len(all_lat) // 2],
                    "p99_ms": all_lat[int(len(all_lat) * 0.99)], "verify_batches": len(v),
                    "mean_batch": round(sum(int(r[4]) for r in v) / max(1, len(v)), 2),
                    "mixed_batches": sum(1 for r in v if len(r) > 8 and int(r[8]) > 1)}
            print(json.dumps(line), flush=True)
            lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/r07_verify_combine.jsonl, with --rounds profiles/r11_verify_round_sharing.jsonl")
    ap.add_argument("--rounds", action="store_true", help="round sharing off / on instead of verify mixing off / on")
    ap.add_argument("--runs", type=int, default=5, help="--rounds: runs per case, arms alternated; median and range over them")
    ap.add_argument("--ms", default="1024,8192")
    ap.add_argument("--dists", default="uniform_1_202,four_values,one_n")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=1, help="runs of every one-N and four-value case (spread)")
    ap.add_argument("--per-n", type=int, default=8, help="distinct proofs per N; requests of the same N reuse them in turn")
    ap.add_argument("--window-us", type=int, default=200)
    ap.add_argument("--max-batch", type=int, default=4096)
    ap.add_argument("--server", action="store_true")
    ap.add_argument("--connections", type=int, default=32, help="server case: connections (threads) per client process")
    ap.add_argument("--client-procs", type=int, default=8)
    ap.add_argument("--server-rounds", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    global bbp
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py)
    import dusk_blindbidproof_amd as bbp
    if a.out is None:
        a.out = "profiles/r11_verify_round_sharing.jsonl" if a.rounds else "profiles/r07_verify_combine.jsonl"
    if a.rounds:
        lines = rounds_main(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
        return
    ctx = bbp.Context(0)
    ctx.set_batching(a.window_us, a.max_batch)
    has_switch = hasattr(ctx, "set_verify_mixing")
    arms = [("off", False), ("on", True)] if has_switch else [("parent", None)]
    r = random.Random(707)
    Ms = [int(x) for x in a.ms.split(",")]
    lines, pool = [], {}
    for dist in a.dists.split(","):
        Ns_all = [DISTS[dist](r) for _ in range(max(Ms))]
        for n in sorted(set(Ns_all)):
            if n not in pool:
                pool[n] = requests_for(ctx, n, a.per_n, r)
        used = {n: 0 for n in pool}
        reqs_all = []
        for n in Ns_all:
            reqs_all.append(pool[n][used[n] % len(pool[n])])
            used[n] += 1
        for M in Ms:
            b = Burst(ctx, reqs_all[:M])
            for rep in range(1 if dist == "uniform_1_202" else a.repeat):
                line = {"case": dist, "M": M, "distinct_n": len(set(Ns_all[:M])), "window_us": a.window_us, "max_batch": a.max_batch, "steps": a.steps,
                        "warmup": a.warmup, "run": rep}
                if a.label:
                    line["label"] = a.label
                for name, on in arms:
                    if on is not None:
                        ctx.set_verify_mixing(on)
                    line[name] = measure(ctx, b, a.warmup, a.steps)
                if has_switch:
                    line["off_over_on"] = round(line["off"]["ms"] / line["on"]["ms"], 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.server:
        for n in (8, 50, 120, 202):
            assert n in pool, "--server needs the four_values case"
        ctx.set_batching(0, 0)
        latency_case(ctx, pool, lines)
    assert ctx.health() == 0
    ctx.close()
    if a.server:
        server_case(a, {n: pool[n] for n in (8, 50, 120, 202)}, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--client":
        client_main(sys.argv[2], sys.argv[3], int(sys.argv[4]), float(sys.argv[5]), int(sys.argv[6]))
    else:
        main()
