#!/usr/bin/env python3
"""BASELINE.json configs[4] measured THROUGH the reference's IPC surface: starts bbp-uds-server on a temp socket, writes K
pre-encoded synthetic bids, runs bbp-uds-loadgen with C closed-loop connections (one op = prove then verify, the Go
BenchmarkProveVerify's shape), prints the load generator's JSON line plus the server's batching statistics.

    python tools/uds_bench.py [--connections 2048] [--ops 16384] [--items 8] [--window-us 300] [--max-batch 1024] [--stub]
    python tools/uds_bench.py --rate 12000 --duration 10 [--connections 8192]     # open loop: Poisson arrivals at a fixed offered load
    python tools/uds_bench.py --sweep 4000,8000,12000,16000,18000 --duration 8     # latency-vs-offered-load table (one JSON line per point)
    python tools/uds_bench.py --connections 1 --depth 1024 --pipeline-depth 1024   # one connection, 1024 ops outstanding on it
    python tools/uds_bench.py --pipelining [--runs 5] [--parent-server BIN] [--out profiles/r14_uds_pipelining.jsonl]
                                                                                   # the (connections, depth) matrix of DESIGN.md 6c
"""
import argparse, json, os, re, signal, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from tests import uds_client as uc


SHUTDOWN_LINE = r"served (\d+) requests \((\d+) errors\) in (\d+) device calls, largest batch (\d+)(?:, deepest pipeline (\d+))?"


def make_bids(a, N, distinct):
    """-> (engine library, [(seven scalars, public list, toggle, score || z_img || seed)])"""
    if a.stub:
        bids = []
        for i in range(distinct):
            s7 = b"".join(bytes([(7 * i + k) & 0xff]) * 31 + b"\x01" for k in range(7))
            pub = b"".join(bytes([(11 * i + j) & 0xff]) * 31 + b"\x02" for j in range(N))
            bids.append((s7, pub, i % N, s7[128:160] + s7[160:192] + s7[192:224]))
        return ge.build_stub_engine(), bids
    import torch  # noqa: F401  (its HIP runtime first, see tests/conftest.py)
    import dusk_blindbidproof_amd as bbp
    from bench_workloads import synth_bids
    ctx = bbp.Context(0)
    ins, _, pubs, qz = synth_bids(ctx, distinct, N, seed=77)
    ctx.close()
    return bbp.lib_path, [(ins[i][:224], pubs[i], int.from_bytes(ins[i][-8:], "little"), qz[i]) for i in range(distinct)]


def verify_tail(pub, qzs, N):
    return uc.tlv(qzs[:32]) + uc.tlv(qzs[32:64]) + uc.tlv(qzs[64:96]) + uc.tlv_list([pub[32 * j:32 * j + 32] for j in range(N)])


def write_requests(path, bids, N, blobs=None):
    """the load generator's FILE: per bid the opcode-1 frame and the verify tail; with blobs (one proof per bid) the first element
    is the complete opcode-2 frame instead (bbp-uds-loadgen --verify-only)"""
    with open(path, "wb") as f:
        for i, (s7, pub, toggle, qzs) in enumerate(bids):
            vt = verify_tail(pub, qzs, N)
            pf = uc.prove_request(s7, pub, toggle) if blobs is None else uc.tlv(b"\x02" + uc.tlv(blobs[i]) + vt)
            f.write(struct.pack("<I", len(pf)) + pf + struct.pack("<I", len(vt)) + vt)


def prove_over_socket(sock, bids):
    """one proof blob per bid, request by request on one connection (the parent commit's server drops a peer that writes ahead)"""
    c = uc.Conn(sock, timeout=120.0)
    blobs = []
    for s7, pub, toggle, _ in bids:
        c.send(uc.prove_request(s7, pub, toggle))
        blobs.append(c.recv_frame())
    c.close()
    if len(blobs) != len(bids) or any(b is None for b in blobs):
        raise RuntimeError("the server did not prove the bids of the verify-only arm")
    return blobs


# (connections, depth) arms of the pipelining measurement; each runs prove-only and prove + verify at N = 8, and two verify-only arms
# at N = 202.  "parent": also measured on --parent-server, the no-regression pair.
ARMS = [dict(name="c%d_d%d_%s" % (c, k, mode), connections=c, depth=k, mode=mode, items=8, parent=(c, k) == (3072, 1))
        for c, k in ((1, 1), (1, 64), (1, 1024), (4, 256), (64, 16), (3072, 1)) for mode in ("prove", "prove+verify")]
ARMS += [dict(name="c1_d3072_prove", connections=1, depth=3072, mode="prove", items=8, parent=False)]  # as many outstanding as (3072, 1), on one connection
ARMS += [dict(name="c1_d256_verify202", connections=1, depth=256, mode="verify", items=202, parent=False),
         dict(name="c2048_d1_verify202", connections=2048, depth=1, mode="verify", items=202, parent=True)]


def run_arm(a, arm, engine, bids, server_bin, parent):
    """one server process, one warm-up and one measured closed-loop run -> the load generator's result plus the shutdown line"""
    d = tempfile.mkdtemp(prefix="bbp-uds-pipe-")
    sock, reqs, N = os.path.join(d, "sock"), os.path.join(d, "bids.bin"), arm["items"]
    conns, depth = arm["connections"], arm["depth"]
    flags = [] if parent or depth <= 64 else ["--pipeline-depth", str(depth)]  # up to 64 the default serves; the parent has no such flag
    log = open(os.path.join(d, "server.log"), "w+")
    srv = subprocess.Popen([server_bin, "-b", sock, "-l", "info", "--engine", engine, "--window-us", str(a.window_us), "--max-batch", str(a.max_batch),
                            "--max-connections", str(max(4096, 2 * conns)), "--io-threads", str(a.io_threads), "--reserve", str(N)] + flags, stderr=log,
                           env=dict(os.environ, GPU_MAX_HW_QUEUES=str(a.hwq)))
    try:
        for _ in range(6000):
            if os.path.exists(sock) or srv.poll() is not None:
                break
            time.sleep(0.02)
        if not os.path.exists(sock):
            log.seek(0)
            raise RuntimeError("server did not come up: " + log.read()[-500:])
        write_requests(reqs, bids, N, prove_over_socket(sock, bids) if arm["mode"] == "verify" else None)
        ops = a.ops if a.stub else min(32768, max(256, 8 * conns * depth))
        cmd = [ge.LOADGEN_BIN, "--socket", sock, "--requests", reqs, "--connections", str(conns), "--threads", str(min(a.gen_threads, conns)),
               "--depth", str(depth)] + {"prove": ["--no-verify"], "prove+verify": [], "verify": ["--verify-only"]}[arm["mode"]]
        subprocess.run(cmd + ["--ops", str(min(ops, 2 * conns * depth))], capture_output=True, text=True, timeout=a.arm_timeout)  # warm-up: buffers grown
        run = subprocess.run(cmd + ["--ops", str(ops)], capture_output=True, text=True, timeout=a.arm_timeout)
    finally:
        if srv.poll() is None:
            srv.send_signal(signal.SIGTERM)
        try:
            srv.wait(timeout=60)
        except subprocess.TimeoutExpired:
            srv.kill()
            srv.wait()
    log.seek(0)
    m = re.search(SHUTDOWN_LINE + r".*", log.read())
    if run.returncode != 0 or not run.stdout.strip() or srv.returncode != 0:
        raise RuntimeError("arm %s failed (loadgen %d, server %s): %s" % (arm["name"], run.returncode, srv.returncode, (run.stdout + run.stderr)[-400:]))
    out = json.loads(run.stdout.strip().splitlines()[-1])
    out["shutdown_line"] = m.group(0) if m else None
    return out


def pipelining(a):
    """The matrix: every arm `--runs` times, the arms alternating (run 1 of every arm, then run 2, ..), each run a fresh server
    under its own time limit; stops at the first failing step.  With --parent-server the no-regression arms run on that binary too,
    next to their own run, the two swapping places from run to run so that neither always follows the other.  One summary
    line per arm: median, range, p50 / p99 op latency."""
    import statistics
    want = [s for s in a.arms.split(",") if s]
    arms = [arm for arm in ARMS if not want or any(s in arm["name"] for s in want)]
    plan = []  # an arm that is also measured on the parent's server has that run next to its own; which of the two goes first alternates by run
    for arm in arms:
        plan += [(arm, False)] + ([(arm, True)] if arm["parent"] and a.parent_server else [])
    engines = {}
    for arm, _ in plan:
        if arm["items"] not in engines:
            engines[arm["items"]] = make_bids(a, arm["items"], 64 if arm["mode"] == "verify" else a.distinct)
    results = {}
    for r in range(a.runs):
        order = list(plan)
        if r % 2:
            for i in range(len(order) - 1):
                if order[i + 1][1] and not order[i][1]:
                    order[i], order[i + 1] = order[i + 1], order[i]
        for arm, parent in order:
            engine, bids = engines[arm["items"]]
            res = run_arm(a, arm, engine, bids, a.parent_server if parent else ge.SERVER_BIN, parent)
            results.setdefault((arm["name"], parent), []).append(res)
            print("run %d %s%s: %.1f ops/s" % (r + 1, arm["name"], " (parent server)" if parent else "", res["ops"] / res["wall_s"]), file=sys.stderr, flush=True)
    lines = []
    for arm, parent in plan:
        rs = results[(arm["name"], parent)]
        rates = [x["ops"] / x["wall_s"] for x in rs]
        lines.append(dict(arm=arm["name"], server="parent commit" if parent else "this commit", connections=arm["connections"], depth=arm["depth"],
                          mode=arm["mode"], bid_list_len=arm["items"], runs=len(rs), ops_per_run=rs[0]["ops"],
                          ops_per_s=dict(median=round(statistics.median(rates), 1), min=round(min(rates), 1), max=round(max(rates), 1), all=[round(x, 1) for x in rates]),
                          op_latency_ms={q: round(statistics.median(x["prove_latency_ms" if arm["mode"] == "prove" else "op_latency_ms"][q] for x in rs), 2)
                                         for q in ("p50", "p99")},  # median over the runs; a prove-only op is its prove
                          failed=sum(x["failed"] for x in rs), rejected=sum(x["rejected"] for x in rs), shutdown_line=rs[-1]["shutdown_line"],
                          window_us=a.window_us, max_batch=a.max_batch, io_threads=a.io_threads, server_hw_queues=a.hwq,
                          engine="stub (not a measurement)" if a.stub else "libbbp_hip.so"))
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=2048)
    ap.add_argument("--ops", type=int, default=16384)
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--window-us", type=int, default=300)
    ap.add_argument("--max-batch", type=int, default=4096)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--rate", type=float, default=0.0, help="open loop: offered ops per second (Poisson arrivals)")
    ap.add_argument("--duration", type=float, default=10.0, help="open loop: seconds of arrivals")
    ap.add_argument("--sweep", default="", help="open loop: comma-separated offered loads, one run each against the same server")
    ap.add_argument("--io-threads", type=int, default=2)
    ap.add_argument("--gen-threads", type=int, default=2)
    ap.add_argument("--preconnect", type=int, default=0, help="open loop: connections opened before the clock starts")
    ap.add_argument("--verify-aggregate", type=int, default=0, help="server --verify-aggregate G (0 = one MSM per proof like the reference)")
    ap.add_argument("--hwq", type=int, default=int(os.environ.get("BBP_SERVER_HWQ", "2")), choices=(1, 2), help="GPU_MAX_HW_QUEUES of the server process")
    ap.add_argument("--devices", default="0", help="server --devices list (a,b,..: device pool)")
    ap.add_argument("--depth", type=int, default=1, help="closed loop: independent ops every connection keeps outstanding")
    ap.add_argument("--pipeline-depth", type=int, default=0, help="server --pipeline-depth (0 = the server's default)")
    ap.add_argument("--max-inflight", type=int, default=0, help="server --max-inflight (0 = the server's default)")
    ap.add_argument("--pipelining", action="store_true", help="run the (connections, depth) matrix, alternating the arms over --runs runs")
    ap.add_argument("--runs", type=int, default=5, help="--pipelining: runs per arm")
    ap.add_argument("--arms", default="", help="--pipelining: only the arms whose name contains one of these comma-separated strings")
    ap.add_argument("--parent-server", default="", help="--pipelining: a bbp-uds-server built from the parent commit, for the no-regression arms")
    ap.add_argument("--arm-timeout", type=float, default=120.0, help="--pipelining: time limit of one arm's load run, seconds")
    ap.add_argument("--out", default="", help="--pipelining: JSONL file for the per-arm summaries (default: standard output only)")
    ap.add_argument("--stub", action="store_true", help="CPU box: the tests' stub engine (plumbing check, not a measurement)")
    a = ap.parse_args()
    ge.build_server()
    if a.pipelining:
        return pipelining(a)
    d = tempfile.mkdtemp(prefix="bbp-uds-bench-")
    sock, reqs = os.path.join(d, "sock"), os.path.join(d, "bids.bin")
    N = a.items
    engine, bids = make_bids(a, N, a.distinct)
    write_requests(reqs, bids, N)
    log = open(os.path.join(d, "server.log"), "w+")
    srv = subprocess.Popen([ge.SERVER_BIN, "-b", sock, "-l", "info", "--engine", engine, "--window-us", str(a.window_us), "--max-batch",
                            str(a.max_batch), "--max-connections", str(max(4096, 2 * a.connections)), "--io-threads", str(a.io_threads),
                            "--devices", a.devices, "--reserve", str(N)] + (["--pipeline-depth", str(a.pipeline_depth)] if a.pipeline_depth else []) +
                           (["--max-inflight", str(a.max_inflight)] if a.max_inflight else []) + (["--verify-aggregate", str(a.verify_aggregate)] if a.verify_aggregate else []), stderr=log, env=dict(os.environ, GPU_MAX_HW_QUEUES=str(a.hwq)))
    for _ in range(6000):
        if os.path.exists(sock) or srv.poll() is not None:
            break
        time.sleep(0.02)
    if not os.path.exists(sock):
        log.seek(0)
        sys.exit("server did not come up: " + log.read()[-500:])
    cmd = [ge.LOADGEN_BIN, "--socket", sock, "--requests", reqs, "--connections", str(a.connections), "--threads", str(a.gen_threads), "--depth", str(a.depth)]
    extra = ["--no-verify"] if a.no_verify else []
    warm = subprocess.run(cmd + ["--ops", str(min(a.ops, 2 * a.connections * a.depth))], capture_output=True, text=True)  # compile the circuit, grow buffers
    runs = []
    if a.sweep or a.rate > 0:
        for r in ([float(x) for x in a.sweep.split(",")] if a.sweep else [a.rate]):
            runs.append(subprocess.run(cmd + ["--rate", str(r), "--duration", str(a.duration), "--preconnect", str(a.preconnect)] + extra,
                                       capture_output=True, text=True))
    else:
        runs.append(subprocess.run(cmd + ["--ops", str(a.ops)] + extra, capture_output=True, text=True))
    srv.send_signal(signal.SIGTERM)
    srv.wait(timeout=60)
    log.seek(0)
    if os.environ.get("BBP_TRACE"):
        sys.stderr.write("".join([ln for ln in log.read().splitlines(True) if "trace" in ln][:int(os.environ.get("BBP_TRACE_HEAD", "0")) or None][-int(os.environ.get("BBP_TRACE_TAIL", "40")):]))
        log.seek(0)
    text = log.read()
    m = re.search(r"served (\d+) requests \((\d+) errors\) in (\d+) device calls, largest batch (\d+)(?:, deepest pipeline (\d+))?", text)
    for run in runs:
        out = json.loads(run.stdout.strip().splitlines()[-1]) if run.stdout.strip() else {"error": run.stderr[-300:], "warmup": warm.stderr[-300:]}
        out.update(workload="configs[4] through the UDS server: %s per connection" % ("prove only" if a.no_verify else "prove then verify"), bid_list_len=N,
                   window_us=a.window_us, max_batch=a.max_batch, pipeline_depth=a.pipeline_depth or "server default", io_threads=a.io_threads, devices=a.devices, server_hw_queues=a.hwq, verify_aggregate=a.verify_aggregate,
                   engine="stub (not a measurement)" if a.stub else "libbbp_hip.so")
        if m and len(runs) == 1:
            out["server"] = dict(requests=int(m.group(1)), errors=int(m.group(2)), device_calls=int(m.group(3)), largest_batch=int(m.group(4)))
            if m.group(5):
                out["server"]["deepest_pipeline"] = int(m.group(5))
        print(json.dumps(out), flush=True)
    if "ERROR" in text and os.environ.get("BBP_SHOW_SERVER_ERRORS"):
        sys.stderr.write(text[-2000:])


if __name__ == "__main__":
    main()
