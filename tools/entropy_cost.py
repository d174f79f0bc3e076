"""What the entropy source costs a host-pointer caller (include/bbp.h bbp_set_entropy_source): bbp_prove_batch without caller
entropy, B = 1024, N in {8, 202}, source OS (the calling thread reads /dev/urandom and wide-reduces every blinding on the host) against
DEVICE (one 32-byte OS key per call, ChaCha20 on the device), back-to-back calls from one thread and from two threads.  A third arm,
EXPLICIT, passes caller entropy (neither host draw nor device draw: what the engine does without any entropy work).  The arms
alternate in one process after warm-up, at least three rounds each.  One JSON line per case (proofs/s per round, medians, the ratios
device / os and device / explicit, ms per call of one thread) goes to stdout and to --out with the box id and the commit given on the command line.
--case NAME --arm device runs one case and arm alone (the kernel-trace pass that prices k_draw_entropy).  The arm HEDGED is source
HEDGED (each row's key bound to the row's inputs: k_hedge_keys, then the draw under per-row keys).

--margin OUT is the hedged source's own measurement: the arms OS, DEVICE and HEDGED in one process on one context, bbp_prove_batch with
entropy == NULL, B = 1024 and one proof at N = 8 and 202; the arms alternate, each figure is the best of 5 calls after 2 warm-ups, 5
runs per arm, reported as median and range in ms per call.  The rule (`within_margin`): HEDGED is not slower than DEVICE by more than
DEVICE's own range over its 5 runs.  `rng_us` is the device time of the TAG_RNG entries (bbp_set_profiling) of one
bbp_draw_entropy_dev / bbp_draw_entropy_hedged_dev of the same shape, best of 5 after 2: the plain draw, and the row keys and the draw
under them.  One JSON line per shape goes to stdout and to OUT."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab import box_id  # noqa: E402

CASES = [("n8_one_thread", 8, 1), ("n8_two_threads", 8, 2), ("n202_one_thread", 202, 1), ("n202_two_threads", 202, 2)]


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


def rng_times(ctx, bbp, torch, B, N, rows):
    """device microseconds of the TAG_RNG entries of one device-form draw, best of 5 after 2"""
    d_in = torch.frombuffer(bytearray(rows), dtype=torch.uint8).cuda()
    d_ent = torch.zeros(B * bbp.entropy_size(N), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {}
    for name, call, n in (("device_draw", lambda: ctx.draw_entropy_dev(B, N, bbp.ENTROPY_PROVE, d_ent.data_ptr()), 1),
                          ("hedged", lambda: ctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), d_ent.data_ptr()), 2)):
        ts = []
        for it in range(7):
            ctx.set_profiling(True)
            ctx.last_timings()
            call()
            t = [us for tag, us in ctx.last_timings() if tag == 4]
            ctx.set_profiling(False)
            assert len(t) == n, t
            if it >= 2:
                ts.append(t)
        if n == 1:
            res[name] = round(min(t[0] for t in ts), 1)
        else:
            res["hedge_keys"], res["hedged_draw"] = round(min(t[0] for t in ts), 1), round(min(t[1] for t in ts), 1)
    return res


def margin(ctx, bbp, torch, synth, args):
    box = box_id()
    arms = ("os", "device", "hedged")
    with open(args.margin, "w") as f:
        for N in (8, 202):
            ins, _, _ = synth(ctx, args.batch, N, seed=1600 + N)
            for B in (args.batch, 1):
                rows = b"".join(ins[:B])
                ctx.reserve(B, N)

                def call():
                    _o, st = ctx.prove_batch(B, N, rows)
                    assert st == [0] * B
                runs = {a: [] for a in arms}
                try:
                    for _ in range(5):
                        for a in arms:
                            ctx.set_entropy_source(a)
                            runs[a].append(best_of(call))
                finally:
                    ctx.set_entropy_source("os")
                rec = {"N": N, "B": B, "unit": "ms per call, best of 5 after 2 warm-ups, 5 runs", "box": box, "commit": args.commit}
                for a in arms:
                    v = runs[a]
                    rec[a] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                rec["hedged_minus_device_ms"] = round(rec["hedged"]["median"] - rec["device"]["median"], 3)
                rec["device_range_ms"] = round(rec["device"]["max"] - rec["device"]["min"], 3)
                rec["within_margin"] = rec["hedged"]["median"] - rec["device"]["median"] <= rec["device"]["max"] - rec["device"]["min"]
                rec["rng_us"] = rng_times(ctx, bbp, torch, B, N, rows)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the arms (>= 3)")
    ap.add_argument("--calls", type=int, default=4, help="bbp_prove_batch calls per thread, arm and round")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None)
    ap.add_argument("--arm", choices=["os", "device", "hedged", "explicit", "all"], default="all")
    ap.add_argument("--margin", default=None, metavar="OUT", help="the OS / DEVICE / HEDGED latency comparison (see above) into OUT")
    ap.add_argument("--commit", default=os.environ.get("BBP_COMMIT", "unknown"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_device_entropy.jsonl"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests.test_gpu_prove_verify import _synth_batch

    ctx = bbp.Context(0)
    if args.margin:
        margin(ctx, bbp, torch, _synth_batch, args)
        flags = ctx.health()
        ctx.close()
        assert flags == 0, "engine health flags %#x" % flags
        return
    B = args.batch
    arms = ["os", "device", "hedged", "explicit"] if args.arm == "all" else [args.arm]
    cases = [c for c in CASES if args.case in (None, c[0])]
    inputs, entropy = {}, {}
    for N in sorted({c[1] for c in cases}):
        ins, ents, _ = _synth_batch(ctx, B, N, seed=1600 + N)
        inputs[N], entropy[N] = b"".join(ins), b"".join(ents)
        ctx.reserve(B, N)  # every buffer exists before the first timed call
    box = box_id()
    lines = []

    def run(arm, N, threads, calls):
        ctx.set_entropy_source("os" if arm == "explicit" else arm)
        ent = entropy[N] if arm == "explicit" else None
        errs = []

        def worker():
            try:
                for _ in range(calls):
                    _o, st = ctx.prove_batch(B, N, inputs[N], ent)
                    if st != [0] * B:
                        errs.append("statuses")
            except Exception as ex:  # noqa: BLE001
                errs.append(repr(ex))
        th = [threading.Thread(target=worker) for _ in range(threads)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        ctx.set_entropy_source("os")
        assert not errs, errs
        return dt

    for name, N, threads in cases:
        for arm in arms:
            run(arm, N, threads, 2)  # warm-up
        rates = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm in arms:
                dt = run(arm, N, threads, args.calls)
                rates[arm].append(threads * B * args.calls / dt)
        row = {"case": name, "B": B, "N": N, "threads": threads, "calls_per_thread": args.calls, "box": box, "commit": args.commit,
               "arms": {a: [round(x, 1) for x in xs] for a, xs in rates.items()},
               "median": {a: round(statistics.median(xs), 1) for a, xs in rates.items()},
               "ms_per_call_per_thread": {a: round(1e3 * threads * B / statistics.median(xs), 2) for a, xs in rates.items()}}
        med = {a: statistics.median(xs) for a, xs in rates.items()}
        if "device" in med and "os" in med:
            row["ratio_device_over_os"] = round(med["device"] / med["os"], 4)
        if "device" in med and "explicit" in med:
            row["ratio_device_over_explicit"] = round(med["device"] / med["explicit"], 4)
        if "hedged" in med and "device" in med:
            row["ratio_hedged_over_device"] = round(med["hedged"] / med["device"], 4)
        print(json.dumps(row), flush=True)
        lines.append(row)
    flags = ctx.health()
    ctx.close()
    assert flags == 0, "engine health flags %#x" % flags
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
