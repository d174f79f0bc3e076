"""What the entropy source costs a host-pointer caller (include/bbp.h bbp_set_entropy_source): bbp_prove_batch without caller
entropy, B = 1024, N in {8, 202}, source OS (the calling thread reads /dev/urandom and wide-reduces every blinding on the host) against
DEVICE (one 32-byte OS key per call, ChaCha20 on the device), back-to-back calls from one thread and from two threads.  A third arm,
EXPLICIT, passes caller entropy (neither host draw nor device draw: what the engine does without any entropy work).  The arms
alternate in one process after warm-up, at least three rounds each.  One JSON line per case (proofs/s per round, medians, the ratios
device / os and device / explicit, ms per call of one thread) goes to stdout and to --out with the box id and the commit given on the command line.
--case NAME --arm device runs one case and arm alone (the kernel-trace pass that prices k_draw_entropy)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the arms (>= 3)")
    ap.add_argument("--calls", type=int, default=4, help="bbp_prove_batch calls per thread, arm and round")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None)
    ap.add_argument("--arm", choices=["os", "device", "explicit", "all"], default="all")
    ap.add_argument("--commit", default=os.environ.get("BBP_COMMIT", "unknown"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_device_entropy.jsonl"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests.test_gpu_prove_verify import _synth_batch

    ctx = bbp.Context(0)
    B = args.batch
    arms = ["os", "device", "explicit"] if args.arm == "all" else [args.arm]
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
