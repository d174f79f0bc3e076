"""What checked proving costs (include/bbp.h bbp_set_prove_check): unchecked and checked arms alternated in one process, after
warm-up, at least three times each; proofs/s per arm and the ratio checked / unchecked for
  (a) the device API, B = 1024, N = 8, calls enqueued back to back over three input / output sets as bench.py's prove workload
      keeps them (bbp_prove_batch_dev against bbp_prove_batch_checked_dev)
  (b) bbp_prove_batch, B = 1024, from two host threads (checking off / on)
  (c) one bbp_prove: latency (median of the arm's calls)
Prints one JSON line per case and a summary.  --only a runs (a) alone with --arm checked|unchecked (a kernel-trace run)."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two arms (>= 3)")
    ap.add_argument("--steps", type=int, default=12, help="(a) device calls per arm and round")
    ap.add_argument("--host-calls", type=int, default=6, help="(b) bbp_prove_batch calls per thread, arm and round")
    ap.add_argument("--single", type=int, default=20, help="(c) bbp_prove calls per arm and round")
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--arm", choices=["checked", "unchecked", "both"], default="both")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests.test_gpu_prove_verify import _synth_batch

    ctx = bbp.Context(0)
    B, N = 1024, 8
    rs_ = bbp.record_size(N)
    ins, ents, _ = _synth_batch(ctx, B, N, seed=2024)
    ctx.set_prove_check(True)
    ctx.reserve(B, N)  # every buffer of both arms exists before the first timed call
    ctx.set_prove_check(False)
    arms = ["unchecked", "checked"] if args.arm == "both" else [args.arm]
    results = {}

    if args.only in (None, "a"):
        dev = torch.device("cuda", 0)
        stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
        sets = []
        for k in range(3):
            rows = ins[k:] + ins[:k]
            er = ents[k:] + ents[:k]
            sets.append((torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev),
                         torch.frombuffer(bytearray(b"".join(er)), dtype=torch.uint8).to(dev),
                         torch.frombuffer(bytearray(os.urandom(32 * B)), dtype=torch.uint8).to(dev),
                         torch.zeros(B * rs_, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize()

        def run_a(arm, steps):
            for j in range(steps):
                i, e, ce, o, st = sets[j % 3]
                if arm == "checked":
                    ctx.prove_batch_checked_dev(B, N, i.data_ptr(), e.data_ptr(), ce.data_ptr(), o.data_ptr(), st.data_ptr(), stream.cuda_stream)
                else:
                    ctx.prove_batch_dev(B, N, i.data_ptr(), e.data_ptr(), o.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
        for arm in arms:
            run_a(arm, 4)  # warm-up
        rates = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm in arms:
                t0 = time.perf_counter()
                run_a(arm, args.steps)
                rates[arm].append(B * args.steps / (time.perf_counter() - t0))
        if "checked" in arms:
            bad = [int((st != 0).sum()) for *_x, st in sets]
            assert bad == [0, 0, 0], "checked arm reported non-OK rows: %s" % bad
        results["a_device_api_b1024_n8"] = rates

    if args.only in (None, "b"):
        blob, eblob = b"".join(ins), b"".join(ents)

        def run_b(arm, calls):
            ctx.set_prove_check(arm == "checked")
            errs = []

            def worker():
                try:
                    for _ in range(calls):
                        _o, st = ctx.prove_batch(B, N, blob, eblob)
                        if st != [0] * B:
                            errs.append("statuses")
                except Exception as ex:  # noqa: BLE001
                    errs.append(repr(ex))
            th = [threading.Thread(target=worker) for _ in range(2)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            ctx.set_prove_check(False)
            assert not errs, errs
        for arm in arms:
            run_b(arm, 2)
        rates = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm in arms:
                t0 = time.perf_counter()
                run_b(arm, args.host_calls)
                rates[arm].append(2 * B * args.host_calls / (time.perf_counter() - t0))
        results["b_prove_batch_b1024_two_threads"] = rates

    if args.only in (None, "c"):
        s7, pub, tg, e = ins[0][:224], ins[0][224:224 + 32 * N], 0, ents[0]

        def run_c(arm, calls):
            ctx.set_prove_check(arm == "checked")
            lat = []
            for _ in range(calls):
                t0 = time.perf_counter()
                ctx.prove(s7, pub, tg, e)
                lat.append((time.perf_counter() - t0) * 1e3)
            ctx.set_prove_check(False)
            return lat
        for arm in arms:
            run_c(arm, 3)
        lat = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm in arms:
                lat[arm].append(statistics.median(run_c(arm, args.single)))
        results["c_single_prove_latency_ms"] = lat

    summary = {}
    for case, v in results.items():
        row = {"case": case, "arms": {a: [round(x, 1) for x in xs] for a, xs in v.items()},
               "median": {a: round(statistics.median(xs), 2) for a, xs in v.items()}}
        if len(v) == 2:
            row["ratio_checked_over_unchecked"] = round(statistics.median(v["checked"]) / statistics.median(v["unchecked"]), 4)
        print(json.dumps(row), flush=True)
        summary[case] = row.get("ratio_checked_over_unchecked")
    print(json.dumps({"summary": summary, "health": ctx.health(), "check_stats": ctx.prove_check_stats()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
