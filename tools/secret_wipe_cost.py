#!/usr/bin/env python3
"""What secret wiping costs (include/bbp.h "Secret wiping"), measured on the device:

    python tools/secret_wipe_cost.py profiles/r17_secret_wipe.jsonl [--runs 5] [--quick]

Arms off / on alternate in ONE process on ONE context (the switch is flipped between timed windows), `runs` windows per arm; a window
is a host clock around calls that end in a device synchronise.  Cases:
  - device-resident bbp_prove_batch_dev at B = 1024 and 256, N = 8 and 202, three calls in flight (a call is enqueued once the call
    three back has finished), all-zero rows and entropy (what bbp_reserve proves: the schedule does not depend on the data);
  - one proof through the host API (bbp_prove_batch of one row).
Per case one JSON line: ms per call for both arms (median, min, max over the windows), the difference of the medians, and for the
wipe by itself (bbp_debug_wipe_cost after ONE call of the shape on the otherwise idle device, wiping on):
  - wiped_bytes, wipe_launches: what that call's own wipes stored, in how many k_wipe_spans launches (the engine's log of its span lists);
  - lone_wipe_us: the device time (events) of ONE k_wipe_spans launch over exactly those spans on the idle device, `runs` times.
ratio = (on - off) / lone wipe is the acceptance figure of DESIGN.md "Secret wiping": above 2, the section says which stream waits
and for what.  --quick: B = 256, N = 8 and the single proof only.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0]
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5
    quick = "--quick" in sys.argv
    import torch
    import dusk_blindbidproof_amd as bbp
    torch.cuda.init()
    lines = []

    def device_case(B, N, calls):
        ctx = bbp.Context(0)
        es = torch.cuda.ExternalStream(ctx.stream, device=torch.device("cuda:0"))
        rows = torch.zeros(B * (7 * 32 + 32 * N + 8), dtype=torch.uint8, device="cuda")
        ent = torch.zeros(B * bbp.entropy_size(N), dtype=torch.uint8, device="cuda")
        outs = [torch.zeros(B * bbp.record_size(N), dtype=torch.uint8, device="cuda") for _ in range(3)]
        evs = [torch.cuda.Event() for _ in range(3)]
        torch.cuda.synchronize()

        def window(n):
            t0 = time.perf_counter()
            for k in range(n):
                if k >= 3:
                    evs[k % 3].synchronize()  # three calls in flight
                ctx.prove_batch_dev(B, N, rows.data_ptr(), ent.data_ptr(), outs[k % 3].data_ptr())
                evs[k % 3].record(es)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n
        ms = {False: [], True: []}
        for on in (False, True):  # every shape of both arms warm: buffers of the rotation, code objects
            ctx.set_secret_wipe(on)
            window(8)
        for r in range(runs):
            for on in ((False, True) if r % 2 == 0 else (True, False)):
                ctx.set_secret_wipe(on)
                ms[on].append(window(calls))
        ctx.set_secret_wipe(True)
        ctx.wipe_secrets()  # empties the wipe log
        window(1)
        wiped = ctx.debug_wipe_cost()
        lone = [ctx.debug_wipe_cost()[2] for _ in range(runs)]
        del es, evs
        ctx.close()
        return ms, lone, wiped

    def host_case(N, calls):
        ctx = bbp.Context(0)
        row, ent = bytes(7 * 32 + 32 * N + 8), bytes(bbp.entropy_size(N))

        def window(n):
            t0 = time.perf_counter()
            for _ in range(n):
                ctx.prove_batch(1, N, row, ent)  # returns after its results (and, when on, its wipes) are complete
            return (time.perf_counter() - t0) * 1e3 / n
        ms = {False: [], True: []}
        for on in (False, True):
            ctx.set_secret_wipe(on)
            window(6)
        for r in range(runs):
            for on in ((False, True) if r % 2 == 0 else (True, False)):
                ctx.set_secret_wipe(on)
                ms[on].append(window(calls))
        ctx.set_secret_wipe(True)
        ctx.wipe_secrets()  # empties the wipe log
        window(1)
        wiped = ctx.debug_wipe_cost()
        lone = [ctx.debug_wipe_cost()[2] for _ in range(runs)]
        ctx.close()
        return ms, lone, wiped

    cases = [("prove_batch_dev, three in flight", 256, 8, 24)] if quick else [
        ("prove_batch_dev, three in flight", 1024, 8, 18), ("prove_batch_dev, three in flight", 256, 8, 24),
        ("prove_batch_dev, three in flight", 1024, 202, 9), ("prove_batch_dev, three in flight", 256, 202, 12)]
    for name, B, N, calls in cases:
        ms, lone, wiped = device_case(B, N, calls)
        lines.append((name, B, N, calls, ms, lone, wiped))
    ms, lone, wiped = host_case(8, 12)
    lines.append(("bbp_prove_batch, one proof, host API", 1, 8, 12, ms, lone, wiped))
    with open(out, "w") as f:
        for name, B, N, calls, ms, lone, wiped in lines:
            off, on, lw = stats(ms[False]), stats(ms[True]), stats(lone)
            diff = on["median"] - off["median"]
            rec = {"case": name, "B": B, "N": N, "runs_per_arm": runs, "calls_per_window": calls, "ms_per_call_off": off, "ms_per_call_on": on,
                   "on_minus_off_ms": round(diff, 4), "wiped_bytes": wiped[0], "wipe_launches": wiped[1], "lone_wipe_us": lw,
                   "ratio": round(diff * 1e3 / lw["median"], 3)}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
