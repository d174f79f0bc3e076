#!/usr/bin/env python3
"""Which of the prover's streams lands on which HARDWARE QUEUE during bench.py's timed region, and how busy each is, from one
`rocprofv3 --kernel-trace --output-format csv` run of bench.py (the program itself after `--`, BBP_BENCH_NO_RESERVE=1 in front as
in tools/prof.sh):

    python tools/prove_queue_map.py <x_kernel_trace.csv> [> profiles/NAME.txt]

The timed region is what follows the last k_ubench launch (bench.py measures its ALU ceilings between warm-up and timed steps).
Per stream: Queue_Id(s), launches, the share of the region in which the stream has a kernel running, and the kernels that tell
what the stream is (k_open_serial / k_open_bulk50 / k_reduce_draws = an opening stage, k_msm_acc = a heavy stage; both = a chain,
BBP_OPEN_ON_CHAIN).  Then, per queue, the streams that share it.  Streams are listed by Stream_Id, i.e. in creation order: the
context creates stream, side, lane[1], lane[2], lane[3], copy, side2, then the verifier lanes (setup.hip)."""
import collections, csv, sys


def short(name):
    return name.split("(")[0].replace("void ", "").replace("bbp::", "").split("<")[0][:24]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    for r in rows:
        r["a"], r["b"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    ub = [r["b"] for r in rows if "k_ubench" in r["Kernel_Name"]]
    t0 = max(ub) if ub else min(r["a"] for r in rows)
    reg = [r for r in rows if r["a"] >= t0]
    t0, t1 = min(r["a"] for r in reg), max(r["b"] for r in reg)
    per = collections.defaultdict(lambda: {"q": collections.Counter(), "iv": [], "k": collections.Counter()})
    for r in reg:
        s = per[r["Stream_Id"]]
        s["q"][r["Queue_Id"]] += 1
        s["iv"].append((r["a"], r["b"]))
        s["k"][short(r["Kernel_Name"])] += 1
    print("timed region: %.1f ms, %d launches on %d streams" % ((t1 - t0) / 1e6, len(reg), len(per)))
    print("%-7s %-10s %8s %9s %7s  %-8s %s" % ("stream", "queue(s)", "launches", "busy ms", "share", "stage", "most frequent kernels"))
    by_queue = collections.defaultdict(list)
    for sid, s in sorted(per.items(), key=lambda kv: int(kv[0])):
        busy, end = 0, 0
        for a, b in sorted(s["iv"]):  # union of the launches' intervals
            if b > end:
                busy += b - max(a, end)
                end = b
        opens = any(k.startswith(("k_open_", "k_reduce_draws")) for k in s["k"])
        heavy = "k_msm_acc" in s["k"]
        for q in s["q"]:
            by_queue[q].append(sid)
        print("%-7s %-10s %8d %9.1f %6.1f%%  %-8s %s" % (sid, ",".join(q for q, _ in s["q"].most_common()), len(s["iv"]), busy / 1e6, 100.0 * busy / (t1 - t0),
                                                     "chain" if opens and heavy else "opening" if opens else "heavy" if heavy else "-",
                                                     ", ".join("%s x%d" % kv for kv in s["k"].most_common(3))))
    shared = {q: v for q, v in sorted(by_queue.items(), key=lambda kv: int(kv[0])) if len(v) > 1}
    print("queues shared by several streams:", shared or "none")


if __name__ == "__main__":
    main()
