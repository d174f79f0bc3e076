"""What the blinding draw costs a prove call (include/bbp.h bbp_set_blinding_draw): MERLIN, the Keccak draw chain, against EXPANDED,
one key per proof and a flat ChaCha20 launch.  The two modes alternate in one process on one context; each figure is the best of 5
timed groups after 2 warm-ups, 5 runs per mode, reported as median and range in ms per call.  The shapes:
  single        one proof through the host API (tools/latency.py's shape), N = 8
  b2b_<B>       back-to-back bbp_prove_batch_dev calls of B proofs, 4 per group, one synchronise (tools/midsize.py's shape), N = 8
  step_n<N>     the 1024-proof step, 6 calls enqueued without synchronisation (three and more in flight), N = 8 and 202
  stream        bench_workloads.py's streaming shape in chunks of 1024, 6 chunks and the drain per group, N = 8
Every timed call's records are checked by the device verifier after the timed region (the stream shape verifies its own chunks).
The rule (`within_margin`): EXPANDED is not slower than MERLIN by more than MERLIN's own range over its 5 runs.  One JSON line per shape
goes to stdout and to --out with the box id and the commit given on the command line.

--trace-loop MODE runs 4 lone 1024-proof calls at N = 8 in MODE and nothing else: the program of a kernel-trace pass of its own
(rocprofv3 --kernel-trace --stats -- python tools/blinding_draw.py --trace-loop expanded), which prices k_open_key, k_expand_draws and
k_witness_gates against k_open_serial / k_open_bulk50 / k_reduce_draws."""
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

MODES = ("merlin", "expanded")


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


class DevBatch:
    """`group` prove_batch_dev calls of B proofs enqueued back to back, one synchronise; an output buffer per call, verified afterwards"""

    def __init__(self, ctx, bbp, torch, synth, B, N, group):
        self.ctx, self.bbp, self.torch, self.B, self.N, self.group = ctx, bbp, torch, B, N, group
        dev = torch.device("cuda", 0)
        ins, ents, vins = synth(ctx, B, N, seed=2800 + N)
        up = lambda data: torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        self.d_in, self.d_ent = up(b"".join(ins)), up(b"".join(ents))
        self.tails = up(b"".join(b"".join(v) for v in vins)).view(B, 96 + 32 * N)
        self.outs = [torch.zeros(B * bbp.record_size(N), dtype=torch.uint8, device=dev) for _ in range(group)]
        self.d_vent = up(os.urandom(32 * B))
        self.d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
        ctx.reserve(B, N)
        torch.cuda.synchronize()

    def call(self):
        s = self.torch.cuda.current_stream().cuda_stream
        for o in self.outs:
            self.ctx.prove_batch_dev(self.B, self.N, self.d_in.data_ptr(), self.d_ent.data_ptr(), o.data_ptr(), s)
        self.torch.cuda.synchronize()

    def check(self):
        rs_ = self.bbp.record_size(self.N)
        for o in self.outs:
            vin = self.torch.cat([o.view(self.B, rs_), self.tails], dim=1).contiguous()
            self.d_st.fill_(-1)
            self.torch.cuda.synchronize()
            self.ctx.verify_batch_dev(self.B, self.N, vin.data_ptr(), self.d_vent.data_ptr(), self.d_st.data_ptr())
            self.torch.cuda.synchronize()
            assert int((self.d_st != 0).sum()) == 0, "a timed call's record failed the device verifier"
            o.zero_()
        self.torch.cuda.synchronize()


class Single:
    group = 1

    def __init__(self, ctx, synth, N):
        self.ctx, self.N = ctx, N
        ins, ents, vins = synth(ctx, 1, N, seed=2899)
        self.s7, self.pub, self.ent, self.v, self.rec = ins[0][:224], ins[0][224:224 + 32 * N], ents[0], vins[0], None
        ctx.reserve(1, N)

    def call(self):
        self.rec = self.ctx.prove(self.s7, self.pub, 0, self.ent)

    def check(self):
        assert self.ctx.verify(self.rec, *self.v) == 0


class Stream:
    def __init__(self, ctx, bbp, torch, B, N, group):
        import bench_workloads as bw
        self.torch, self.group = torch, group
        ctx.reserve(B, N)
        self.wl = bw.make_workload("stream", ctx, bbp, torch, torch.device("cuda", 0), B, N, 28)
        self.eng = torch.cuda.ExternalStream(ctx.stream, device=torch.device("cuda", 0))  # bench.py's engine stream: the context's own

    def call(self):
        with self.torch.cuda.stream(self.eng):
            for _ in range(self.group):
                self.wl.step(self.eng.cuda_stream)
            self.wl.drain()
        self.torch.cuda.synchronize()

    def check(self):
        assert self.wl.failed == 0, "%d chunk verifications failed" % self.wl.failed


def measure(ctx, name, shape, args, box, f):
    runs = {m: [] for m in MODES}
    try:
        for _ in range(5):
            for m in MODES:
                ctx.set_blinding_draw(m)
                runs[m].append(best_of(shape.call) / shape.group)
                shape.check()
    finally:
        ctx.set_blinding_draw("merlin")
    rec = {"shape": name, "unit": "ms per call, best of 5 groups of %d after 2 warm-ups, 5 runs" % shape.group, "box": box, "commit": args.commit}
    for m in MODES:
        v = runs[m]
        rec[m] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    rec["expanded_minus_merlin_ms"] = round(rec["expanded"]["median"] - rec["merlin"]["median"], 3)
    rec["merlin_range_ms"] = round(rec["merlin"]["max"] - rec["merlin"]["min"], 3)
    rec["within_margin"] = rec["expanded"]["median"] - rec["merlin"]["median"] <= rec["merlin"]["max"] - rec["merlin"]["min"]
    line = json.dumps(rec)
    print(line, flush=True)
    f.write(line + "\n")
    f.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="single,b2b_64,b2b_256,b2b_768,b2b_1024,step_n8,step_n202,stream")
    ap.add_argument("--trace-loop", choices=MODES, default=None)
    ap.add_argument("--commit", default=os.environ.get("BBP_COMMIT", "unknown"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_expanded_draw.jsonl"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import dusk_blindbidproof_amd as bbp
    from tests.test_gpu_prove_verify import _synth_batch

    ctx = bbp.Context(0)
    if args.trace_loop:
        shape = DevBatch(ctx, bbp, torch, _synth_batch, 1024, 8, 1)
        ctx.set_blinding_draw(args.trace_loop)
        for _ in range(4):
            shape.call()
        shape.check()
    else:
        box = box_id()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for name in args.shapes.split(","):
                if name == "single":
                    shape = Single(ctx, _synth_batch, 8)
                elif name.startswith("b2b_"):
                    shape = DevBatch(ctx, bbp, torch, _synth_batch, int(name[4:]), 8, 4)
                elif name.startswith("step_n"):
                    shape = DevBatch(ctx, bbp, torch, _synth_batch, 1024, int(name[6:]), 6)
                elif name == "stream":
                    shape = Stream(ctx, bbp, torch, 1024, 8, 6)
                else:
                    raise SystemExit("unknown shape %r" % name)
                measure(ctx, name, shape, args, box, f)
                del shape
    flags = ctx.health()
    ctx.close()
    assert flags == 0, "engine health flags %#x" % flags


if __name__ == "__main__":
    main()
