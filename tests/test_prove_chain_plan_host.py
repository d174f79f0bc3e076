"""not-gpu tier: the rule that puts a rotating prove call's opening stage on the stream of its heavy stage (csrc/prove_plan.h:
ProveKnobs::open_on_chain / hw_queues, ProvePlan::open_on_chain / chain_stream), through tests/prove_chain_check.cpp, a host program
of its own built with the system compiler under AddressSanitizer + UBSan and run as it is.  Expected values are literals worked out
from the rule as DESIGN.md section 4 states it."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "prove_chain_check.cpp")
BIN = os.path.join(ROOT, "tests", "_build", "prove_chain_check")
CALLER, SIDE, LANE1, LANE2, LANE3, COPY, SIDE2 = range(7)  # StreamRole


@pytest.fixture(scope="module")
def prog():
    hdr = os.path.join(ROOT, "dusk_blindbidproof_amd", "csrc", "prove_plan.h")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", BIN, SRC])

    def run(lines):
        """one process for a whole script; a plan (dict) per `call` line"""
        p = subprocess.run([BIN], input="".join(ln + "\n" for ln in lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        plans = []
        for ln in p.stdout.decode().splitlines():
            old, new, trace = ln.split(" | ")
            on, chain_stream, roles, raw = (int(x) for x in new.split())
            plans.append(dict(old=old, trace=trace, deep=int(old.split()[1]), rotate=int(old.split()[11]), heavy_stream=int(old.split()[12]), on=on, chain_stream=chain_stream,
                              roles={r for r in range(7) if roles >> r & 1}, raw=raw))
        assert len(plans) == sum(ln.startswith("call") for ln in lines)
        return plans

    return run


# which (B, inflight) rotate under the default knobs: up to 1023 proofs always, up to 4096 with three calls in flight (deep mode)
ROTATES = {(1, 0): 1, (1, 3): 1, (64, 0): 1, (64, 3): 1, (767, 0): 1, (767, 3): 1, (1024, 0): 0, (1024, 3): 1, (4097, 0): 0, (4097, 3): 0}
# ... and which are planned deep: the ones that find three calls in flight, up to 4096 proofs
DEEP = {(1, 0): 0, (1, 3): 1, (64, 0): 0, (64, 3): 1, (767, 0): 0, (767, 3): 1, (1024, 0): 0, (1024, 3): 1, (4097, 0): 0, (4097, 3): 0}
# the rule for a rotating call, by (hw_queues, knob): 1 = every rotating call; unset = below seven queues, and then the deep ones only
RULE = {(2, -1): 1, (4, -1): 1, (6, -1): 1, (7, -1): 0, (16, -1): 0,
        (2, 0): 0, (4, 0): 0, (6, 0): 0, (7, 0): 0, (16, 0): 0,
        (2, 1): 1, (4, 1): 1, (6, 1): 1, (7, 1): 1, (16, 1): 1}
# call index -> heavy_stream -> the chain's stream and its draw buffer
CHAIN_OF_CALL = {0: (1, LANE1, 2), 1: (2, LANE2, 3), 2: (3, SIDE, 0)}


def test_open_on_chain_and_chain_stream_tables(prog):
    lines, want = [], []
    for (hwq, knob), rule in RULE.items():
        for (B, inflight), rot in ROTATES.items():
            for first in range(3):
                lines += ["reset %d %d" % (hwq, knob)] + ["call 5000 0 0"] * first + ["call %d %d 0" % (B, inflight)]
                want += [None] * first + [(hwq, knob, B, inflight, first, rot, rule)]
    for p, w in zip(prog(lines), want):
        if w is None:
            continue
        hwq, knob, B, inflight, first, rot, rule = w
        rule = rule and (knob == 1 or DEEP[(B, inflight)])
        assert p["deep"] == DEEP[(B, inflight)], w
        hs, role, raw = CHAIN_OF_CALL[first]
        assert p["rotate"] == rot, w
        assert p["on"] == (rot and rule), w
        assert p["chain_stream"] == (role if rot and rule else -1), w
        if rot:
            assert p["heavy_stream"] == hs, w
            assert p["roles"] == ({CALLER, role} if rule else {CALLER, SIDE2 if first & 1 else SIDE, LANE1 + hs - 1}), w
            assert p["raw"] == (raw if rule else first & 1), w


SIZES = [1, 31, 64, 130, 511, 512, 767, 768, 1023, 1024, 2048, 4096, 4097]


def test_every_earlier_field_is_what_the_knob_off_plan_has(prog):
    rng = random.Random(20261019)
    seqs = [[(rng.choice(SIZES), rng.choice([0, 0, 1, 2, 3, 4]), rng.randrange(2)) for _ in range(rng.randrange(1, 13))] for _ in range(2000)]
    script = {arm: [] for arm in ("off", "on", "unset4", "unset8")}
    for seq in seqs:
        calls = ["call %d %d %d" % c for c in seq]
        script["off"] += ["reset 4 0"] + calls
        script["on"] += ["reset 4 1"] + calls
        script["unset4"] += ["reset 4 -1"] + calls
        script["unset8"] += ["reset 8 -1"] + calls
    plans = {arm: prog(lines) for arm, lines in script.items()}
    assert len(plans["off"]) == sum(len(s) for s in seqs) > 10000
    for arm in ("on", "unset4", "unset8"):
        assert [(p["old"], p["trace"]) for p in plans[arm]] == [(p["old"], p["trace"]) for p in plans["off"]], arm
    assert [(p["on"], p["roles"]) for p in plans["unset8"]] == [(p["on"], p["roles"]) for p in plans["off"]]
    # unset below seven queues: a rotating call planned deep is what the knob-on plan is, any other call what the knob-off plan is
    assert any(p["rotate"] and not p["deep"] for p in plans["off"]) and any(p["rotate"] and p["deep"] for p in plans["off"])
    for u, p, q in zip(plans["unset4"], plans["on"], plans["off"]):
        assert u["on"] == (u["rotate"] and u["deep"])
        assert (u["chain_stream"], u["roles"], u["raw"]) == tuple((p if u["on"] else q)[k] for k in ("chain_stream", "roles", "raw"))
    assert any(p["on"] for p in plans["on"]) and not any(p["on"] for p in plans["off"])
    # with the rule on a call stays on the first four streams the context creates; a rotating one on the caller's and one chain
    for p, q in zip(plans["on"], plans["off"]):
        assert p["on"] == p["rotate"]
        if p["rotate"]:
            assert len(p["roles"]) == 2 and p["roles"] <= {CALLER, SIDE, LANE1, LANE2}
            assert p["raw"] == {SIDE: 0, LANE1: 2, LANE2: 3}[p["chain_stream"]]
        else:
            assert (p["roles"], p["raw"]) == (q["roles"], q["raw"])  # a sliced call is what it was
    # ... whereas the two-stream form reaches the fifth and the seventh
    assert any(LANE3 in p["roles"] for p in plans["off"]) and any(SIDE2 in p["roles"] for p in plans["off"])


def test_three_consecutive_rotating_calls_take_three_chains(prog):
    for first in range(7):
        lines = ["reset 4 -1"] + ["call 2048 0 0"] * first + ["call 300 3 0", "call 1024 3 0", "call 33 0 0", "call 4096 1 0"]
        p = prog(lines)[first:]
        assert all(q["on"] for q in p)
        for i in range(2):
            assert {q["chain_stream"] for q in p[i:i + 3]} == {SIDE, LANE1, LANE2}
            assert len({q["raw"] for q in p[i:i + 3]}) == 3  # ... and three draw buffers
    # four slices (BBP_SLICES=4) put a slice on lane[3]; rotating calls still keep to the three chain streams
    p = prog(["reset 4 1 BBP_SLICES 4", "call 4096 0 0", "call 100 0 0", "call 100 0 0", "call 100 0 0"])
    assert p[0]["roles"] == {CALLER, SIDE, LANE1, LANE2, LANE3} and [q["chain_stream"] for q in p[1:]] == [LANE2, SIDE, LANE1]
