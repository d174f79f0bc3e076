"""GPU tier: verify round sharing (include/bbp.h bbp_set_verify_round_sharing; csrc/submit.cpp).  Concurrent bbp_verify /
bbp_verify_async requests that carry a byte-equal seed || pub_list leave the call combiner as one bbp_verify_rounds call whose table
holds every distinct round once.

Every status must be what the same request gets with sharing off, and what the existing calls report on the expanded rows.  That
requests did share is read from the totals of bbp_verify_round_sharing_stats (n_calls >= 1, n_rounds < n_rows), never from an exact
batch count: a straggler may miss the batching window.  Proofs are made by the engine under fixed entropy, a few per round, tiled.

Every child process a test starts runs under a time limit of its own, and nothing is retried."""
import json
import os
import subprocess
import sys
import tempfile
import threading

import pytest

from tests import oracle_c
from tests import verify_round_sharing_cases as rc
from tests.verify_combine_cases import burst, corrupt, to_json, two_phase

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT = 0, 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_US = 100000
L = rc.L


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def rounds(ctx, oc, bbp):
    """a, b, c: N = 8 -- b is a with one raw byte of list item 7 changed, c is a's list under another seed; one: N = 1; big: N = 202;
    lone: another N = 8 round (the singleton of the mixed burst)"""
    a = rc.Round(ctx, oc, bbp, 1, 8)
    return {"a": a,
            "b": rc.Round(ctx, oc, bbp, 2, 8, like=a, patch=(7, 5, 0x20)),
            "c": rc.Round(ctx, oc, bbp, 3, 8, like=a, seed=rc.seed_of(3)),
            "one": rc.Round(ctx, oc, bbp, 4, 1),
            "big": rc.Round(ctx, oc, bbp, 5, 202),
            "lone": rc.Round(ctx, oc, bbp, 6, 8, k=1)}


@pytest.fixture()
def sharing(ctx):
    """The shared context with a 100 ms batching window and round sharing on; afterwards as it was (no window, sharing off, mixing on,
    OS entropy)."""
    ctx.set_batching(WINDOW_US, 4096)
    ctx.set_verify_round_sharing(True)
    yield ctx
    ctx.set_batching(0, 0)
    ctx.set_verify_round_sharing(False)
    ctx.set_verify_mixing(True)
    ctx.set_entropy_source("os")


def _off_then_on(ctx, reqs):
    """The burst with sharing off, then with sharing on: (statuses off, statuses on, what the on burst added to the sharing counters)"""
    ctx.set_verify_round_sharing(False)
    before_off = ctx.verify_round_sharing_stats()
    off = burst(ctx, reqs)
    assert ctx.verify_round_sharing_stats() == before_off  # sharing off: no rounds call
    ctx.set_verify_round_sharing(True)
    before = ctx.verify_round_sharing_stats()
    on = burst(ctx, reqs)
    delta = tuple(x - y for x, y in zip(ctx.verify_round_sharing_stats(), before))
    print("off", off, "on", on, "rounds calls / rows / rounds", delta)
    return off, on, delta


def _shared(delta):
    return delta[0] >= 1 and delta[2] < delta[1]


def _expanded(reqs):
    return [len(r[4]) // 32 for r in reqs], b"".join(b"".join(r) for r in reqs)


def test_default_is_off_and_describe_reports_the_switch(ctx):
    assert "verify round sharing" not in ctx.describe()
    ctx.set_verify_round_sharing(True)
    try:
        assert "verify round sharing: on" in ctx.describe()
    finally:
        ctx.set_verify_round_sharing(False)
    assert "verify round sharing" not in ctx.describe()


def test_one_round_with_three_corrupted_requests(sharing, rounds):
    ctx, a = sharing, rounds["a"]
    reqs = [a.req(i) for i in range(32)]
    reqs[4] = corrupt(reqs[4], "bit")                                         # the record
    reqs[11] = corrupt(reqs[11], "score")                                     # the score
    z = bytearray(reqs[29][2])
    z[0] ^= 0x01
    reqs[29] = reqs[29][:2] + (bytes(z),) + reqs[29][3:]                       # z_img (still canonical)
    off, on, delta = _off_then_on(ctx, reqs)
    want = [VERIFY if i in (4, 11, 29) else OK for i in range(32)]
    assert off == want and on == want
    assert on == ctx.verify_batch(32, 8, _expanded(reqs)[1])
    assert _shared(delta), delta
    assert delta[1] <= 32 and delta[2] == delta[0]  # every rounds call held the one round, once


def test_two_rounds_of_equal_n_differ_in_one_byte_or_in_the_seed(sharing, rounds, oc):
    ctx, a, b, c = sharing, rounds["a"], rounds["b"], rounds["c"]
    assert a.seed == b.seed and a.pub != b.pub and sum(x != y for x, y in zip(a.pub, b.pub)) == 1
    assert a.pub == c.pub and a.seed != c.seed
    reqs, want = [], []
    for i in range(10):
        for r in (a, b, c):
            reqs.append(r.req(i))
            want.append(OK)
    crossed = {7: rc.with_round(a.req(1), b.req(0)),   # a's proof against b's list: one byte of a list item differs
               20: rc.with_round(b.req(2), a.req(0)),
               13: rc.with_round(a.req(0), c.req(0))}  # a's proof against c's seed
    for i, r in crossed.items():
        reqs[i], want[i] = r, VERIFY
        assert oc.verify(*r) == VERIFY
    off, on, delta = _off_then_on(ctx, reqs)
    assert off == want and on == want  # every proof against its own round; the neighbours of a crossed request untouched
    assert _shared(delta), delta


def test_rounds_of_three_list_lengths_and_a_singleton(sharing, rounds):
    ctx = sharing
    order = ["big", "one", "a", "one", "lone", "a", "big", "one", "a", "big", "a", "one"]
    reqs = [rounds[name].req(i) for i, name in enumerate(order)]
    reqs[5] = corrupt(reqs[5], "bit")
    reqs[9] = corrupt(reqs[9], "score")
    off, on, delta = _off_then_on(ctx, reqs)
    Ns, blob = _expanded(reqs)
    assert sorted(set(Ns)) == [1, 8, 202]
    mixed = ctx.verify_batch_mixed(Ns, blob)
    assert on == mixed == off
    assert on == [VERIFY if i in (5, 9) else OK for i in range(len(reqs))]
    assert _shared(delta), delta


def test_a_round_with_a_non_canonical_seed(sharing, rounds):
    ctx, a, c = sharing, rounds["a"], rounds["c"]
    bad_seed = (int.from_bytes(a.seed, "little") + L).to_bytes(32, "little")
    reqs, want = [], []
    for i in range(12):
        if i % 3 == 1:
            reqs.append(a.req(i)[:3] + (bad_seed, a.pub))
            want.append(FORMAT)
        else:
            reqs.append((a if i % 3 == 0 else c).req(i))
            want.append(OK)
    off, on, delta = _off_then_on(ctx, reqs)
    assert off == want and on == want
    assert _shared(delta), delta


def test_a_list_item_stored_as_x_plus_l(sharing, rounds):
    ctx, a = sharing, rounds["a"]
    x = int.from_bytes(a.pub[:32], "little")
    assert x < L
    pub_l = (x + L).to_bytes(32, "little") + a.pub[32:]
    reqs = [a.req(0)[:4] + (pub_l,) if i % 4 == 2 else a.req(i) for i in range(12)]
    off, on, delta = _off_then_on(ctx, reqs)
    assert on == off == ctx.verify_batch(12, 8, _expanded(reqs)[1])
    assert [s for i, s in enumerate(on) if i % 4 != 2] == [OK] * 9
    assert _shared(delta), delta


def test_a_two_phase_record_keeps_the_batch_on_the_old_path(sharing, rounds):
    ctx, a = sharing, rounds["a"]
    reqs = [a.req(i) for i in range(16)]
    # first and last of the queue: should a straggler miss the window, both batches still hold a two-phase record
    reqs[0] = two_phase(reqs[0])
    reqs[15] = corrupt(two_phase(reqs[15]), "bit")
    off, on, delta = _off_then_on(ctx, reqs)
    want = [VERIFY if i == 15 else OK for i in range(16)]
    assert off == want and on == want
    assert delta == (0, 0, 0), delta  # a batch that holds a two-phase record makes no rounds call


def test_all_distinct_rounds_and_a_single_blocking_call_do_not_share(sharing, rounds):
    ctx = sharing
    reqs = [rounds[name].req(0) for name in ("a", "b", "c", "one", "big", "lone")]
    off, on, delta = _off_then_on(ctx, reqs)
    assert off == on == [OK] * 6
    assert delta == (0, 0, 0), delta
    before = ctx.verify_round_sharing_stats()
    assert ctx.verify(*rounds["a"].req(1)) == OK
    assert ctx.verify(*corrupt(rounds["a"].req(1), "bit")) == VERIFY
    assert ctx.verify_round_sharing_stats() == before


def test_eight_blocking_callers_of_one_round(sharing, rounds):
    ctx, big = sharing, rounds["big"]
    reqs = [big.req(j) if j % 3 else corrupt(big.req(j), "score") for j in range(8)]
    out, errors = [None] * 8, []
    gate = threading.Barrier(8)

    def worker(j):
        try:
            gate.wait(30)
            out[j] = ctx.verify(*reqs[j])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    before = ctx.verify_round_sharing_stats()
    th = [threading.Thread(target=worker, args=(j,)) for j in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    delta = tuple(x - y for x, y in zip(ctx.verify_round_sharing_stats(), before))
    print(out, delta)
    assert not errors, errors
    assert out == [OK if j % 3 else VERIFY for j in range(8)]
    assert _shared(delta), delta


def test_one_round_through_a_pool(bbp, ctx, rounds):
    pool = bbp.Pool([0, 0])  # two member contexts on the one card (tests/test_gpu_multi.py)
    try:
        pool.set_batching(WINDOW_US, 4096)
        a = rounds["a"]
        reqs = [corrupt(a.req(i), "bit") if i % 9 == 4 else a.req(i) for i in range(64)]
        want = [VERIFY if i % 9 == 4 else OK for i in range(64)]
        assert burst(pool, reqs) == want
        assert pool.verify_round_sharing_stats() == (0, 0, 0)  # off by default
        pool.set_verify_round_sharing(True)
        assert "verify round sharing: on" in pool.describe()
        assert burst(pool, reqs) == want
        calls, rows, tables = pool.verify_round_sharing_stats()
        members = [pool.member(i).verify_round_sharing_stats() for i in range(2)]
        print("pool rounds calls / rows / rounds", (calls, rows, tables), "members", members)
        assert calls >= 1 and tables < rows <= 64
        assert tuple(sum(m[k] for m in members) for k in range(3)) == (calls, rows, tables)
        assert pool.health() == 0
    finally:
        pool.close()


def _child(job, env_extra, limit=420):
    d = tempfile.mkdtemp(prefix="bbp-round-sharing-")
    pin, pout = os.path.join(d, "in.json"), os.path.join(d, "out.json")
    json.dump(job, open(pin, "w"))
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "verify_round_sharing_cases.py"), pin, pout], env=env, capture_output=True,
                       text=True, timeout=limit, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.load(open(pout))


def _three_round_burst(rounds, count=48):
    reqs, want = [], []
    for i in range(count):
        r = rounds[("a", "one", "c")[i % 3]].req(i // 3)
        kind = (None, None, None, "bit", None, None, "score")[i % 7]
        reqs.append(corrupt(r, kind) if kind else r)
        want.append(VERIFY if kind else OK)
    return reqs, want


def test_aggregated_engine_gives_the_same_statuses(sharing, rounds):
    """BBP_VERIFY_AGGREGATE=8 in a child process with sharing on: the rounds call is checked in groups and reports what the plain path
    reports here."""
    ctx = sharing
    reqs, want = _three_round_burst(rounds)
    plain = burst(ctx, reqs)
    assert plain == want
    res = _child({"bursts": [to_json(reqs), to_json(reqs)]}, {"BBP_VERIFY_AGGREGATE": "8"})
    print(res["describe"], [b["shared"] for b in res["bursts"]])
    assert "aggregate groups of 8" in res["describe"] and "aggregate groups of 8 (off)" not in res["describe"]
    assert "verify round sharing: on" in res["describe"]
    assert res["bursts"][0]["status"] == res["bursts"][1]["status"] == plain
    assert all(_shared(b["shared"]) for b in res["bursts"]) and res["health"] == 0


def test_device_entropy_gives_the_same_statuses(sharing, rounds):
    ctx = sharing
    reqs, want = _three_round_burst(rounds)
    st_os = burst(ctx, reqs)
    ctx.set_entropy_source("device")
    before = ctx.verify_round_sharing_stats()
    st_dev = burst(ctx, reqs)
    delta = tuple(x - y for x, y in zip(ctx.verify_round_sharing_stats(), before))
    assert st_dev == st_os == want
    assert _shared(delta), delta
