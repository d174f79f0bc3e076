"""GPU tier: concurrent single-proof verify callers share device calls across bid-list lengths and record layouts
(include/bbp.h bbp_verify / bbp_verify_async / bbp_set_verify_mixing; csrc/submit.cpp, csrc/verifier_mixed.inc).

Every status a request receives from a combined call must be what the proof gets on its own: bbp_verify_batch with the row's N
for a compact record, a lone bbp_verify for a two-phase one, and the C oracle's verdict for every compact record (the oracle
parses that layout only).  The
call counts (bbp_batching_stats) show that the requests did share calls: a burst of eight list lengths inside one batching
window is at most two device calls (one straggler may miss the window) where grouping by list length needs at least eight.

Every child process a test starts runs under a time limit of its own, and nothing is retried."""
import json
import os
import re
import signal
import subprocess
import sys
import tempfile
import threading
import time

import pytest

from tests import oracle_c, uds_client as uc
from tests import verify_combine_cases as vc
from tests.test_gpu_verify_mixed import _synth

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT = 0, 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_US = 100000
PER_N = 12


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def valid(ctx, oc, bbp):
    """PER_N valid requests for every list length of the burst, proved by the engine under fixed entropy."""
    out = {}
    for n in vc.NS_BURST:
        ins, ents, tails = _synth(oc, PER_N, n, seed=7000 + n)
        rec, st = ctx.prove_batch(PER_N, n, b"".join(ins), b"".join(ents))
        assert st == [0] * PER_N
        rs_ = bbp.record_size(n)
        out[n] = [(rec[i * rs_:(i + 1) * rs_], tails[i][:32], tails[i][32:64], tails[i][64:96], tails[i][96:]) for i in range(PER_N)]
    return out


@pytest.fixture()
def windowed(ctx):
    """The shared context with a 100 ms batching window; afterwards as it was (no window, mixing on, OS entropy)."""
    ctx.set_batching(WINDOW_US, 4096)
    ctx.set_verify_mixing(True)
    yield ctx
    ctx.set_batching(0, 0)
    ctx.set_verify_mixing(True)
    ctx.set_entropy_source("os")


def _alone(ctx, reqs):
    """What every request gets on its own, with no batching window: bbp_verify_batch of one row for a compact-length record (the
    row's N), a lone bbp_verify for a two-phase one."""
    ctx.set_batching(0, 0)
    out = []
    for r in reqs:
        n = vc.n_of(r)
        if len(r[0]) == 1121 + 32 * (4 + n):
            out.append(ctx.verify_batch(1, n, b"".join(r))[0])
        else:
            out.append(ctx.verify(*r))
    ctx.set_batching(WINDOW_US, 4096)
    return out


def _many_n_burst(valid, count=96):
    """`count` requests over the eight list lengths: valid, a flipped bit, a wrong score, a first byte that is neither 0 nor 1."""
    reqs, kinds = [], []
    for i in range(count):
        n = vc.NS_BURST[i % len(vc.NS_BURST)]
        r = valid[n][(i // len(vc.NS_BURST)) % PER_N]
        kind = (None, None, "bit", None, "score", None, None, "version", None, None, None)[i % 11]
        reqs.append(vc.corrupt(r, kind) if kind else r)
        kinds.append(kind)
    return reqs, kinds


def _calls(handle):
    return handle.batching_stats()[0]


def test_one_burst_of_many_list_lengths_is_one_call(windowed, valid, oc):
    ctx = windowed
    reqs, kinds = _many_n_burst(valid)
    assert len({vc.n_of(r) for r in reqs}) == 8 and {None, "bit", "score", "version"} == set(kinds)
    alone = _alone(ctx, reqs)
    vc.burst(ctx, reqs)  # warm: every circuit compiled and the buffers at size before the burst that is counted
    before = _calls(ctx)
    st = vc.burst(ctx, reqs)
    calls = _calls(ctx) - before
    print("statuses", st, "calls", calls)
    assert st == alone
    assert [s for s, k in zip(st, kinds) if k is None] == [OK] * kinds.count(None)
    assert all(s == FORMAT for s, k in zip(st, kinds) if k == "version")
    assert all(s == VERIFY for s, k in zip(st, kinds) if k in ("bit", "score"))
    for r, s, k in zip(reqs, st, kinds):
        assert oc.verify(*r) == s, (vc.n_of(r), k)
    assert calls <= 2, calls


def test_both_layouts_in_one_burst(windowed, valid):
    ctx = windowed
    reqs = []
    for j, n in enumerate((2, 8, 40)):
        a, b, c, d = valid[n][:4]
        reqs += [a, vc.two_phase(b), vc.corrupt(c, "bit"), vc.corrupt(vc.two_phase(d), "bit"), vc.corrupt(vc.two_phase(a), "score")]
    compact_as_1 = (b"\x01" + valid[8][5][0][1:],) + valid[8][5][1:]
    two_as_0 = vc.two_phase(valid[8][6])
    two_as_0 = (b"\x00" + two_as_0[0][1:],) + two_as_0[1:]
    reqs += [compact_as_1, two_as_0]
    alone = _alone(ctx, reqs[:-2]) + [ctx.verify(*compact_as_1), ctx.verify(*two_as_0)]
    assert alone[-2:] == [FORMAT, FORMAT]
    assert alone[:5] == [OK, OK, VERIFY, VERIFY, VERIFY]
    vc.burst(ctx, reqs)
    before = _calls(ctx)
    st = vc.burst(ctx, reqs)
    print("statuses", st, "calls", _calls(ctx) - before)
    assert st == alone
    assert _calls(ctx) - before <= 2


@pytest.mark.parametrize("where", ["first", "last", "between"])
def test_a_bad_row_changes_no_neighbour(windowed, valid, where):
    ctx = windowed
    good = [valid[1][0], vc.two_phase(valid[202][0]), valid[13][0], valid[202][1], valid[1][1], vc.two_phase(valid[5][0])]
    bad = vc.corrupt(valid[40][0], "bit")
    reqs = {"first": [bad] + good, "last": good + [bad], "between": good[:1] + [valid[1][2], bad, valid[202][2]] + good[1:]}[where]
    st = vc.burst(ctx, reqs)
    assert st == [VERIFY if r is bad else OK for r in reqs]


def test_single_list_length_same_with_mixing_on_and_off(windowed, valid):
    ctx = windowed
    reqs = [vc.corrupt(r, "bit") if i % 5 == 2 else r for i, r in enumerate(valid[8] * 3)]
    want = [VERIFY if i % 5 == 2 else OK for i in range(len(reqs))]
    res = {}
    for on in (True, False):
        ctx.set_verify_mixing(on)
        before = _calls(ctx)
        res[on] = (vc.burst(ctx, reqs), _calls(ctx) - before)
        assert ("verify mixing: on" if on else "verify mixing: off") in ctx.describe()
    print(res)
    assert res[True][0] == res[False][0] == want
    assert res[True][1] <= 2 and res[False][1] <= 2


def test_mixing_off_restores_one_call_per_list_length(windowed, valid):
    ctx = windowed
    reqs, kinds = _many_n_burst(valid, 48)
    vc.burst(ctx, reqs)
    on_before = _calls(ctx)
    st_on = vc.burst(ctx, reqs)
    on_calls = _calls(ctx) - on_before
    ctx.set_verify_mixing(False)
    before = _calls(ctx)
    st_off = vc.burst(ctx, reqs)
    off_calls = _calls(ctx) - before
    print("calls on", on_calls, "off", off_calls)
    assert st_on == st_off
    assert off_calls >= 8 and on_calls <= 2


def test_eight_blocking_callers_of_different_list_lengths(windowed, valid):
    ctx = windowed
    reqs = [valid[n][3] if j % 3 else vc.corrupt(valid[n][3], "score") for j, n in enumerate(vc.NS_BURST)]
    out, errors = [None] * 8, []
    gate = threading.Barrier(8)

    def worker(j):
        try:
            gate.wait(30)
            out[j] = ctx.verify(*reqs[j])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    before = _calls(ctx)
    th = [threading.Thread(target=worker, args=(j,)) for j in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errors, errors
    assert out == [OK if j % 3 else VERIFY for j in range(8)]
    assert _calls(ctx) - before < 8


def test_mixed_burst_through_a_pool(bbp, ctx, valid):
    pool = bbp.Pool([0, 0])  # two member contexts on the one card (tests/test_gpu_multi.py)
    try:
        pool.set_batching(WINDOW_US, 4096)
        reqs, kinds = _many_n_burst(valid, 192)
        want = [OK if k is None else FORMAT if k == "version" else VERIFY for k in kinds]
        assert vc.burst(pool, reqs) == want
        before = pool.batching_stats()
        members_before = [pool.member_stats(i) for i in range(2)]
        assert vc.burst(pool, reqs) == want
        calls, nreq, _ = pool.batching_stats()
        members = [pool.member_stats(i) for i in range(2)]
        queued = sum(1 for k in kinds if k != "version")  # a foreign first byte is refused on the host: never queued
        print("pool calls", calls - before[0], "requests", nreq - before[1], members_before, members)
        assert nreq - before[1] == queued
        assert sum(m[1] - b[1] for m, b in zip(members, members_before)) == queued
        assert sum(m[0] - b[0] for m, b in zip(members, members_before)) == calls - before[0] <= 4
        pool.set_verify_mixing(False)
        assert vc.burst(pool, reqs) == want
        assert pool.batching_stats()[0] - calls >= 8
        assert pool.health() == 0
    finally:
        pool.close()


def _child(job, env_extra, limit=420):
    d = tempfile.mkdtemp(prefix="bbp-combine-")
    pin, pout = os.path.join(d, "in.json"), os.path.join(d, "out.json")
    json.dump(job, open(pin, "w"))
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "verify_combine_cases.py"), pin, pout], env=env, capture_output=True, text=True,
                       timeout=limit, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.load(open(pout))


def test_aggregated_engine_gives_the_same_statuses(windowed, valid):
    """BBP_VERIFY_AGGREGATE=8 in a child process: a compact-only mixed burst is checked in groups and reports what the plain path
    reports; a burst that holds one two-phase row runs plain and still answers every row correctly."""
    ctx = windowed
    compact, kinds = _many_n_burst(valid, 64)
    with_two = list(compact)
    with_two[17] = vc.two_phase(valid[40][7])
    with_two[30] = vc.corrupt(vc.two_phase(valid[3][7]), "bit")
    plain = [vc.burst(ctx, compact), vc.burst(ctx, with_two)]
    res = _child({"bursts": [vc.to_json(compact), vc.to_json(compact), vc.to_json(with_two)]}, {"BBP_VERIFY_AGGREGATE": "8"})
    print(res["describe"], [b["calls"] for b in res["bursts"]])
    assert "aggregate groups of 8" in res["describe"] and "aggregate groups of 8 (off)" not in res["describe"]
    assert res["bursts"][0]["status"] == res["bursts"][1]["status"] == plain[0]
    assert res["bursts"][2]["status"] == plain[1]
    assert plain[1][17] == OK and plain[1][30] == VERIFY
    assert res["bursts"][1]["calls"] <= 2 and res["health"] == 0


def test_device_entropy_gives_the_same_statuses(windowed, valid):
    ctx = windowed
    reqs, kinds = _many_n_burst(valid, 48)
    reqs[5] = vc.two_phase(reqs[5])
    st_os = vc.burst(ctx, reqs)
    ctx.set_entropy_source("device")
    before = _calls(ctx)
    st_dev = vc.burst(ctx, reqs)
    assert st_dev == st_os == [OK if k is None else FORMAT if k == "version" else VERIFY for k in kinds]
    assert _calls(ctx) - before <= 2


def _blob(record, n):
    """The wire form of a proof as opcode 1 answers it: TLV(proof) || LIST(4 commitments) || LIST(t_c)."""
    body = record[1121:]
    pts = [body[32 * i:32 * i + 32] for i in range(4 + n)]
    return uc.tlv(record[:1121]) + uc.tlv_list(pts[:4]) + uc.tlv_list(pts[4:])


def test_sixty_four_connections_of_four_list_lengths_through_the_server(built, bbp, valid):
    built.build_server()
    d = tempfile.mkdtemp(prefix="bbp-uds-combine-")
    path, batch_log = os.path.join(d, "sock"), os.path.join(d, "batches")
    err = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", str(WINDOW_US),
                          "--verify-mixing", "on"], stderr=err, env=dict(os.environ, BBP_BATCH_LOG=batch_log))
    try:
        for _ in range(3000):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), "server did not bind: " + open(err.name).read()[-800:]
        ns = (2, 8, 40, 202)
        jobs = []
        for i in range(64):
            r = valid[ns[i % 4]][(i // 4) % PER_N]
            bad = i % 8 == 3
            if bad:
                r = vc.corrupt(r, "bit" if i % 16 == 3 else "score")
            jobs.append((uc.verify_request(_blob(r[0], vc.n_of(r)), r[1], r[2], r[3], r[4]), b"\x00" if bad else b"\x01"))
        for round_ in range(2):  # the first round compiles the four circuits and sizes the buffers
            answers, errors = [None] * 64, []
            gate = threading.Barrier(64)

            def worker(i):
                try:
                    c = uc.Conn(path, timeout=240.0)
                    try:
                        gate.wait(60)
                        c.send(jobs[i][0])
                        answers[i] = c.recv_frame()
                    finally:
                        c.close()
                except Exception as e:  # noqa: BLE001
                    errors.append(repr(e))
            th = [threading.Thread(target=worker, args=(i,)) for i in range(64)]
            for t in th:
                t.start()
            for t in th:
                t.join(300)
            assert not errors, errors[:3]
            assert answers == [j[1] for j in jobs], round_
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=60)
    err.seek(0)
    log = err.read()
    assert "verify mixing on" in log, log[-1500:]
    rows = [l.split() for l in open(batch_log) if l.strip()]
    verify_rows = [r for r in rows if r[2] == "verify"]
    print(verify_rows)
    assert sum(int(r[4]) for r in verify_rows) == 128
    assert any(int(r[8]) >= 2 for r in verify_rows), verify_rows       # mixed batches: several list lengths in one device call
    assert len(verify_rows) <= 6, verify_rows                          # per list length it would be at least eight
    m = re.search(r"served (\d+) requests", log)
    assert m and int(m.group(1)) == 128, log[-800:]
