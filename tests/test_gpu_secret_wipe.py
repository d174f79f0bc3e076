"""GPU tier: secret wiping (include/bbp.h "Secret wiping": bbp_set_secret_wipe, bbp_wipe_secrets and the two test hooks).  With
wiping on, every secret-class buffer of the context (csrc/secret_map.h) reads zero whenever no prove-side call is in flight -- the
residue hook counts non-zero bytes over the buffers' whole capacity, the scan hook looks for a bid's own d, k, y^-1, first blinding and
rng seed in every buffer of the table and in the resident tables, secret or public -- and every record, status and toggle is byte for byte what it is with
wiping off.  The first test shows that the hooks see what an unwiped call leaves behind; every other test leans on it."""
import os
import random
import re
import signal
import subprocess
import tempfile
import threading
import time

import pytest

from tests import prove_round_cases as rc
from tests import uds_client as uc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes((0x3C ^ (17 * i)) & 0xFF for i in range(32))
BAD_ARG = 4
TAG_WIPE = 13  # csrc/context.h: the tag of k_wipe_spans in bbp_last_timings


@pytest.fixture(scope="module")
def wctx(ctx, bbp):
    """A context of this module's own (the switch is flipped here; after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    c.set_secret_wipe(False)
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def batches(ctx):
    """Synthesised once: (B, N) -> (input rows, entropy rows, verify tails)."""
    made = {}

    def get(B, N, seed=0):
        if (B, N, seed) not in made:
            made[(B, N, seed)] = _synth_batch(ctx, B, N, seed=9100 + 7 * N + B + seed)
        return made[(B, N, seed)]
    return get


def _patterns(ins, ents, i=0):
    """What a bid must not leave behind: d, k and y^-1 of input row i, its first commitment blinding and its TranscriptRng seed"""
    row, ent = ins[i], ents[i]
    return {"d": row[0:32], "k": row[32:64], "y_inv": row[96:128], "blinding": ent[0:32], "rng seed": ent[-32:]}


def _assert_clean(c, pats):
    dev, host, where = c.debug_secret_residue()
    assert (dev, host) == (0, 0), "residue: %d device bytes, %d host bytes, first in %r" % (dev, host, where)
    for name, p in pats.items():
        assert c.debug_secret_scan(p) == (0, 0), name


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


# ---- 1. the hooks can see ------------------------------------------------------------------------------------------------------------
def test_hooks_see_what_an_unwiped_call_leaves(wctx, batches):
    B, N = 3, 8
    ins, ents, _ = batches(B, N)
    wctx.set_secret_wipe(False)
    wctx.wipe_secrets()
    out, st = wctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    assert st == [0] * B
    dev, host, where = wctx.debug_secret_residue()
    assert dev > 0 and host > 0 and where != "", (dev, host, where)
    pats = _patterns(ins, ents)
    for name in ("d", "k", "blinding"):
        hits = wctx.debug_secret_scan(pats[name])
        assert hits[0] >= 1 and sum(hits) >= 1, (name, hits)
    wctx.wipe_secrets()
    _assert_clean(wctx, pats)
    # the scan's argument screening
    for bad in (b"", b"abc", b"x" * 6, b"y" * 68):
        with pytest.raises(Exception):
            wctx.debug_secret_scan(bad)
    assert wctx.debug_secret_scan(b"\x5a\xa5\x5a\xa5") == (0, 0)


# ---- 2. invariant and byte equality per path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,env", [
    (1, 1, {}),                                # wave-mode transcript, split MSMs
    (3, 202, {}),                              # largest m, no padded range
    (130, 8, {}),                              # 128 or more MSMs per launch: the unsplit sort and accumulate; rotating
    (12, 8, {"BBP_ROTATE_BELOW": "0"}),        # three slices of four proofs, the sliced joins
    (12, 8, {"BBP_OPEN_ON_CHAIN": "1"}),       # opening stage on the call's chain stream
    (7, 8, {"BBP_HOST_CHUNK_PROVE": "3"}),     # a host call cut into chunks wipes per chunk
])
def test_invariant_and_byte_equality_per_path(wctx, bbp, batches, monkeypatch, B, N, env):
    ins, ents, _ = batches(B, N)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = bbp.Context(0) if env else wctx  # the knobs are read by bbp_init
    try:
        c.set_secret_wipe(False)
        off = c.prove_batch(B, N, b"".join(ins), b"".join(ents))
        assert off[1] == [0] * B
        c.set_secret_wipe(True)
        for _ in range(2):  # the second call finds the first call's wiped buffers
            on = c.prove_batch(B, N, b"".join(ins), b"".join(ents))
            assert on == off
            for i in sorted({0, B - 1}):
                _assert_clean(c, _patterns(ins, ents, i))
    finally:
        if env:
            flags = c.health()
            c.close()
            assert flags == 0
        else:
            c.set_secret_wipe(False)


# ---- 3. the wipe races nothing -----------------------------------------------------------------------------------------------------
def test_device_calls_back_to_back_and_host_threads(wctx, bbp, batches):
    import torch
    N = 8
    sizes = [5, 70, 5, 70, 5, 70, 5]  # seven: more than PROVE_BUFS, so a buffer comes round again with its wipe between two users
    sets = [batches(Bk, N, seed=100 + j) for j, Bk in enumerate(sizes)]
    d_in = [_dev(b"".join(s[0])) for s in sets]
    d_ent = [_dev(b"".join(s[1])) for s in sets]
    rec = bbp.record_size(N)

    def sequence():
        outs = [torch.zeros(Bk * rec, dtype=torch.uint8, device="cuda") for Bk in sizes]
        torch.cuda.synchronize()
        for j, Bk in enumerate(sizes):  # no host synchronisation between the calls, all on the context's stream
            wctx.prove_batch_dev(Bk, N, d_in[j].data_ptr(), d_ent[j].data_ptr(), outs[j].data_ptr())
        assert wctx.health() == 0  # synchronises the device
        return [_host(o) for o in outs]
    wctx.set_secret_wipe(False)
    off = sequence()
    wctx.set_secret_wipe(True)
    try:
        on = sequence()
        assert on == off
        for j in (0, 1, 6):
            _assert_clean(wctx, _patterns(sets[j][0], sets[j][1]))
        # the caller's own device buffers stay the caller's
        assert _host(d_in[1]) == b"".join(sets[1][0]) and _host(d_ent[1]) == b"".join(sets[1][1])
        # four host threads in prove_batch: staging slots in rotation, calls overlapping on the device
        wctx.set_secret_wipe(False)
        want = [wctx.prove_batch(sizes[j], N, b"".join(sets[j][0]), b"".join(sets[j][1])) for j in range(4)]
        wctx.set_secret_wipe(True)
        got = [None] * 4

        def work(j):
            got[j] = wctx.prove_batch(sizes[j], N, b"".join(sets[j][0]), b"".join(sets[j][1]))
        th = [threading.Thread(target=work, args=(j,)) for j in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == want
        for j in range(4):
            _assert_clean(wctx, _patterns(sets[j][0], sets[j][1]))
        # ... and four single-proof callers through the combiner
        single = [None] * 4

        def one(j):
            row = sets[j][0][0]
            single[j] = wctx.prove(row[:224], row[224:224 + 32 * N], int.from_bytes(row[-8:], "little"), sets[j][1][0])
        th = [threading.Thread(target=one, args=(j,)) for j in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert single == [want[j][0][:rec] for j in range(4)]
        for j in range(4):
            _assert_clean(wctx, _patterns(sets[j][0], sets[j][1]))
    finally:
        wctx.set_secret_wipe(False)


# ---- 4. checked proving and hedging keep their contracts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "round"])
@pytest.mark.parametrize("source", ["explicit", "hedged"])
def test_checked_proving_and_hedging_keep_their_contracts(bbp, batches, form, source):
    B, N = 3, 8
    if form == "rows":
        ins, ents, _ = batches(B, N)
        ent = b"".join(ents)
    else:
        r = rc.honest(N, B, tag=41)
        ins = [r.in_row(i) for i in range(B)]
        ent = rc.entropy(41, B, N)
        ents = [ent[i * bbp.entropy_size(N):(i + 1) * bbp.entropy_size(N)] for i in range(B)]
    c = bbp.Context(0)
    try:
        c.set_prove_check(True)
        if source == "hedged":
            c.set_entropy_source("hedged")

        def call():
            if source == "hedged":
                c.debug_next_entropy_key(KEY)
            c.debug_corrupt_next_proof(1)
            n0 = c.prove_check_stats()
            e = None if source == "hedged" else ent
            res = c.prove_batch(B, N, b"".join(ins), e) if form == "rows" else c.prove_round(N, r.table, r.bid_bytes, e)
            n1 = c.prove_check_stats()
            return res, tuple(b - a for a, b in zip(n0, n1))
        off = call()
        assert off[1][0] == B and off[1][2] == 1, off[1]  # one record failed its check and was proved again
        c.set_secret_wipe(True)
        on = call()
        assert on == off
        pats = _patterns(ins, ents, 1)  # the corrupted row: proved twice
        if source == "hedged":
            pats = {k: v for k, v in pats.items() if k not in ("blinding", "rng seed")}  # drawn on the device: not these bytes
        pats["call key"] = KEY
        _assert_clean(c, pats)
    finally:
        flags = c.health()
        c.close()
        assert flags == 0


# ---- 5. round calls, witness, MSM hook -----------------------------------------------------------------------------------------------
def _round_with_a_stranger(N, B, tag):
    r = rc.honest(N, B, tag)
    rnd = random.Random(tag)
    bids, expect = list(r.bids), list(r.expect)
    bids[3] = (rnd.getrandbits(64), rnd.randrange(rc.L))  # its x is in no list
    expect[3] = (BAD_ARG, 0, None)
    return rc.Round(N, r.seed, r.items, bids, expect)


def test_round_calls_witness_and_msm_hook(wctx, bbp):
    import torch
    N, B = 8, 5
    r = _round_with_a_stranger(N, B, tag=77)
    ent = rc.entropy(77, B, N)
    es = bbp.entropy_size(N)
    pats = {"bid 0": rc.b32(r.bids[0][0]) + rc.b32(r.bids[0][1]), "bid 3 (refused)": rc.b32(r.bids[3][0]) + rc.b32(r.bids[3][1]),
            "blinding": ent[:32], "rng seed": ent[es - 32:es]}
    dks = b"".join(rc.b32(d) + rc.b32(k) + r.seed for d, k in r.bids[:3])
    rnd = random.Random(5)
    scal = b"".join(rc.b32(rnd.randrange(rc.L)) for _ in range(3 * 5))

    def device_round():
        d_tab, d_bids, d_ent = _dev(r.table), _dev(r.bid_bytes), _dev(ent)
        rows = torch.zeros(B * bbp.round_row_size(N), dtype=torch.uint8, device="cuda")
        st = torch.zeros(B, dtype=torch.int32, device="cuda")
        tog = torch.zeros(B, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        wctx.prove_round_dev(N, d_tab.data_ptr(), B, d_bids.data_ptr(), d_ent.data_ptr(), rows.data_ptr(), st.data_ptr(), tog.data_ptr())
        assert wctx.health() == 0  # synchronises
        return _host(rows), st.cpu().tolist(), tog.cpu().tolist()

    def everything():
        return (wctx.prove_round(N, r.table, r.bid_bytes, ent), device_round(), wctx.witness_batch(dks), wctx.msm_batch(3, 5, scal, 1))
    wctx.set_secret_wipe(False)
    off = everything()
    assert off[0][2] == r.status and off[0][1] == r.toggles and off[1][1] == r.status
    wctx.set_secret_wipe(True)
    try:
        host_round = wctx.prove_round(N, r.table, r.bid_bytes, ent)
        _assert_clean(wctx, pats)
        dev_round = device_round()
        _assert_clean(wctx, pats)
        wit = wctx.witness_batch(dks)
        _assert_clean(wctx, {"dks": dks[:64], "y_inv": wit[96:128]})
        msm = wctx.msm_batch(3, 5, scal, 1)
        _assert_clean(wctx, {"scalars": scal[:64]})
        assert (host_round, dev_round, wit, msm) == off
    finally:
        wctx.set_secret_wipe(False)


# ---- 6. growth -------------------------------------------------------------------------------------------------------------------------
def _allocations(c):
    return int(re.search(r"in (\d+) allocation", c.describe()).group(1))


def test_growth_erases_before_it_frees(bbp, batches):
    N = 8
    small, large = batches(4, N), batches(40, N)
    results = {}
    for on in (False, True):
        c = bbp.Context(0)
        try:
            c.set_secret_wipe(on)
            a = c.prove_batch(4, N, b"".join(small[0]), b"".join(small[1]))
            n0 = _allocations(c)
            b = c.prove_batch(40, N, b"".join(large[0]), b"".join(large[1]))
            assert _allocations(c) > n0  # the second call grew buffers the first had made (free + malloc)
            results[on] = (a, b)
            if on:
                _assert_clean(c, _patterns(small[0], small[1]))
                _assert_clean(c, _patterns(large[0], large[1], 39))
        finally:
            flags = c.health()
            c.close()
            assert flags == 0
    assert results[True] == results[False]


# ---- 7. surface ------------------------------------------------------------------------------------------------------------------------
def _tags(c, call):
    c.set_profiling(True)
    c.last_timings()
    res = call()
    tags = [int(t) for t, _ in c.last_timings()]
    c.set_profiling(False)
    return res, tags


def test_describe_challenges_verify_and_launch_tables(wctx, bbp, batches):
    B, N = 3, 8
    ins, ents, vins = batches(B, N)
    wctx.set_secret_wipe(False)
    assert "secret wipe: off" in wctx.describe()
    out, st = wctx.prove_batch(B, N, b"".join(ins), b"".join(ents))
    ch = wctx.debug_challenges(B, N, 0)
    rs_ = bbp.record_size(N)
    vin = b"".join(out[i * rs_:(i + 1) * rs_] + b"".join(vins[i][:3]) + vins[i][3] for i in range(B))
    bad = bytearray(vin)
    bad[rs_ + 96 + 32 * N + 200] ^= 0x10
    v_off, t_off = _tags(wctx, lambda: (wctx.verify_batch(B, N, vin), wctx.verify_batch(B, N, bytes(bad))))
    assert v_off == ([0] * B, [0, 1, 0])
    assert TAG_WIPE not in t_off
    # one prove call with wiping off: the launch table is the parent commit's (profiles/r17_prove_launches_plain_parent.csv, written by
    # the parent's own tools/prove_launches.py: all-zero rows, B = 64, N = 8) -- no added launch.  k_wipe_spans carries a tag of its own,
    # so a wipe that ran while off, or in a verify call, would show here.
    zr, ze = bytes((7 * 32 + 32 * N + 8) * 64), bytes(bbp.entropy_size(N) * 64)
    wctx.prove_batch(64, N, zr, ze)
    _, p_off = _tags(wctx, lambda: wctx.prove_batch(64, N, zr, ze))
    table = open(os.path.join(ROOT, "profiles", "r17_prove_launches_plain_parent.csv")).read()
    assert "order," + " ".join(str(t) for t in p_off) + "\n" in table
    assert TAG_WIPE not in p_off
    wctx.set_secret_wipe(True)
    try:
        assert "secret wipe: on" in wctx.describe()
        assert wctx.prove_batch(B, N, b"".join(ins), b"".join(ents)) == (out, st)
        with pytest.raises(bbp.BbpError) as e:
            wctx.debug_challenges(B, N, 0)
        assert e.value.status == BAD_ARG and "secret wiping is on" in str(e.value)
        v_on, t_on = _tags(wctx, lambda: (wctx.verify_batch(B, N, vin), wctx.verify_batch(B, N, bytes(bad))))
        assert v_on == v_off and t_on == t_off and TAG_WIPE not in t_on  # verify calls are untouched: no wipe launch
        wctx.wipe_secrets()  # (empties the wipe log)
        _, p_on = _tags(wctx, lambda: wctx.prove_batch(64, N, zr, ze))
        # the parent's table plus exactly one wipe per stream the call used: opening stream (draws), heavy-stage stream (MSM scratch
        # slot), the caller's stream (batch buffer), the copy stream (staging slot)
        assert [t for t in p_on if t != TAG_WIPE] == p_off
        assert p_on.count(TAG_WIPE) == 4, p_on
        rng_end = max(i for i, t in enumerate(p_on) if t == 4)
        assert p_on[rng_end + 1] == TAG_WIPE and p_on[-3:] == [TAG_WIPE, TAG_WIPE, TAG_WIPE], p_on  # draws' wipe before the heavy stage; the rest behind it
        nbytes, launches, lone_us = wctx.debug_wipe_cost(clear=True)
        assert launches == 4 and nbytes > 64 * 1000000 and lone_us > 0  # ~1.3 MB per proof
    finally:
        wctx.set_secret_wipe(False)
    assert wctx.prove_batch(B, N, b"".join(ins), b"".join(ents)) == (out, st)
    assert wctx.debug_challenges(B, N, 0) == ch  # working again after off and a new call


def test_pool_sets_every_member_and_refuses_the_hooks(bbp, batches):
    B, N = 6, 8
    ins, ents, _ = batches(B, N)
    p = bbp.Pool([0, 0])  # two member contexts on the one card of a GPU box
    try:
        off = p.prove_batch(B, N, b"".join(ins), b"".join(ents))
        p.set_secret_wipe(True)
        assert p.prove_batch(B, N, b"".join(ins), b"".join(ents)) == off
        row = ins[0]
        assert p.prove(row[:224], row[224:224 + 32 * N], int.from_bytes(row[-8:], "little"), ents[0]) == off[0][:bbp.record_size(N)]
        for i in range(2):
            m = p.member(i)
            assert "secret wipe: on" in m.describe()
            _assert_clean(m, _patterns(ins, ents, 0))
            _assert_clean(m, _patterns(ins, ents, B - 1))
        with pytest.raises(bbp.BbpError):
            p.debug_secret_residue()
        with pytest.raises(bbp.BbpError):
            p.debug_secret_scan(b"abcd")
        p.wipe_secrets()
    finally:
        p.close()


def test_server_with_wipe_secrets(ctx, built, bbp, batches):
    built.build_server()
    N, K = 8, 3
    ins, _, vins = batches(K, N)
    d = tempfile.mkdtemp(prefix="bbp-uds-wipe-")
    path = os.path.join(d, "sock")
    log = open(os.path.join(d, "log"), "w+")
    p = subprocess.Popen([built.SERVER_BIN, "-b", path, "-l", "info", "--engine", bbp.lib_path, "--device", "0", "--window-us", "200",
                          "--wipe-secrets"], stderr=log)
    try:
        for _ in range(1500):
            if os.path.exists(path) or p.poll() is not None:
                break
            time.sleep(0.02)
        assert os.path.exists(path), open(log.name).read()[-800:]
        blobs = [uc.prove(path, ins[j][:224], ins[j][224:224 + 32 * N], int.from_bytes(ins[j][-8:], "little")) for j in range(K)]
        for j in range(K):
            assert uc.verify(path, blobs[j], *vins[j]) == b"\x01"
        assert "secret wiping on" in open(log.name).read()
    finally:
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
            p.wait(timeout=30)
