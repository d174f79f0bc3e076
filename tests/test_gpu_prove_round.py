"""GPU tier: proving a round from raw bids (include/bbp.h bbp_prove_round, bbp_prove_round_dev, bbp_prepare_round_dev).  One call
takes the round (seed || pub_list, once) and raw bids (d || k); witness, toggle search and proofs happen on the device and the rows
that come back are the rows bbp_verify_rounds takes.  Expected values come from tests/prove_round_cases.py (the big-int oracle; the
same cases the CPU tier runs through the header), the C oracle, bbp_prove_batch on the expanded rows and bbp_witness_batch."""
import ctypes
import re

import pytest

from tests import entropy_ref as er
from tests import oracle_c
from tests import prove_round_cases as rc

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG = 0, 1, 3, 4
KEY = bytes((0xC3 ^ (7 * i)) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def rctx(ctx, bbp):
    """A context of this module's own (settings are switched here; after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def status_case(rctx):
    """The statuses round and the result of ONE call on it, shared by the tests that look at it."""
    r = rc.status_round()
    ent = rc.entropy(5, r.B, r.N)
    return r, ent, rctx.prove_round(r.N, r.table, r.bid_bytes, ent)


def _split(rows, N, bbp):
    rs_, row = bbp.record_size(N), bbp.round_row_size(N)
    return [(rows[row * i:row * i + rs_], rows[row * i + rs_:row * (i + 1)]) for i in range(len(rows) // row)]


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("N,B", [(1, 5), (3, 5), (8, 5), (202, 3)])
def test_parity_with_oracle_prove_batch_and_witness_batch(rctx, oc, bbp, N, B):
    r = rc.honest(N, B, tag=2)
    assert {0, N - 1} <= set(r.toggles)
    ent = rc.entropy(N, B, N)
    rows, toggles, st = rctx.prove_round(N, r.table, r.bid_bytes, ent)
    assert st == [OK] * B and toggles == r.toggles
    ins = r.in_rows()
    cout, cst = oc.prove_many(ins, ent, B, N, threads=4)       # the C oracle on the expanded rows
    pout, pst = rctx.prove_batch(B, N, ins, ent)                # bbp_prove_batch on the same rows
    assert cst == [0] * B and pst == [0] * B
    w = rctx.witness_batch(b"".join(rc.b32(d) + rc.b32(k) + r.seed for d, k in r.bids))
    rs_ = bbp.record_size(N)
    for i, (rec, tail) in enumerate(_split(rows, N, bbp)):
        assert rec == cout[rs_ * i:rs_ * (i + 1)] == pout[rs_ * i:rs_ * (i + 1)], i
        assert tail == w[192 * i + 128:192 * i + 192] == r.tail(i), i  # q, z_img of bbp_witness_batch


def test_rows_go_unchanged_into_verify_rounds(rctx, bbp):
    N, B = 8, 5
    r = rc.honest(N, B, tag=3)
    rows, _, st = rctx.prove_round(N, r.table, r.bid_bytes, rc.entropy(9, B, N))
    assert st == [OK] * B
    assert rctx.verify_rounds([N], r.table, None, rows) == [OK] * B
    bad = bytearray(rows)
    bad[bbp.round_row_size(N) * 3 + bbp.record_size(N) + 5] ^= 0x20  # one byte of row 3's score
    assert rctx.verify_rounds([N], r.table, None, bytes(bad)) == [OK, OK, OK, VERIFY, OK]


def test_statuses_in_one_call(rctx, status_case, bbp):
    r, ent, (rows, toggles, st) = status_case
    assert st == r.status == [OK, BAD_ARG, FORMAT, FORMAT, OK, OK, OK, OK]
    assert toggles == r.toggles == [2, 0, 0, 0, 0, 7, 1, 3]
    parts = _split(rows, r.N, bbp)
    for i in (1, 2, 3):
        assert parts[i] == (bytes(bbp.record_size(r.N)), bytes(64)), i
    assert [t for _, t in parts] == [r.tail(i) for i in range(r.B)]
    good = [0, 4, 5, 6, 7]
    assert rctx.verify_rounds([r.N], r.table, None, b"".join(parts[i][0] + parts[i][1] for i in good)) == [OK] * 5
    # entropy is per row: the good rows' bytes are those of a call without the bad rows
    sub = rc.subset(r, good)
    es = bbp.entropy_size(r.N)
    rows2, toggles2, st2 = rctx.prove_round(r.N, sub.table, sub.bid_bytes, b"".join(ent[es * i:es * (i + 1)] for i in good))
    assert st2 == [OK] * 5 and toggles2 == [r.toggles[i] for i in good]
    assert _split(rows2, r.N, bbp) == [parts[i] for i in good]


def test_noncanonical_seed_refuses_every_row(rctx, bbp):
    r = rc.status_round(seed=rc.L)
    rows, toggles, st = rctx.prove_round(r.N, r.table, r.bid_bytes, rc.entropy(6, r.B, r.N))
    assert st == [FORMAT] * 8 and toggles == [0] * 8 and rows == bytes(len(rows))


def test_batch_crosses_a_wavefront(rctx, bbp):
    N, B = 8, 65
    r = rc.honest(N, B, tag=4)
    ent = rc.entropy(12, B, N)
    rows, toggles, st = rctx.prove_round(N, r.table, r.bid_bytes, ent)
    assert st == [OK] * B and toggles == r.toggles
    pout, pst = rctx.prove_batch(B, N, r.in_rows(), ent)
    assert pst == [OK] * B and rows == r.rows(pout)


@pytest.mark.parametrize("source", ["os", "device"])
def test_host_chunks_equal_the_unchunked_call(rctx, bbp, monkeypatch, source):
    """BBP_HOST_CHUNK_PROVE=3: a 7-bid call goes out as three engine calls.  Explicit entropy under source OS; under source DEVICE
    the call draws from a known key and every chunk draws its own row range of it (the row index is the bid's index in the call)."""
    N, B = 8, 7
    r = rc.honest(N, B, tag=5)
    ent = rc.entropy(13, B, N) if source == "os" else er.expand_prove(KEY, N, B)
    whole = rctx.prove_round(N, r.table, r.bid_bytes, ent)
    assert whole[2] == [OK] * B
    rctx.set_entropy_source(source)
    try:
        monkeypatch.setenv("BBP_HOST_CHUNK_PROVE", "3")
        if source == "device":
            rctx.debug_next_entropy_key(KEY)
        cut = rctx.prove_round(N, r.table, r.bid_bytes, ent if source == "os" else None)
        monkeypatch.delenv("BBP_HOST_CHUNK_PROVE")
    finally:
        rctx.set_entropy_source("os")
    assert cut == whole


def test_prepare_round_dev_writes_the_expanded_rows(rctx, status_case, bbp):
    import torch
    r = status_case[0]
    d_tab, d_bids = _dev(r.table), _dev(r.bid_bytes)
    d_in = torch.full(((7 * 32 + 32 * r.N + 8) * r.B,), 0xEE, dtype=torch.uint8, device="cuda")
    d_tail = torch.full((64 * r.B,), 0xEE, dtype=torch.uint8, device="cuda")
    d_tog = torch.full((r.B,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((r.B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rctx.prepare_round_dev(r.N, d_tab.data_ptr(), r.B, d_bids.data_ptr(), d_in.data_ptr(), d_st.data_ptr(), d_tail.data_ptr(), d_tog.data_ptr(),
                           stream=s.cuda_stream)
    s.synchronize()
    assert _host(d_in) == r.in_rows()  # byte-equal to the host-assembled rows; refused rows are zero
    assert _host(d_tail) == b"".join(r.tail(i) for i in range(r.B))
    assert d_tog.cpu().tolist() == r.toggles and d_st.cpu().tolist() == r.status


def test_two_prove_round_dev_calls_back_to_back(rctx, status_case, bbp):
    """Different tables, one non-default stream, ONE synchronise at the end: each call equals the host form.  The second call passes
    toggles_out_dev = NULL."""
    import torch
    r1, ent1, host1 = status_case
    r2 = rc.honest(3, 5, tag=6)
    ent2 = rc.entropy(14, r2.B, r2.N)
    host2 = rctx.prove_round(r2.N, r2.table, r2.bid_bytes, ent2)
    bufs = []
    s = torch.cuda.Stream()
    for r, ent, want_toggles in ((r1, ent1, True), (r2, ent2, False)):
        b = dict(tab=_dev(r.table), bids=_dev(r.bid_bytes), ent=_dev(ent),
                 rows=torch.full((bbp.round_row_size(r.N) * r.B,), 0xEE, dtype=torch.uint8, device="cuda"),
                 tog=torch.full((r.B,), -1, dtype=torch.int64, device="cuda") if want_toggles else None,
                 st=torch.full((r.B,), -1, dtype=torch.int32, device="cuda"))
        bufs.append(b)
    torch.cuda.synchronize()
    for r, b in zip((r1, r2), bufs):
        rctx.prove_round_dev(r.N, b["tab"].data_ptr(), r.B, b["bids"].data_ptr(), b["ent"].data_ptr(), b["rows"].data_ptr(), b["st"].data_ptr(),
                             toggles_ptr=b["tog"].data_ptr() if b["tog"] is not None else None, stream=s.cuda_stream)
    s.synchronize()
    for b, host in zip(bufs, (host1, host2)):
        assert _host(b["rows"]) == host[0]
        assert b["st"].cpu().tolist() == host[2]
        if b["tog"] is not None:
            assert b["tog"].cpu().tolist() == host[1]


def test_checked_round_reproves_a_corrupted_record(rctx, status_case, bbp):
    r, ent, plain = status_case
    rctx.set_prove_check(True)
    try:
        n0 = rctx.prove_check_stats()
        rctx.debug_corrupt_next_proof(4)  # a good row: its record fails the check once and is proved again from its bid
        rows, toggles, st = rctx.prove_round(r.N, r.table, r.bid_bytes, ent)
        n1 = rctx.prove_check_stats()
    finally:
        rctx.set_prove_check(False)
    assert st == r.status and st[1] == BAD_ARG  # all good rows OK, the missing bid still 4
    assert (rows, toggles) == plain[:2]          # the bytes of the unchecked call
    assert n1[2] - n0[2] == 1 and n1[0] - n0[0] == r.B


def test_pool_splits_bids_in_request_order(rctx, bbp):
    import torch
    N, B = 8, 5
    r = rc.honest(N, B, tag=7)
    ent = rc.entropy(15, B, N)
    want = rctx.prove_round(N, r.table, r.bid_bytes, ent)
    pool = bbp.Pool([0, 0])
    try:
        assert pool.prove_round(N, r.table, r.bid_bytes, ent) == want
        # 3 + 2: each member's block equals the context's call on those bids
        for m, (lo, hi) in enumerate(((0, 3), (3, 5))):
            sub = rc.subset(r, list(range(lo, hi)))
            es = bbp.entropy_size(N)
            got = pool.member(m).prove_round(N, sub.table, sub.bid_bytes, ent[es * lo:es * hi])
            row = bbp.round_row_size(N)
            assert got == (want[0][row * lo:row * hi], want[1][lo:hi], want[2][lo:hi]), m
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        assert bbp.lib.bbp_prove_round_dev(pool.handle, N, p, 1, p, p, p, None, p, None) == BAD_ARG
        assert bbp.lib.bbp_prepare_round_dev(pool.handle, N, p, 1, p, p, None, None, p, None) == BAD_ARG
    finally:
        pool.close()


def test_screening_order(rctx, bbp):
    """A NULL required pointer first, then N (0: BAD_ARG, above 202: GENS_LEN), then B == 0: OK -- in every form."""
    import torch
    lib, h = bbp.lib, rctx.handle
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    buf = (bbp.lib.bbp_round_row_size(8) * 2 * b"\0")
    one = bytes(64)
    st = (ctypes.c_int32 * 2)()
    # host form: round, bids, rows_out, status are required; toggles_out and entropy are not
    assert lib.bbp_prove_round(h, 0, None, 1, one, None, buf, None, st) == BAD_ARG  # NULL beats N == 0 ...
    assert lib.bbp_prove_round(h, 203, one, 1, None, None, buf, None, st) == BAD_ARG
    assert lib.bbp_prove_round(h, 8, one, 1, one, None, None, None, st) == BAD_ARG
    assert lib.bbp_prove_round(h, 8, one, 1, one, None, buf, None, None) == BAD_ARG
    assert lib.bbp_prove_round(h, 0, one, 0, one, None, buf, None, st) == BAD_ARG     # ... N beats B == 0
    assert lib.bbp_prove_round(h, 203, one, 0, one, None, buf, None, st) == 2
    assert lib.bbp_prove_round(h, 8, one, 0, one, None, buf, None, st) == OK
    assert lib.bbp_prove_round_dev(h, 0, p, 1, p, None, p, None, p, None) == BAD_ARG  # entropy_dev is required
    assert lib.bbp_prove_round_dev(h, 0, p, 0, p, p, p, None, p, None) == BAD_ARG
    assert lib.bbp_prove_round_dev(h, 203, p, 0, p, p, p, None, p, None) == 2
    assert lib.bbp_prove_round_dev(h, 8, p, 0, p, p, p, None, p, None) == OK
    assert lib.bbp_prepare_round_dev(h, 203, p, 1, p, None, None, None, p, None) == BAD_ARG  # prove_in_dev is required
    assert lib.bbp_prepare_round_dev(h, 8, p, 1, p, p, None, None, None, None) == BAD_ARG     # status_dev is required
    assert lib.bbp_prepare_round_dev(h, 0, p, 0, p, p, None, None, p, None) == BAD_ARG
    assert lib.bbp_prepare_round_dev(h, 203, p, 0, p, p, None, None, p, None) == 2
    assert lib.bbp_prepare_round_dev(h, 8, p, 0, p, p, None, None, p, None) == OK


def _allocs(c):
    m = re.search(r"in (\d+) allocation\(s\) since bbp_init", c.describe())
    assert m
    return int(m.group(1))


def test_reserved_context_allocates_nothing_in_round_calls(bbp, ctx):
    import torch
    N = 8
    c = bbp.Context(0)
    try:
        c.reserve(64, N)
        a0 = _allocs(c)
        assert a0 > 0
        for B in (64, 5, 33):  # three staging slots
            r = rc.honest(N, B, tag=8)
            rows, _, st = c.prove_round(N, r.table, r.bid_bytes, rc.entropy(16, B, N))
            assert st == [OK] * B and c.verify_rounds([N], r.table, None, rows) == [OK] * B
        r = rc.honest(N, 64, tag=8)
        d_tab, d_bids, d_ent = _dev(r.table), _dev(r.bid_bytes), _dev(rc.entropy(16, 64, N))
        d_rows = torch.zeros(bbp.round_row_size(N) * 64, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.prove_round_dev(N, d_tab.data_ptr(), 64, d_bids.data_ptr(), d_ent.data_ptr(), d_rows.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [OK] * 64
        assert _allocs(c) == a0, (a0, _allocs(c))
    finally:
        c.close()


def test_reserved_context_allocates_nothing_in_checked_calls(bbp, ctx):
    """bbp_reserve on a context with checked proving on sizes every staging buffer for a checked call: the check's weights travel
    behind the prover's entropy (32 bytes per row more than an unchecked call uploads).  (640, 1) is the smallest shape at which a
    slot's entropy buffer sized for unchecked calls (a row of 192 bytes plus an eighth of slack) is too small for that."""
    N, B = 1, 640
    r = rc.honest(N, B, tag=8)
    rows, ent = r.in_rows(), rc.entropy(17, B, N)
    c = bbp.Context(0)
    try:
        c.set_prove_check(True)
        c.reserve(B, N)
        a0 = _allocs(c)
        assert a0 > 0
        results = [c.prove_batch(B, N, rows, ent) for _ in range(3)]  # three staging slots
        c.set_entropy_source("device")
        results.append(c.prove_batch(B, N, rows))
        assert _allocs(c) == a0, (a0, _allocs(c))
        rs_ = bbp.record_size(N)
        for recs, st in results:
            assert st == [OK] * B
            vin = b"".join(recs[rs_ * i:rs_ * (i + 1)] + r.tail(i) + r.table for i in range(B))
            assert c.verify_batch(B, N, vin) == [OK] * B
        assert c.health() == 0
    finally:
        c.close()
