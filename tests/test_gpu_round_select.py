"""GPU tier: selecting a round's bids (include/bbp.h bbp_select_round_dev, bbp_prove_round_select, bbp_debug_round_select).  Scores and
statuses are held against bbp_witness_batch and bbp_prove_round, selections against the model of tests/round_select_cases.py, rows
against bbp_prepare_round_dev and bbp_prove_round on the gathered bids -- the calls the feature is defined as equal to."""
import ctypes

import pytest

from tests import prove_round_cases as rc
from tests import round_select_cases as sc

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG = 0, 1, 3, 4
TAG_MSM = 1
KEY = bytes((0x5A ^ (11 * i)) & 0xFF for i in range(32))
FILL = 0x6E


@pytest.fixture(scope="module")
def sctx(ctx, bbp):
    """A context of this module's own (settings are switched here; after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _scores(r):
    """the oracle's score of every bid (0 for a refused one)"""
    return [e[2]["q"] if e[0] == OK else 0 for e in r.expect]


def _select_dev(c, r, floor, K, cap, expand=False, stream=None):
    """One select_round_dev call; every output buffer starts as FILL bytes.  Returns host copies."""
    import torch
    B, N = r.B, r.N
    d_tab, d_bids = _dev(r.table), _dev(r.bid_bytes)

    def fill(n):
        return torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    o = dict(sel=fill(4 * cap), counts=fill(8), status=fill(4 * B), scores=fill(32 * B), tab=d_tab, bids=d_bids)  # (inputs: kept alive with the outputs)
    if expand:
        o.update(prove_in=fill((7 * 32 + 32 * N + 8) * cap), tails=fill(64 * cap), toggles=fill(8 * cap))
    torch.cuda.synchronize()
    s = stream or torch.cuda.Stream()
    c.select_round_dev(N, d_tab.data_ptr(), B, d_bids.data_ptr(), floor, K, cap, o["sel"].data_ptr(), o["counts"].data_ptr(), o["status"].data_ptr(),
                       o["scores"].data_ptr(), *([o[k].data_ptr() for k in ("prove_in", "tails", "toggles")] if expand else [None] * 3), stream=s.cuda_stream)
    if stream is not None:
        return o
    s.synchronize()
    h = {k: _host(v) for k, v in o.items()}
    h["n_sel"], h["n_qualified"] = (int.from_bytes(h["counts"][i:i + 4], "little") for i in (0, 4))
    n = min(h["n_sel"], cap)
    h["sel_list"] = [int.from_bytes(h["sel"][4 * j:4 * j + 4], "little") for j in range(n)]
    assert h["sel"][4 * n:4 * max(cap, 1)] == bytes([FILL]) * (4 * max(cap, 1) - 4 * n) or cap == 0  # entries at or beyond n_sel are not written
    h["status_list"] = [int.from_bytes(h["status"][4 * i:4 * i + 4], "little", signed=True) for i in range(B)]
    h["score_list"] = [int.from_bytes(h["scores"][32 * i:32 * i + 32], "little") for i in range(B)]
    return h


def _refusing(r, every=5):
    """r with every fifth bid refused, alternating a non-canonical k (FORMAT) and a bid that is not in the list (BAD_ARG)"""
    bids, expect = list(r.bids), list(r.expect)
    for n, i in enumerate(range(2, r.B, every)):
        if n % 2 == 0:
            bids[i], expect[i] = (bids[i][0], rc.L + 5), (FORMAT, 0, None)
        else:
            bids[i], expect[i] = (bids[i][0] ^ 1, bids[i][1]), (BAD_ARG, 0, None)
    return rc.Round(r.N, r.seed, r.items, bids, expect)


@pytest.fixture(scope="module")
def r70():
    """N = 3, B = 70 (crosses a wavefront): three distinct bids in rotation, so every score is tied many times"""
    return rc.honest(3, 70, tag=21)


@pytest.fixture(scope="module")
def r70_refusing(r70):
    return _refusing(r70)


def test_scores_and_statuses(sctx, bbp):
    r = rc.status_round()
    got = _select_dev(sctx, r, 0, 0, r.B)
    want_rows, _, want_st = sctx.prove_round(r.N, r.table, r.bid_bytes, rc.entropy(31, r.B, r.N))
    assert got["status_list"] == want_st == r.status
    w = sctx.witness_batch(b"".join(rc.b32(d % rc.L) + rc.b32(k % rc.L) + r.seed for d, k in r.bids))
    for i in range(r.B):
        q = w[192 * i + 128:192 * i + 160] if r.status[i] == OK else bytes(32)
        assert got["scores"][32 * i:32 * i + 32] == q == rc.b32(_scores(r)[i]), i
    ok = [i for i in range(r.B) if r.status[i] == OK]
    assert got["sel_list"] == ok and (got["n_sel"], got["n_qualified"]) == (len(ok), len(ok))
    bad = rc.status_round(seed=rc.L)  # a non-canonical seed: every bid FORMAT, nothing qualifies
    got = _select_dev(sctx, bad, 0, 0, bad.B)
    assert got["status_list"] == [FORMAT] * 8 and got["score_list"] == [0] * 8 and (got["n_sel"], got["n_qualified"]) == (0, 0)


def test_neighbours_of_refused_bids(sctx, r70, r70_refusing):
    honest = _select_dev(sctx, r70, 0, 0, 70)
    assert honest["status_list"] == [OK] * 70 and honest["score_list"] == _scores(r70)
    got = _select_dev(sctx, r70_refusing, 0, 0, 70)
    assert got["status_list"] == r70_refusing.status and {OK, FORMAT, BAD_ARG} == set(r70_refusing.status)
    for i in range(70):
        assert got["score_list"][i] == (honest["score_list"][i] if r70_refusing.status[i] == OK else 0), i
    assert got["sel_list"] == [i for i in range(70) if r70_refusing.status[i] == OK]


def _floors(scores, statuses):
    ok = sorted(s for s, st in zip(scores, statuses) if st == OK)
    return [0, ok[len(ok) // 2], ok[0], ok[-1] + 1, sc.ALL_ONES]


@pytest.mark.parametrize("K", [0, 1, 5, 70])
def test_selection_against_the_model(sctx, r70_refusing, K):
    r = r70_refusing
    scores = _scores(r)
    for floor in _floors(scores, r.status):
        want = sc.model(scores, r.status, floor, K)
        got = _select_dev(sctx, r, floor, K, 70)
        assert (got["sel_list"], got["n_sel"], got["n_qualified"]) == want, (floor, K)
        if want[1] > 3:  # n_sel > cap: the first cap entries in index order, the counts still true
            cut = _select_dev(sctx, r, floor, K, 3)
            assert (cut["sel_list"], cut["n_sel"], cut["n_qualified"]) == (want[0][:3], want[1], want[2]), (floor, K)


def test_workgroup_boundary_and_ties(sctx):
    """N = 2, B = 1100: two distinct bids alternate, so each score is tied 550 times with copies on both sides of index 1024.  Each K
    puts the K-th place inside a tie: among the better bid's copies near the start, and among the other's copies beyond index 1024."""
    r = rc.honest(2, 1100, tag=22)
    scores = _scores(r)
    assert len(set(scores)) == 2
    for K in (3, 550 + 5, 550 + 513, 1099):
        want = sc.model(scores, r.status, 0, K)
        got = _select_dev(sctx, r, 0, K, 1100)
        assert (got["sel_list"], got["n_sel"], got["n_qualified"]) == want, K
    assert max(sc.model(scores, r.status, 0, 550 + 513)[0]) > 1024


@pytest.mark.parametrize("name", ["top31", "equal", "lastword"])
def test_deep_radix_passes(sctx, name):
    if name == "top31":
        c = sc.cluster(256, 5, 8)
        scores = c + c[:44]                                                # 300 scores that share their top 31 bytes (44 of them twice)
    elif name == "equal":
        scores = [sc.cluster(1, 6, 8)[0]] * 300
    else:
        scores = sc.cluster(2049, 7, 32)                                   # distinct in the last word only
    B = len(scores)
    statuses = [OK] * B
    for i in (1, B // 2):
        statuses[i] = BAD_ARG
    for K in (1, 17, B - 1):
        for floor in (0, min(scores), max(scores), max(scores) + 1):
            want = sc.model(scores, statuses, floor, K)
            got = sctx.debug_round_select(b"".join(sc.b32(s) for s in scores), statuses, floor, K)
            assert got == want, (name, K, floor)


def test_every_workgroup_of_the_selection(sctx):
    """B = 2^18 + 1: the most workgroups the selection launches, the last ones with nothing to walk; distinct 20-bit tails under one
    prefix, so three radix passes decide and the early stop is taken in a pass that many workgroups share."""
    B = (1 << 18) + 1
    scores = sc.cluster(B, 8, 20)
    statuses = [OK] * B
    statuses[5] = statuses[B - 2] = FORMAT
    raw = b"".join(sc.b32(s) for s in scores)
    for K, floor in ((1, 0), (4097, 0), (B, 0), (300, sorted(scores)[B - 200])):
        assert sctx.debug_round_select(raw, statuses, floor, K) == sc.model(scores, statuses, floor, K), (K, floor)


def test_debug_hook_refuses_bad_input(sctx, bbp):
    one = sc.b32(5)
    with pytest.raises(bbp.BbpError) as e:
        sctx.debug_round_select(sc.b32(sc.L), [OK])
    assert e.value.status == BAD_ARG
    with pytest.raises(bbp.BbpError) as e:
        sctx.debug_round_select(one, [VERIFY])
    assert e.value.status == BAD_ARG
    with pytest.raises(bbp.BbpError) as e:
        sctx.debug_round_select(b"", [])
    assert e.value.status == BAD_ARG
    assert sctx.debug_round_select(one, [OK], 5, 1) == ([0], 1, 1)


def test_compacted_rows_and_a_following_prove(sctx, r70_refusing, bbp):
    import torch
    r = r70_refusing
    N, B, K, cap = r.N, r.B, 5, 8
    floor = _floors(_scores(r), r.status)[1]
    want_sel = sc.model(_scores(r), r.status, floor, K)[0]
    assert len(want_sel) == 5
    # bbp_prepare_round_dev over all bids: the rows the compacted ones must equal
    pin, row = 7 * 32 + 32 * N + 8, bbp.round_row_size(N)
    d_tab, d_bids = _dev(r.table), _dev(r.bid_bytes)
    a_in, a_tail = torch.zeros(pin * B, dtype=torch.uint8, device="cuda"), torch.zeros(64 * B, dtype=torch.uint8, device="cuda")
    a_tog, a_st = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sctx.prepare_round_dev(N, d_tab.data_ptr(), B, d_bids.data_ptr(), a_in.data_ptr(), a_st.data_ptr(), a_tail.data_ptr(), a_tog.data_ptr())
    torch.cuda.synchronize()
    all_in, all_tail, all_tog = _host(a_in), _host(a_tail), a_tog.cpu().tolist()
    # the select call and, with no ordering by the caller, the prove call on another stream
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ent = rc.entropy(32, 5, N)
    d_ent = _dev(ent)
    d_rec = torch.zeros(bbp.record_size(N) * 5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    o = _select_dev(sctx, r, floor, K, cap, expand=True, stream=s1)
    sctx.prove_batch_dev(5, N, o["prove_in"].data_ptr(), d_ent.data_ptr(), d_rec.data_ptr(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    h = {k: _host(v) for k, v in o.items()}
    assert [int.from_bytes(h["sel"][4 * j:4 * j + 4], "little") for j in range(5)] == want_sel
    for j, i in enumerate(want_sel):
        assert h["prove_in"][pin * j:pin * (j + 1)] == all_in[pin * i:pin * (i + 1)] == r.in_row(i), j
        assert h["tails"][64 * j:64 * (j + 1)] == all_tail[64 * i:64 * (i + 1)] == r.tail(i), j
        assert int.from_bytes(h["toggles"][8 * j:8 * (j + 1)], "little") == all_tog[i] == r.toggles[i], j
    for k, per in (("prove_in", pin), ("tails", 64), ("toggles", 8), ("sel", 4)):  # rows at or beyond n_sel are not written
        assert h[k][per * 5:per * cap] == bytes([FILL]) * (per * (cap - 5)), k
    recs, rs_ = _host(d_rec), bbp.record_size(N)
    rows = b"".join(recs[rs_ * j:rs_ * (j + 1)] + h["tails"][64 * j:64 * (j + 1)] for j in range(5))
    assert sctx.verify_rounds([N], r.table, None, rows) == [OK] * 5
    want_rows, _, st = sctx.prove_round(N, r.table, rc.subset(r, want_sel).bid_bytes, ent)
    assert st == [OK] * 5 and rows == want_rows and len(rows) == row * 5


@pytest.mark.parametrize("N,B,K", [(2, 70, 3), (202, 3, 1)])
def test_host_call_parity(sctx, bbp, N, B, K):
    r = _refusing(rc.honest(N, B, tag=23)) if B > 5 else rc.honest(N, B, tag=23)
    scores = _scores(r)
    ent = rc.entropy(33, K, N)
    got = sctx.prove_round_select(N, r.table, r.bid_bytes, 0, K, entropy=ent, want_scores=True)
    want_sel, n_sel, n_q = sc.model(scores, r.status, 0, K)
    assert (got.sel, got.n_sel, got.n_qualified) == (want_sel, n_sel, n_q) and n_sel == K
    assert got.status == r.status and got.scores == b"".join(rc.b32(s) for s in scores)
    rows, toggles, st = sctx.prove_round(N, r.table, rc.subset(r, want_sel).bid_bytes, ent)
    assert st == [OK] * K and (got.rows, got.toggles) == (rows, toggles)
    assert sctx.verify_rounds([N], r.table, None, got.rows) == [OK] * K


def test_host_call_with_no_floor_and_no_k_is_prove_round_over_the_accepted_bids(sctx, bbp):
    r = rc.status_round()
    ok = [i for i in range(r.B) if r.status[i] == OK]
    ent = rc.entropy(34, r.B, r.N)  # cap defaults to B: the first five rows are used
    got = sctx.prove_round_select(r.N, r.table, r.bid_bytes, entropy=ent)
    es = bbp.entropy_size(r.N)
    rows, toggles, st = sctx.prove_round(r.N, r.table, rc.subset(r, ok).bid_bytes, ent[:es * len(ok)])
    assert st == [OK] * len(ok) and (got.rows, got.sel, got.toggles, got.status) == (rows, ok, toggles, r.status)
    assert (got.n_sel, got.n_qualified, got.scores) == (len(ok), len(ok), None)


@pytest.mark.parametrize("source", ["device", "hedged"])
def test_device_entropy(sctx, source):
    r = rc.status_round()
    scores = _scores(r)
    want_sel = sc.model(scores, r.status, 0, 3)[0]
    sctx.set_entropy_source(source)
    try:
        sctx.debug_next_entropy_key(KEY)
        got = sctx.prove_round_select(r.N, r.table, r.bid_bytes, 0, 3)
        sctx.debug_next_entropy_key(KEY)
        want = sctx.prove_round(r.N, r.table, rc.subset(r, want_sel).bid_bytes)
    finally:
        sctx.set_entropy_source("os")
    assert got.sel == want_sel and (got.rows, got.toggles) == want[:2] and want[2] == [OK] * 3


def test_checked_proving_reproves_a_corrupted_record(sctx):
    r = rc.status_round()
    ent = rc.entropy(35, 3, r.N)
    plain = sctx.prove_round_select(r.N, r.table, r.bid_bytes, 0, 3, entropy=ent)
    sctx.set_prove_check(True)
    try:
        n0 = sctx.prove_check_stats()
        sctx.debug_corrupt_next_proof(1)
        got = sctx.prove_round_select(r.N, r.table, r.bid_bytes, 0, 3, entropy=ent)
        n1 = sctx.prove_check_stats()
    finally:
        sctx.set_prove_check(False)
    assert got == plain and got.rc == OK and got.n_sel == 3
    assert n1[2] - n0[2] == 1 and n1[0] - n0[0] == 3


def test_buffer_too_small_and_nothing_selected(sctx, bbp):
    r = rc.status_round()
    N, B, cap = r.N, r.B, 2
    with pytest.raises(bbp.BbpError) as e:
        sctx.prove_round_select(N, r.table, r.bid_bytes, cap=cap)
    assert e.value.status == BAD_ARG and "5 bids selected" in str(e.value) and "room for 2" in str(e.value)
    lib = bbp.lib
    u8 = ctypes.c_uint8
    rows = (u8 * (cap * bbp.round_row_size(N)))(*([FILL] * (cap * bbp.round_row_size(N))))
    sel = (ctypes.c_uint32 * cap)(*([0x6E6E6E6E] * cap))
    scores, status = (u8 * (32 * B))(), (ctypes.c_int32 * B)(*([-1] * B))
    n_sel, n_q = ctypes.c_uint32(77), ctypes.c_uint32(77)
    tab, bids, floor = (u8 * len(r.table)).from_buffer_copy(r.table), (u8 * len(r.bid_bytes)).from_buffer_copy(r.bid_bytes), (u8 * 32)()
    ent = rc.entropy(36, cap, N)
    rc_ = lib.bbp_prove_round_select(sctx.handle, N, tab, B, bids, floor, 0, cap, (u8 * len(ent)).from_buffer_copy(ent), rows, sel, ctypes.byref(n_sel),
                                     ctypes.byref(n_q), None, scores, status)
    assert rc_ == BAD_ARG and (n_sel.value, n_q.value) == (5, 5)
    assert list(status) == r.status and bytes(scores) == b"".join(rc.b32(s) for s in _scores(r))
    assert bytes(rows) == bytes([FILL]) * len(rows) and list(sel) == [0x6E6E6E6E] * cap  # untouched: nothing was proved
    # nothing selected: BBP_OK, no prove call (no MSM launch)
    sctx.set_profiling(True)
    sctx.last_timings()
    got = sctx.prove_round_select(N, r.table, r.bid_bytes, sc.ALL_ONES, 0, cap=0, want_scores=True)
    tags = [int(t) for t, _ in sctx.last_timings()]
    sctx.set_profiling(False)
    assert (got.rc, got.n_sel, got.n_qualified, got.sel, got.rows) == (OK, 0, 0, [], b"") and tags and TAG_MSM not in tags
    assert got.status == r.status and got.scores == bytes(scores)  # scoring alone: the all-ones floor and cap = 0


def test_screening_order(sctx, bbp):
    import torch
    lib, h = bbp.lib, sctx.handle
    one, st, n = bytes(64), (ctypes.c_int32 * 2)(), ctypes.c_uint32()
    big = bbp.SELECT_MAX_BIDS + 1
    args = lambda N, B: (h, N, one, B, one, one, 0, 0, None, None, None, ctypes.byref(n), None, None, None, st)  # noqa: E731
    assert lib.bbp_prove_round_select(h, 0, None, 1, one, one, 0, 0, None, None, None, ctypes.byref(n), None, None, None, st) == BAD_ARG
    assert lib.bbp_prove_round_select(h, 8, one, 1, one, one, 0, 1, None, None, None, ctypes.byref(n), None, None, None, st) == BAD_ARG  # cap > 0
    assert lib.bbp_prove_round_select(*args(0, big)) == BAD_ARG
    assert lib.bbp_prove_round_select(*args(203, big)) == 2
    assert lib.bbp_prove_round_select(*args(8, big)) == BAD_ARG
    n.value = 9
    assert lib.bbp_prove_round_select(*args(8, 0)) == OK and n.value == 0
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    assert lib.bbp_select_round_dev(h, 8, p, 1, p, None, 0, 0, None, p, p, None, None, None, None, None) == BAD_ARG   # floor32
    assert lib.bbp_select_round_dev(h, 8, p, 1, p, one, 0, 1, None, p, p, None, None, None, None, None) == BAD_ARG    # sel_dev with cap > 0
    assert lib.bbp_select_round_dev(h, 203, p, 1, p, one, 0, 0, None, p, p, None, None, None, None, None) == 2
    assert lib.bbp_select_round_dev(h, 8, p, big, p, one, 0, 0, None, p, p, None, None, None, None, None) == BAD_ARG
    d[:8] = FILL
    torch.cuda.synchronize()
    assert lib.bbp_select_round_dev(h, 8, p, 0, p, one, 0, 0, None, p, p, None, None, None, None, None) == OK
    torch.cuda.synchronize()
    assert d[:8].cpu().tolist() == [0] * 8  # B == 0: zero counts, in stream order


def test_secret_wiping(bbp, ctx):
    r = rc.status_round()
    ent = rc.entropy(37, 2, r.N)
    c = bbp.Context(0)
    try:
        plain = c.prove_round_select(r.N, r.table, r.bid_bytes, 0, 2, entropy=ent, want_scores=True)
        c.set_secret_wipe(True)
        got = c.prove_round_select(r.N, r.table, r.bid_bytes, 0, 2, entropy=ent, want_scores=True)
        assert c.debug_secret_residue()[:2] == (0, 0), c.debug_secret_residue()
        unselected = [i for i in range(r.B) if r.status[i] == OK and i not in got.sel]
        assert unselected and c.debug_secret_scan(rc.b32(r.bids[unselected[0]][1])) == (0, 0)
        assert c.debug_secret_scan(rc.b32(r.bids[got.sel[0]][1])) == (0, 0)
        assert got == plain and got.n_sel == 2
        # the device form: the ring entry is erased on the stream, ahead of its event
        _select_dev(c, r, 0, 2, 2, expand=True)
        assert c.debug_secret_residue()[:2] == (0, 0), c.debug_secret_residue()
        assert c.health() == 0
    finally:
        c.close()


def test_pool(sctx, bbp):
    import torch
    r = _refusing(rc.honest(8, 12, tag=24))
    ent = rc.entropy(38, 5, r.N)
    want = sctx.prove_round_select(r.N, r.table, r.bid_bytes, 0, 5, entropy=ent, want_scores=True)
    assert want.n_sel == 5
    pool = bbp.Pool([0, 0])
    try:
        assert pool.prove_round_select(r.N, r.table, r.bid_bytes, 0, 5, entropy=ent, want_scores=True) == want
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        one, n = bytes(64), ctypes.c_uint32()
        assert bbp.lib.bbp_select_round_dev(pool.handle, 8, p, 1, p, one, 0, 0, None, p, p, None, None, None, None, None) == BAD_ARG
        assert bbp.lib.bbp_debug_round_select(pool.handle, 1, one, one, one, 0, 0, None, ctypes.byref(n), ctypes.byref(n)) == BAD_ARG
    finally:
        pool.close()
