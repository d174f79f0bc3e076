"""GPU tier: no call may read scratch it has not written (DESIGN.md "Scratch discipline").

Every case warms a context with calls of a different, larger shape -- so the buffers exist and the carve of the call under test lies
somewhere else inside them -- and with calls of the shape under test itself, because which buffers a call takes and how large they are
is not monotonic in its size (an MSM launch of 33 is cut into sub-MSMs and needs more scratch than one of 140).  A warm call only
allocates: the fill that follows leaves nothing of it.  Then the case fills every scratch buffer, ring, staging slot and pinned mirror
with a small word (bbp_debug_poison_scratch; csrc/secret_map.h exempts an open standing's entries and nothing else), runs the call and
compares it with its reference: the C oracle, or the Python model of the family applied to the oracle's verdicts.  Both words of poison_cases.WORDS run:
one alone can happen to be neutral.  After every case the call under test has allocated nothing (it ran over filled memory only) and
the health word is zero.  Builders: tests/poison_cases.py.

    family                                            filled scratch it runs over                                   reference
    prove_batch, prove_batch_dev, checked, pool       batch[0..2], raw[], sorted, pts, slice_*, io[0..2].*, h_in/h_out   C oracle's records
    verify: uniform, mixed, rounds; plain and G = 8   batch[3 + lane], vl.misc / agg / agg_io, slice_*[4 + lane],    C oracle's verdicts,
                                                      io[3..].*, ns_ring                                            _expected_fallback
    msm_batch (split, unsplit)                        scal, enc, sorted, pts                                        C oracle's points
    witness_batch, prepare_bids_dev                   io_in, io_out (the latter writes the caller's buffers only)   C oracle's witness
    prove_round, prove_round_dev                      io[].*, rnd[], the prove buffers                              C oracle's records
    select_round_dev, prove_round_select, its hook    sel, sel.h, rnd[], the prove buffers                          selection model, oracle
    verify_round(s)_best[_distinct], their hooks      best, best.h, best.rows, the verifier lanes                   the models on the oracle's verdicts
    standing_offer, standing_read                     as above; stand[] is exempt and persists                      standing model, truth()
    draw_entropy_dev, draw_entropy_hedged_dev         (the caller's buffers only)                                   entropy_ref, hedge_ref"""
import ctypes

import pytest

from tests import entropy_ref as er
from tests import hedge_ref as hr
from tests import msm_cases as mc
from tests import poison_cases as pc
from tests import prove_round_cases as rc
from tests import round_best_cases as bc
from tests import round_best_distinct_cases as dc
from tests import round_select_cases as sc
from tests import round_standing_cases as stc
from tests import rounds_best_cases as mbc
from tests import rounds_best_distinct_cases as mdc
from tests import test_gpu_verify_rounds as vr
from tests.test_gpu_verify_mixed import oc  # noqa: F401  (fixture: the C oracle)
from tests.test_gpu_verify_plan import NS, proved  # noqa: F401  (fixture: one oracle-proved row and its tampered copy per N)

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG = pc.OK, pc.VERIFY, pc.FORMAT, pc.BAD_ARG
WORDS = pc.WORDS
G = pc.G
SIZES = (130, 1, 65, 33, 130)  # grows, shrinks and regrows the carve; crosses 128 (split MSMs), 32 | 33 (wavefront transcripts, wide IPA
#                               round) and 64 | 65 (the folded-generator tail with slice_vtab and fpts)
KEY = bytes((0x3C ^ (5 * i)) & 0xFF for i in range(32))
FILL = 0x6E


def _own_context(bbp):
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def pctx(ctx, bbp):
    """the prove-side context of this module (after `ctx`, so torch's HIP runtime is initialised first)"""
    yield from _own_context(bbp)


@pytest.fixture(scope="module")
def vctx(ctx, bbp):
    """the verify-side context of this module"""
    yield from _own_context(bbp)


# ---- the rows every prove case shares: proved once by the C oracle, never changed --------------------------------------------------------
@pytest.fixture(scope="module")
def rows130(oc, bbp):
    return pc.proved_rows(oc, bbp, 130, 1, seed=130001)


@pytest.fixture(scope="module")
def rows8(oc, bbp):
    return pc.proved_rows(oc, bbp, 5, 8, seed=5008)


@pytest.fixture(scope="module")
def rows202(oc, bbp):
    return pc.proved_rows(oc, bbp, 2, 202, seed=2202)


def _warm_prove(c, p, sizes, form="host"):
    """calls of the sizes the case runs -- the same paths, the same buffers -- at another list length, so every array of the carve starts
    somewhere else; repeated over the rotation of batch buffers and staging slots"""
    for B in sorted(set(sizes), reverse=True):
        for _ in range(pc.WARM_CALLS):
            if form == "host":
                _, st = c.prove_batch(*pc.tiled(p, B))
                assert st == [OK] * B
            else:
                _prove_dev(c, pc.tiled(p, B), p.rs)


def _prove_dev(c, args, rs_):
    import torch
    B, N, ins, ents = args
    d_in, d_ent, d_out = pc.dev(ins), pc.dev(ents), pc.filled(B * rs_)
    torch.cuda.synchronize()
    c.prove_batch_dev(B, N, d_in.data_ptr(), d_ent.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    return pc.host(d_out)


def _poisoned(c, word, call):
    """the call once per buffer of every rotation it takes part in, the fill, and the call under test"""
    for _ in range(pc.WARM_CALLS):
        call()
    with pc.Poisoned(c, word):
        return call()


def _sequence(c, p, word):
    for call, B in enumerate(SIZES):
        with pc.Poisoned(c, word):
            out, st = c.prove_batch(*pc.prove_args(p, B))
        assert st == [OK] * B, (call, B)
        wrong = [i for i in range(B) if out[i * p.rs:(i + 1) * p.rs] != p.records[i]]
        assert not wrong, (call, B, wrong[:8])


# ---- 1. the hook itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", WORDS)
def test_hook_fills_what_it_reports(pctx, vctx, rows8, word):
    _warm_prove(pctx, rows8, (6,))
    for c in (pctx, vctx):
        dev_bytes, host_bytes, n_buffers = c.debug_poison_scratch(word)
        dev16, host16 = c.debug_secret_scan(pc.pattern(word))
        dev4, host4 = c.debug_secret_scan(pc.pattern(word)[:4])
        if c is pctx:
            assert n_buffers >= 5 and dev_bytes > 1 << 20 and host_bytes > 8192
        # a buffer of w whole words holds the 16-byte pattern at w - 3 offsets; capacities are whole 16-byte grains
        # (the 4-byte scan of the device also meets the word in the resident tables -- a point's Z = 1 --: no count is asked of it)
        assert dev16 == dev_bytes // 4 - 3 * n_buffers and dev4 >= dev_bytes // 4
        n_host = (host4 - host16) // 3
        assert host4 == host_bytes // 4 and host16 == host_bytes // 4 - 3 * n_host and (host_bytes == 0 or n_host >= 1)
        other = 4 - word
        assert c.debug_secret_scan(pc.pattern(other)) == (0, 0)  # the other word is nowhere: the fill is this call's
        assert c.health() == 0


def test_hook_refuses_a_pool_and_null_pointers(bbp, pctx):
    n64, n32 = ctypes.c_uint64(), ctypes.c_uint32()
    a, b, n = ctypes.byref(n64), ctypes.byref(n64), ctypes.byref(n32)
    lib = bbp.lib
    for args in ((None, b, n), (a, None, n), (a, b, None)):
        assert lib.bbp_debug_poison_scratch(pctx.handle, 1, 0, *args) == BAD_ARG
    assert lib.bbp_debug_poison_scratch(None, 1, 0, a, b, n) == BAD_ARG
    pool = bbp.Pool([0, 0])
    try:
        assert lib.bbp_debug_poison_scratch(pool.handle, 1, 0, a, b, n) == BAD_ARG
        assert pool.member(0).debug_poison_scratch(1)[2] >= 0
    finally:
        pool.close()


@pytest.mark.parametrize("word", WORDS)
def test_sticky_fresh_context_and_regrowth(bbp, ctx, rows8, rows130, word):
    """No warm call: the first call of a fresh context allocates every buffer it uses, and a later, larger one allocates them again --
    with `sticky` they start out as the word.  The grown buffers' slack still holds it afterwards."""
    c = bbp.Context(0)
    try:
        c.debug_poison_scratch(word, sticky=True)
        before = pc.allocations(c)
        out, st = c.prove_batch(*pc.prove_args(rows8, 5))
        assert st == [OK] * 5 and out == b"".join(rows8.records)
        first = pc.allocations(c)
        assert first > before and c.debug_secret_scan(pc.pattern(word))[0] > 0
        out, st = c.prove_batch(*pc.prove_args(rows130, 33))  # grows the batch buffer, the MSM scratch and the staging slot
        assert st == [OK] * 33 and out == b"".join(rows130.records[:33])
        assert pc.allocations(c) > first and c.debug_secret_scan(pc.pattern(word))[0] > 0
        c.debug_poison_scratch(word, sticky=False)  # a later allocation is the driver's again
        assert c.health() == 0
    finally:
        c.close()


# ---- 2. prove ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warmed_pctx(pctx, rows8, rows202):
    _warm_prove(pctx, rows8, SIZES + (6,))
    _warm_prove(pctx, rows8, (6, 3), form="dev")
    _warm_prove(pctx, rows202, (3,))
    _warm_prove(pctx, rows202, (3,), form="dev")
    return pctx


@pytest.mark.parametrize("word", WORDS)
def test_prove_sizes_on_the_default_context(warmed_pctx, rows130, word):
    _sequence(warmed_pctx, rows130, word)


@pytest.mark.parametrize("knobs", [{"BBP_ROTATE_BELOW": "0", "BBP_DUAL_OPEN_BELOW": "0"},  # B = 130 runs as two slices of 65
                                   {"BBP_RNG_COOP": "0"}],                                  # the serial draw chain
                         ids=["two_slices", "serial_draws"])
def test_prove_sizes_on_the_knob_contexts(bbp, ctx, rows8, rows130, knobs):
    c = pc.knob_context(bbp, knobs)
    try:
        _warm_prove(c, rows8, SIZES)
        for word in WORDS:
            _sequence(c, rows130, word)
    finally:
        c.close()


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("shape", ["N202_B2", "N8_B5"])
def test_prove_further_shapes(warmed_pctx, rows8, rows202, shape, form, word):
    """N = 202: no padded range; N = 8, B = 5; through the host-pointer call and through bbp_prove_batch_dev"""
    p = rows202 if shape == "N202_B2" else rows8
    with pc.Poisoned(warmed_pctx, word):
        if form == "host":
            out, st = warmed_pctx.prove_batch(*pc.prove_args(p, p.B))
            assert st == [OK] * p.B
        else:
            out = _prove_dev(warmed_pctx, pc.prove_args(p, p.B), p.rs)
    assert out == b"".join(p.records)


@pytest.mark.parametrize("word", WORDS)
def test_checked_proving_reproves_over_poison(bbp, ctx, rows8, word):
    """bbp_debug_corrupt_next_proof(1) at B = 5: the check refuses record 1 and the row is proved again, all of it over filled scratch"""
    c = bbp.Context(0)
    try:
        c.set_prove_check(True)
        _warm_prove(c, rows8, (6,))
        n0 = c.prove_check_stats()
        with pc.Poisoned(c, word):
            c.debug_corrupt_next_proof(1)
            out, st = c.prove_batch(*pc.prove_args(rows8, 5))
        n1 = c.prove_check_stats()
        assert st == [OK] * 5 and out == b"".join(rows8.records)
        assert (n1[0] - n0[0], n1[1] - n0[1], n1[2] - n0[2]) == (5, 0, 1)  # five rows checked, none refused, one proved again
    finally:
        c.close()


def test_pool_members_poisoned(bbp, ctx, oc, rows8):
    """Pool([0, 0]): 37 rows split 19 + 18 over two members, both filled before the call"""
    p = pc.proved_rows(oc, bbp, 37, 8, seed=37008)
    pool = bbp.Pool([0, 0])
    try:
        for _ in range(pc.WARM_CALLS):
            _, st = pool.prove_batch(*pc.tiled(rows8, 45))
            assert st == [OK] * 45
        for word in WORDS:
            before = [pc.allocations(pool.member(i)) for i in range(2)]
            for i in range(2):
                assert pool.member(i).debug_poison_scratch(word)[2] > 0
            out, st = pool.prove_batch(*pc.prove_args(p, 37))
            assert st == [OK] * 37 and out == b"".join(p.records), word
            assert [pc.allocations(pool.member(i)) for i in range(2)] == before
            assert pool.health() == 0
    finally:
        pool.close()


# ---- 3. verify ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vrounds(oc, proved):
    return pc.verify_rounds_of(oc, proved, NS)


def _verify_forms(c, vrounds, B):
    """name -> (plain call, aggregated call) of every verify form over B rows"""
    forms = {}
    picks = pc.verify_picks(B, len(NS))
    Ns = [NS[r] for r, _ in picks]
    mixed = b"".join(vrounds[r].full[v] for r, v in picks)
    forms["mixed"] = (lambda: c.verify_batch_mixed(Ns, mixed), lambda: c.verify_batch_mixed_aggregated(Ns, mixed, G))
    round_Ns, table, round_of, rows, want = vr._batch(vrounds, picks)
    assert want == pc.verify_want(B)
    forms["rounds"] = (lambda: c.verify_rounds(round_Ns, table, round_of, rows), lambda: c.verify_rounds_aggregated(round_Ns, table, round_of, rows, G))
    for k, n in enumerate(NS):
        blob = b"".join(vrounds[k].full[v] for _, v in pc.verify_picks(B, 1))
        forms["uniform%d" % n] = (lambda n=n, blob=blob: c.verify_batch(B, n, blob), lambda n=n, blob=blob: c.verify_batch_aggregated(B, n, blob, G))
    return forms


@pytest.fixture(scope="module")
def warmed_vctx(vctx, vrounds):
    """every form, plain and aggregated, at B = 140 and at the sizes under test, once per verifier lane and staging slot"""
    for B in (140, 130, 33):
        for plain, agg in _verify_forms(vctx, vrounds, B).values():
            for _ in range(pc.WARM_CALLS):
                assert plain() == pc.verify_want(B)
                assert agg()[0] == pc.verify_want(B)
    return vctx


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("B", [33, 130])
@pytest.mark.parametrize("form", ["uniform1", "uniform8", "uniform202", "mixed", "rounds"])
def test_verify_forms(warmed_vctx, vrounds, form, B, word):
    c = warmed_vctx
    plain, agg = _verify_forms(c, vrounds, B)[form]
    want = pc.verify_want(B)
    with pc.Poisoned(c, word):
        assert plain() == want
    with pc.Poisoned(c, word):
        st, nfb = agg()
    assert st == want
    assert nfb == pc.expected_fallback(B, want) == (B - 1) % G + 1


# ---- 4. the MSM hook ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def msm(built, oc, pctx):
    """the two launches, their rows and the oracle's points; the context warmed by a launch larger than both"""
    lib = ctypes.CDLL(built.build_hostcheck())
    layout, n, B = mc.SPLIT_SHAPE
    p = mc.plan(lib, B, n)
    assert mc.path(p) == (mc.SMALL, mc.PLAIN, mc.SMALL_FOLD) and p.split == 16
    split = [mc.row_bytes(s) for s in mc.split_rows(n, p.n_sub).values()]
    n1 = 1467
    assert mc.plan(lib, mc.UNSPLIT_B, n1).split == 1
    rows = dict(mc.filler_rows(n1))
    for b in mc.ADVERSARIAL_AT:
        rows[b] = mc.uniform_row(n1)
    unsplit = [mc.row_bytes(rows[b]) for b in range(mc.UNSPLIT_B)]
    distinct = list(dict.fromkeys(unsplit))
    pts = oc.msm_layout_many(distinct, [n1] * len(distinct), [mc.LAYOUT_G] * len(distinct), threads=16)
    point = {r: pts[32 * i:32 * i + 32] for i, r in enumerate(distinct)}
    want_split = oc.msm_layout_many(split, [n] * B, [layout] * B, threads=16)
    for _ in range(2):
        pctx.msm_batch(mc.UNSPLIT_B + 4, n, bytes(32 * n * (mc.UNSPLIT_B + 4)), layout)  # larger than both launches, on either path's scratch
        pctx.msm_batch(B + 1, n, bytes(32 * n * (B + 1)), layout)
    return {"split": (B, n, b"".join(split), layout, want_split), "unsplit": (mc.UNSPLIT_B, n1, b"".join(unsplit), mc.LAYOUT_G, b"".join(point[r] for r in unsplit))}


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("launch", ["split", "unsplit"])
def test_msm_hook(pctx, msm, launch, word):
    B, n, scalars, layout, want = msm[launch]
    got = _poisoned(pctx, word, lambda: pctx.msm_batch(B, n, scalars, layout))
    wrong = [b for b in range(B) if got[32 * b:32 * b + 32] != want[32 * b:32 * b + 32]]
    assert not wrong, wrong[:8]


# ---- 5. the other families ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", WORDS)
def test_witness_batch(pctx, oc, word):
    import random
    rnd = random.Random(11)
    rows = [bc.b32(rnd.getrandbits(64)) + bc.b32(rnd.randrange(pc.L)) + bc.b32(rnd.randrange(pc.L)) for _ in range(70)]
    pctx.witness_batch(b"".join(rows) + rows[0] * 30)
    out = _poisoned(pctx, word, lambda: pctx.witness_batch(b"".join(rows)))
    for i, r in enumerate(rows):
        assert out[192 * i:192 * i + 192] == oc.witness(r), i


@pytest.mark.parametrize("word", WORDS)
def test_prepare_bids_dev(pctx, rows8, word):
    import torch
    p, B, N = rows8, rows8.B, rows8.N
    bids = b"".join(r[:64] + r[192:224] for r in p.ins)           # d || k || seed
    lists = b"".join(r[224:224 + 32 * N] for r in p.ins)
    d_bids, d_lists = pc.dev(bids), pc.dev(lists)
    d_tog = torch.tensor([int.from_bytes(r[-8:], "little") for r in p.ins], dtype=torch.int64, device="cuda")
    d_in, d_tail = pc.filled(len(p.ins[0]) * B), pc.filled((96 + 32 * N) * B)
    torch.cuda.synchronize()

    def call():
        d_in.fill_(FILL), d_tail.fill_(FILL)
        torch.cuda.synchronize()
        pctx.prepare_bids_dev(B, N, d_bids.data_ptr(), d_lists.data_ptr(), d_tog.data_ptr(), d_in.data_ptr(), d_tail.data_ptr())
        torch.cuda.synchronize()
    _poisoned(pctx, word, call)
    assert pc.host(d_in) == b"".join(p.ins) and pc.host(d_tail) == b"".join(p.tails)


@pytest.fixture(scope="module")
def round35(oc, bbp):
    """N = 3, B = 5: five honest bids of one round and the oracle's rows for them"""
    return pc.OracleRound(oc, bbp, 3, 5, 5, 301, {})


@pytest.fixture(scope="module")
def rctx(ctx, bbp):
    """the context of the round calls (prove_round, the selection, the best-of-round calls and the standing)"""
    yield from _own_context(bbp)


def _prove_round_dev(c, bbp, r, ent):
    import torch
    N, B = r.N, r.B
    d_tab, d_bids, d_ent = pc.dev(r.table), pc.dev(r.bid_bytes), pc.dev(ent)
    d_rows, d_st, d_tog = pc.filled(bbp.round_row_size(N) * B), pc.filled(4 * B), pc.filled(8 * B)
    torch.cuda.synchronize()
    c.prove_round_dev(N, d_tab.data_ptr(), B, d_bids.data_ptr(), d_ent.data_ptr(), d_rows.data_ptr(), d_st.data_ptr(), d_tog.data_ptr())
    torch.cuda.synchronize()
    st, tog = pc.host(d_st), pc.host(d_tog)
    return pc.host(d_rows), [int.from_bytes(tog[8 * i:8 * i + 8], "little") for i in range(B)], [int.from_bytes(st[4 * i:4 * i + 4], "little") for i in range(B)]


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_prove_round(rctx, bbp, round35, form, word):
    o, r = round35, round35.round
    big = rc.honest(8, 9, 302)
    call = (lambda x, e: rctx.prove_round(x.N, x.table, x.bid_bytes, e)) if form == "host" else (lambda x, e: _prove_round_dev(rctx, bbp, x, e))
    for _ in range(pc.WARM_CALLS):
        assert call(big, rc.entropy(302, 9, 8))[2] == [OK] * 9
    rows, toggles, st = _poisoned(rctx, word, lambda: call(r, o.entropy))
    assert st == [OK] * 5 and toggles == r.toggles and rows == o.honest_rows


@pytest.fixture(scope="module")
def select_case(oc, bbp):
    """rc.status_round() (N = 8, B = 8, three refused bids), K = 3: the model's selection and the oracle's rows for the selected bids"""
    r = rc.status_round()
    scores = [e[2]["q"] if e[0] == OK else 0 for e in r.expect]
    sel, n_sel, n_q = sc.model(scores, r.status, 0, 3)
    sub, ent = rc.subset(r, sel), rc.entropy(303, 3, r.N)
    recs, st = oc.prove_many(sub.in_rows(), ent, 3, r.N, threads=16)
    assert st == [OK] * 3 and (n_sel, n_q) == (3, 5)
    return r, scores, sel, sub, ent, sub.rows(recs)


def _select_dev(c, r, K, cap):
    import torch
    B, N = r.B, r.N
    d_tab, d_bids = pc.dev(r.table), pc.dev(r.bid_bytes)
    o = dict(sel=pc.filled(4 * cap), counts=pc.filled(8), status=pc.filled(4 * B), scores=pc.filled(32 * B), prove_in=pc.filled((232 + 32 * N) * cap),
             tails=pc.filled(64 * cap), toggles=pc.filled(8 * cap))
    torch.cuda.synchronize()
    c.select_round_dev(N, d_tab.data_ptr(), B, d_bids.data_ptr(), 0, K, cap, o["sel"].data_ptr(), o["counts"].data_ptr(), o["status"].data_ptr(),
                       o["scores"].data_ptr(), o["prove_in"].data_ptr(), o["tails"].data_ptr(), o["toggles"].data_ptr())
    torch.cuda.synchronize()
    return {k: pc.host(v) for k, v in o.items()}


@pytest.mark.parametrize("word", WORDS)
def test_round_selection(rctx, select_case, word):
    """bbp_select_round_dev, bbp_prove_round_select and the selection kernel alone (bbp_debug_round_select)"""
    r, scores, sel, sub, ent, want_rows = select_case
    big = rc.honest(8, 20, 304)
    for _ in range(pc.WARM_CALLS):
        rctx.prove_round_select(8, big.table, big.bid_bytes, 0, 5, entropy=rc.entropy(304, 5, 8))
        _select_dev(rctx, big, 5, 5)
        rctx.debug_round_select(b"".join(sc.b32(s) for s in range(1, 41)), [OK] * 40, 0, 5)
    u32 = lambda b, n: [int.from_bytes(b[4 * i:4 * i + 4], "little", signed=True) for i in range(n)]  # noqa: E731
    h = _poisoned(rctx, word, lambda: _select_dev(rctx, r, 3, 3))
    assert u32(h["sel"], 3) == sel and u32(h["counts"], 2) == [3, 5] and u32(h["status"], r.B) == r.status
    assert h["scores"] == b"".join(rc.b32(s) for s in scores)
    assert h["prove_in"] == sub.in_rows() and h["tails"] == b"".join(sub.tail(j) for j in range(3))
    assert [int.from_bytes(h["toggles"][8 * j:8 * j + 8], "little") for j in range(3)] == sub.toggles
    got = _poisoned(rctx, word, lambda: rctx.prove_round_select(r.N, r.table, r.bid_bytes, 0, 3, entropy=ent, want_scores=True))
    assert (got.rc, got.sel, got.n_sel, got.n_qualified, got.toggles, got.status) == (OK, sel, 3, 5, sub.toggles, r.status)
    assert got.rows == want_rows and got.scores == b"".join(rc.b32(s) for s in scores)
    assert _poisoned(rctx, word, lambda: rctx.debug_round_select(b"".join(rc.b32(s) for s in scores), r.status, 0, 3)) == (sel, 3, 5)


@pytest.fixture(scope="module")
def best_case(oc, bbp):
    """N = 3, nine rows of three bids: row 1 claims the top score (forged, VERIFY: a second tranche runs), row 4 has a flipped byte, row 7
    a score >= l; every bidder turns up three times"""
    c = pc.OracleRound(oc, bbp, 3, 3, 9, 305, {1: "top", 4: "flip", 7: "score_l"})
    assert [c.verdicts[i] for i in (1, 4, 7)] == [VERIFY, VERIFY, FORMAT] and c.verdicts.count(OK) == 6
    return c


@pytest.fixture(scope="module")
def best_warm(oc, bbp):
    return pc.OracleRound(oc, bbp, 8, 2, 24, 306, {0: "top"})


def _check_best(got, want):
    best, n_best, n_cand, n_exam, status = want
    assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.status) == (best, n_best, n_cand, n_exam, status)


def _check_distinct(got, want):
    best, n_best, n_cand, n_exam, n_dup, status = want
    assert (got[0], got.n_best if hasattr(got, "n_best") else got.n_entered, got.n_candidates, got.n_examined, got.n_duplicates, got.status) == \
        (best, n_best, n_cand, n_exam, n_dup, status)


@pytest.mark.parametrize("word", WORDS)
def test_round_best_and_distinct(rctx, best_case, best_warm, word):
    c, w = best_case, best_warm
    kb, wkb = b"".join(bc.b32(k) for k in c.keys), b"".join(bc.b32(k) for k in w.keys)
    for _ in range(pc.WARM_CALLS):
        rctx.verify_round_best(w.N, w.table, w.rows, 0, 0, 1)
        rctx.verify_round_best_distinct(w.N, w.table, w.rows, 0, 0, 1)
        rctx.debug_round_best(wkb, w.verdicts, 0, 0, 1)
        rctx.debug_round_best_distinct(wkb, b"".join(w.ids), w.verdicts, 0, 0, 1)
    for K, tranche in ((1, 1), (2, 1), (0, 1)):
        want = bc.model(c.keys, c.verdicts, 0, K, tranche)
        assert K == 0 or want[3] > max(K, tranche)  # the forged top claim: more than the first tranche is examined
        _check_best(_poisoned(rctx, word, lambda: rctx.verify_round_best(c.N, c.table, c.rows, 0, K, tranche, fill=FILL)), want)
        _check_best(_poisoned(rctx, word, lambda: rctx.debug_round_best(kb, c.verdicts, 0, K, tranche, fill=FILL)), want)
        want = dc.model(c.keys, c.ids, c.verdicts, 0, K, tranche)
        _check_distinct(_poisoned(rctx, word, lambda: rctx.verify_round_best_distinct(c.N, c.table, c.rows, 0, K, tranche, fill=FILL)), want)
        _check_distinct(_poisoned(rctx, word, lambda: rctx.debug_round_best_distinct(kb, b"".join(c.ids), c.verdicts, 0, K, tranche, fill=FILL)), want)


@pytest.fixture(scope="module")
def rounds_case(oc, bbp):
    """two rounds, N = (202, 1), four rows each, interleaved; round 0's row 1 claims the top score (forged)"""
    a = pc.OracleRound(oc, bbp, 202, 2, 4, 307, {1: "top"})
    b = pc.OracleRound(oc, bbp, 1, 2, 4, 308, {2: "flip"})
    round_of = [i % 2 for i in range(8)]
    rows = [(a, b)[i % 2].row_list[i // 2] for i in range(8)]
    return dict(Ns=[202, 1], table=a.table + b.table, round_of=round_of, rows=b"".join(rows), keys=[(a, b)[i % 2].keys[i // 2] for i in range(8)],
                ids=[x[-32:] for x in rows], verdicts=[(a, b)[i % 2].verdicts[i // 2] for i in range(8)])


@pytest.mark.parametrize("word", WORDS)
def test_rounds_best_and_distinct(rctx, rounds_case, word):
    c = rounds_case
    kb, ib = b"".join(bc.b32(k) for k in c["keys"]), b"".join(c["ids"])
    big = dict(round_of=c["round_of"] * 3, rows=c["rows"] * 3)  # the same rows three times over: a larger call of the same rounds
    for _ in range(pc.WARM_CALLS):
        rctx.verify_rounds_best(c["Ns"], c["table"], big["round_of"], big["rows"], None, 0, 1)
        rctx.verify_rounds_best_distinct(c["Ns"], c["table"], big["round_of"], big["rows"], None, 0, 1)
        rctx.debug_rounds_best(2, big["round_of"], kb * 3, c["verdicts"] * 3, None, 0, 1)
        rctx.debug_rounds_best_distinct(2, big["round_of"], kb * 3, ib * 3, c["verdicts"] * 3, None, 0, 1)
    for K, tranche in ((1, 1), (0, 1)):
        want = mbc.model(2, c["round_of"], c["keys"], c["verdicts"], None, K, tranche)
        for call in (lambda: rctx.verify_rounds_best(c["Ns"], c["table"], c["round_of"], c["rows"], None, K, tranche, fill=FILL),
                     lambda: rctx.debug_rounds_best(2, c["round_of"], kb, c["verdicts"], None, K, tranche, fill=FILL)):
            got = _poisoned(rctx, word, call)
            assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.n_steps, got.status) == want
        want = mdc.model(2, c["round_of"], c["keys"], c["ids"], c["verdicts"], None, K, tranche)[:7]
        for call in (lambda: rctx.verify_rounds_best_distinct(c["Ns"], c["table"], c["round_of"], c["rows"], None, K, tranche, fill=FILL),
                     lambda: rctx.debug_rounds_best_distinct(2, c["round_of"], kb, ib, c["verdicts"], None, K, tranche, fill=FILL)):
            got = _poisoned(rctx, word, call)
            assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.n_duplicates, got.n_steps, got.status) == want


@pytest.mark.parametrize("word", WORDS)
def test_standing_offers(rctx, best_case, best_warm, word):
    """two offers to one open standing, the scratch filled between them: the standing's own entries are exempt and persist, the rows the
    second offer works on (best_dev, best.rows, the verifier lanes) are not"""
    c, w = best_case, best_warm
    hw = rctx.standing_open(w.N, w.table, 0, 2)
    for _ in range(pc.WARM_CALLS):
        rctx.standing_offer(hw, w.N, w.rows, 1)
    rctx.standing_close(hw)
    bursts = (slice(0, 2), slice(2, 9))
    for _ in range(pc.WARM_CALLS):  # ... and the offers under test themselves, to standings that are closed again
        hw = rctx.standing_open(c.N, c.table, 0, 2)
        for sl in bursts:
            rctx.standing_offer(hw, c.N, b"".join(c.row_list[sl]), 1)
            rctx.standing_read(hw)
        rctx.standing_close(hw)
    h = rctx.standing_open(c.N, c.table, 0, 2)
    model = stc.Standing(0, 2)
    try:
        for sl in bursts:
            with pc.Poisoned(rctx, word):
                got = rctx.standing_offer(h, c.N, b"".join(c.row_list[sl]), 1, fill=FILL)
            _check_distinct(got, model.offer(c.keys[sl], c.ids[sl], c.verdicts[sl], 1))
            with pc.Poisoned(rctx, word):
                read = rctx.standing_read(h)
            assert (read.n_entries, read.n_offered, read.serials) == (len(model.entries), model.offered, [s for _, _, s in model.entries])
            assert read.scores == [bc.b32(k) for k, _, _ in model.entries] and read.z_imgs == [i for _, i, _ in model.entries]
        assert [(k, i) for k, i, _ in model.entries] == [(k, i) for k, i, _ in stc.truth(c.keys, c.ids, c.verdicts, 0, 2)]
        # the second offer found row 0's entry, kept it, put row 2 above it and turned both bidders' later rows away as duplicates
        assert [s for _, _, s in model.entries] == [2, 0] and got.n_duplicates > 0
    finally:
        rctx.standing_close(h)


@pytest.mark.parametrize("word", WORDS)
def test_entropy_draws(pctx, bbp, rows8, word):
    """bbp_draw_entropy_dev (both kinds) against tests/entropy_ref.py, the hedged draw against tests/hedge_ref.py"""
    import torch
    B, N, es = rows8.B, rows8.N, bbp.entropy_size(rows8.N)
    d_in = pc.dev(b"".join(rows8.ins))
    d_prove, d_verify, d_hedged = pc.filled(B * es), pc.filled(B * 32), pc.filled(B * es)
    torch.cuda.synchronize()

    def call():
        for d in (d_prove, d_verify, d_hedged):
            d.fill_(FILL)
        torch.cuda.synchronize()
        pctx.draw_entropy_dev(B, N, bbp.ENTROPY_PROVE, d_prove.data_ptr(), key=KEY)
        pctx.draw_entropy_dev(B, N, bbp.ENTROPY_VERIFY, d_verify.data_ptr(), key=KEY)
        pctx.draw_entropy_hedged_dev(B, N, d_in.data_ptr(), d_hedged.data_ptr(), key=KEY)
        torch.cuda.synchronize()
    _poisoned(pctx, word, call)
    assert pc.host(d_prove) == er.expand_prove(KEY, N, B) and pc.host(d_verify) == er.expand_verify(KEY, B)
    assert pc.host(d_hedged) == hr.expand_prove(KEY, N, rows8.ins) and pc.host(d_in) == b"".join(rows8.ins)
