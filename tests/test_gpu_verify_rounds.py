"""Rounds on the device (include/bbp.h bbp_verify_rounds*): rows of record || score || z_img against a table of rounds, seed and
bid list sent once per round.  Every row's status is what bbp_verify_batch_mixed reports for the expanded row
record || score || z_img || seed_r || pub_list_r.

Anchors: the C oracle's verdict on every distinct expanded row (oracle/c, on the CPU) and the existing calls on the expanded rows
(expand_round_rows).  The proofs are a handful of distinct records per round, made by the engine under fixed entropy, tiled."""
import ctypes
import hashlib
import random

import pytest

from oracle.ref_py import ristretto as rs
from tests import forgery_cases as fc
from tests import oracle_c

pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG = 0, 1, 2, 3, 4
L = fc.L
# a flipped record byte (t_x), a wrong score, a wrong z_img, a non-canonical score / z_img, an undecodable point (A_I1), the version byte
KINDS = ("flip", "score", "zimg", "score_l", "zimg_l", "point", "parse")
ROUND_NS = (1, 3, 8, 8, 57, 202)  # round ids 0..5; 2 and 3 share N = 8 under different seeds and lists


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


def _h(tag, *ids):
    return hashlib.sha512(b"bbp-rounds-v1" + b"".join(i.to_bytes(8, "little") for i in ids) + tag).digest()


def _tamper(row, N, kind):
    rs_ = 1121 + 32 * (4 + N)
    b = bytearray(row)
    if kind == "flip":       # t_x: after the version byte, A_I1 A_O1 S1 and T_1 T_3..T_6
        b[257] ^= 0x01
    elif kind == "score":
        b[rs_] ^= 0x01
    elif kind == "zimg":
        b[rs_ + 32] ^= 0x01
    elif kind == "score_l":
        b[rs_:rs_ + 32] = (int.from_bytes(b[rs_:rs_ + 32], "little") + L).to_bytes(32, "little")
    elif kind == "zimg_l":
        b[rs_ + 32:rs_ + 64] = (int.from_bytes(b[rs_ + 32:rs_ + 64], "little") + L).to_bytes(32, "little")
    elif kind == "point":    # A_I1 = ff..ff: not a ristretto encoding
        b[1:33] = b"\xff" * 32
    elif kind == "parse":
        b[0] ^= 0x01
    return bytes(b)


class Round:
    """One round: seed, bid list, up to three valid short rows (bids at list positions 0..2) and one tampered copy of row 0 per kind,
    every one with the C oracle's verdict on its expanded row."""

    def __init__(self, ctx, oc, bbp, rid, N):
        self.N, self.rid = N, rid
        self.seed = rs.sc_bytes(rs.sc_wide(_h(b"seed", rid)))
        k_bids = min(N, 3)
        pub = [rs.sc_bytes(rs.sc_wide(_h(b"pub", rid, j))) for j in range(N)]
        wit = []
        for i in range(k_bids):
            d, k = _h(b"d", rid, i)[:8] + bytes(24), rs.sc_bytes(rs.sc_wide(_h(b"k", rid, i)))
            w = oc.witness(d + k + self.seed)
            m, x, y, yi, q, z = [w[32 * j:32 * j + 32] for j in range(6)]
            pub[i] = x
            wit.append((d, k, y, yi, q, z))
        self.pub = b"".join(pub)
        ins = b"".join(d + k + y + yi + q + z + self.seed + self.pub + i.to_bytes(8, "little") for i, (d, k, y, yi, q, z) in enumerate(wit))
        ents = b"".join(b"".join(rs.sc_bytes(rs.sc_wide(_h(b"ent", rid, i, j))) for j in range(4 + N)) + _h(b"es", rid, i)[:32]
                        for i in range(k_bids))
        out, st = ctx.prove_batch(k_bids, N, ins, ents)
        assert st == [OK] * k_bids
        rsz = bbp.record_size(N)
        self.good = [out[i * rsz:(i + 1) * rsz] + wit[i][4] + wit[i][5] for i in range(k_bids)]
        self.bad = [_tamper(self.good[0], N, kind) for kind in KINDS]
        self.variants = self.good + self.bad
        assert all(len(v) == bbp.round_row_size(N) for v in self.variants)
        blob = b"".join(v + self.seed + self.pub for v in self.variants)
        self.verdict = oc.verify_many(blob, len(self.variants), N, threads=8)
        assert self.verdict[:k_bids] == [OK] * k_bids
        assert self.verdict[k_bids:] == [VERIFY, VERIFY, VERIFY, FORMAT, FORMAT, VERIFY, FORMAT]

    def table(self):
        return self.seed + self.pub

    def five(self, i=0):
        """valid row i as the (record, score, z_img, seed, pub_list) tuple of tests/forgery_cases.py"""
        rsz = len(self.good[i]) - 64
        g = self.good[i]
        return (g[:rsz], g[rsz:rsz + 32], g[rsz + 32:], self.seed, self.pub)


@pytest.fixture(scope="module")
def rounds(ctx, oc, bbp):
    return [Round(ctx, oc, bbp, rid, n) for rid, n in enumerate(ROUND_NS)]


def _batch(rnds, picks):
    """picks: [(index into rnds, variant index)] -> (round_Ns, table, round_of, rows, oracle verdicts)"""
    round_Ns = [r.N for r in rnds]
    table = b"".join(r.table() for r in rnds)
    round_of = [ri for ri, _ in picks]
    rows = b"".join(rnds[ri].variants[vi] for ri, vi in picks)
    return round_Ns, table, round_of, rows, [rnds[ri].verdict[vi] for ri, vi in picks]


def _interleaved(rnds, B, skip=(), seed=5):
    """B picks that walk over the rounds (those in `skip` get no row) and over each round's variants, shuffled"""
    live = [i for i in range(len(rnds)) if i not in skip]
    picks = [(live[j % len(live)], (j // len(live)) % len(rnds[live[j % len(live)]].variants)) for j in range(B)]
    random.Random(seed).shuffle(picks)
    return picks


def _put(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


# ---- 1. one round -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 65, 130])
@pytest.mark.parametrize("rid", [0, 1, 2, 5])  # N = 1, 3, 8, 202
def test_one_round(ctx, bbp, rounds, rid, B):
    r = rounds[rid]
    picks = [(0, j % len(r.variants)) for j in range(B)]
    round_Ns, table, _, rows, oracle = _batch([r], picks)
    st = ctx.verify_rounds(round_Ns, table, None, rows)
    print("one round N=%d B=%d:" % (r.N, B), st)
    assert st == oracle
    Ns, blob = bbp.expand_round_rows(round_Ns, table, None, rows)
    assert Ns == [r.N] * B
    assert st == ctx.verify_batch(B, r.N, blob)
    assert st == ctx.verify_round(r.N, r.seed, r.pub, rows)
    assert st == ctx.verify_rounds(round_Ns, table, [0] * B, rows)  # round_of given all the same


# ---- 2. several rounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", [3, 0])  # the round no row names: N = 57 in the middle of the table, N = 1 at its head
def test_several_rounds(ctx, bbp, rounds, empty):
    rnds = [rounds[i] for i in (0, 2, 3, 4, 5)]  # N = (1, 8, 8, 57, 202)
    assert [r.N for r in rnds] == [1, 8, 8, 57, 202] and rnds[1].table() != rnds[2].table()
    picks = _interleaved(rnds, 70, skip=(empty,))
    round_Ns, table, round_of, rows, oracle = _batch(rnds, picks)
    assert empty not in round_of and len(set(round_of)) == 4
    st = ctx.verify_rounds(round_Ns, table, round_of, rows)
    print("several rounds, empty %d:" % empty, st)
    assert st == oracle
    Ns, blob = bbp.expand_round_rows(round_Ns, table, round_of, rows)
    assert st == ctx.verify_batch_mixed(Ns, blob)
    # rows that name round 1 verified against round 2's table entry (same N = 8) must fail: indexing by N would not notice
    swapped = [2 if r == 1 else 1 if r == 2 else r for r in round_of]
    st2 = ctx.verify_rounds(round_Ns, table, swapped, rows)
    for i, r in enumerate(round_of):
        assert st2[i] == (st[i] if r not in (1, 2) else (FORMAT if st[i] == FORMAT else VERIFY)), i


# ---- 3. isolation -----------------------------------------------------------------------------------------------------------
def test_isolation(ctx, bbp, rounds):
    rnds = [rounds[i] for i in (1, 2, 3, 4)]  # N = 3, 8, 8, 57
    picks = [(j % 4, (j // 4) % len(rnds[j % 4].good)) for j in range(24)]  # valid rows only
    round_Ns, table, round_of, rows, oracle = _batch(rnds, picks)
    assert oracle == [OK] * 24
    assert ctx.verify_rounds(round_Ns, table, round_of, rows) == oracle
    toff = bbp.round_table_offsets(round_Ns)

    def with_scalar(at, fn):
        v = int.from_bytes(table[at:at + 32], "little")
        return table[:at] + fn(v).to_bytes(32, "little") + table[at + 32:]

    for r in range(4):
        n = round_Ns[r]
        # one list item flipped (the last: a stride mistake would read past it into the next round)
        t = with_scalar(toff[r] + 32 * n, lambda v: v ^ 1)
        st = ctx.verify_rounds(round_Ns, t, round_of, rows)
        assert st == [VERIFY if ro == r else OK for ro in round_of], r
        assert st == ctx.verify_batch_mixed(*bbp.expand_round_rows(round_Ns, t, round_of, rows))
        # a non-canonical seed: seed + l
        t = with_scalar(toff[r], lambda v: v + L)
        st = ctx.verify_rounds(round_Ns, t, round_of, rows)
        assert st == [FORMAT if ro == r else OK for ro in round_of], r
        assert st == ctx.verify_batch_mixed(*bbp.expand_round_rows(round_Ns, t, round_of, rows))
        assert ctx.verify_rounds_aggregated(round_Ns, t, round_of, rows, 7)[0] == st
        # Scalar::from_bits: bit 255 set, and item + l, are the same item
        for at in (toff[r] + 32, toff[r] + 32 * n):
            for fn in (lambda v: v | 1 << 255, lambda v: v + L):
                t = with_scalar(at, fn)
                assert t != table
                assert ctx.verify_rounds(round_Ns, t, round_of, rows) == oracle, (r, at)


# ---- 4. above 4096 rows: the other variable-base path ---------------------------------------------------------------------------
def test_above_4096_rows(ctx, bbp, rounds):
    rnds = [rounds[2], rounds[3]]  # N = 8 twice
    B = 4100
    bad = {0: 3, 63: 4, 64: 6, 2049: 7, 4095: 8, 4096: 9, 4099: 5}  # row -> variant (3.. are the tampered ones)
    picks = [(i % 2, bad.get(i, (i // 2) % 3)) for i in range(B)]
    round_Ns, table, round_of, rows, oracle = _batch(rnds, picks)
    st = ctx.verify_rounds(round_Ns, table, round_of, rows)
    assert [i for i, s in enumerate(st) if s != OK] == sorted(bad)
    assert st == oracle
    assert st == ctx.verify_batch_mixed(*bbp.expand_round_rows(round_Ns, table, round_of, rows))
    assert ctx.verify_rounds_aggregated(round_Ns, table, round_of, rows)[0] == oracle


# ---- 5. aggregated ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agg_case(bbp, rounds):
    """70 interleaved rows over five rounds, with one cancelling triple (a shifted by d, d, -2d) inside the N = 57 round"""
    rnds = [rounds[i] for i in (0, 2, 3, 4, 5)]
    picks = _interleaved(rnds, 70, skip=(), seed=11)
    round_Ns, table, round_of, rows, oracle = _batch(rnds, picks)
    off = [0]
    for r in round_of:
        off.append(off[-1] + bbp.round_row_size(round_Ns[r]))
    triple = fc.cancelling_sets(rnds[3].five(0), random.Random(3), which=("triple",))["a:triple"]
    parts = [rows[off[i]:off[i + 1]] for i in range(70)]
    where = [i for i, r in enumerate(round_of) if r == 3][:3]
    for i, row5 in zip(where, triple):
        parts[i] = row5[fc.REC] + row5[fc.SCORE] + row5[fc.Z_IMG]
        oracle[i] = VERIFY
    return round_Ns, table, round_of, b"".join(parts), oracle, where


@pytest.mark.parametrize("G", [1, 2, 7, 32])
def test_aggregated(ctx, bbp, agg_case, G):
    import torch
    round_Ns, table, round_of, rows, oracle, where = agg_case
    B = len(round_of)
    Ns, blob = bbp.expand_round_rows(round_Ns, table, round_of, rows)
    key = hashlib.sha256(b"rounds-agg-key%d" % G).digest()
    try:
        for source in ("os", "device"):
            ctx.set_entropy_source(source)
            if source == "device":
                ctx.debug_next_entropy_key(key)
            st, nfb = ctx.verify_rounds_aggregated(round_Ns, table, round_of, rows, G)
            if source == "device":
                ctx.debug_next_entropy_key(key)
            mst, mnfb = ctx.verify_batch_mixed_aggregated(Ns, blob, G)
            print("aggregated G=%d %s: n_fallback %d (mixed %d)" % (G, source, nfb, mnfb))
            assert st == oracle and mst == oracle
            assert nfb == mnfb
            assert [st[i] for i in where] == [VERIFY] * 3  # the cancelling set: member by member
    finally:
        ctx.set_entropy_source("os")
    d_tab, d_rows, d_blob = _put(table), _put(rows), _put(blob)
    d_ent = _put(b"".join(hashlib.sha256(b"rounds-ent%d" % i).digest() for i in range(B)))
    a = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    b = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nfb = ctx.verify_rounds_aggregated_dev(round_Ns, d_tab.data_ptr(), round_of, B, d_rows.data_ptr(), d_ent.data_ptr(), a.data_ptr(), group=G)
    mnfb = ctx.verify_batch_mixed_aggregated_dev(Ns, d_blob.data_ptr(), d_ent.data_ptr(), b.data_ptr(), group=G)
    torch.cuda.synchronize()
    assert a.cpu().tolist() == oracle and b.cpu().tolist() == oracle
    assert nfb == mnfb


def test_aggregated_one_round(ctx, bbp, rounds):
    """R = 1 behind the uniform front end: statuses and n_fallback of verify_batch_aggregated on the expanded rows"""
    import torch
    r = rounds[2]
    B = 67
    picks = [(0, j % len(r.variants)) for j in range(B)]
    round_Ns, table, _, rows, oracle = _batch([r], picks)
    Ns, blob = bbp.expand_round_rows(round_Ns, table, None, rows)
    d_tab, d_rows, d_blob = _put(table), _put(rows), _put(blob)
    d_ent = _put(b"".join(hashlib.sha256(b"rounds-ent1-%d" % i).digest() for i in range(B)))
    for G in (2, 32):
        st, _ = ctx.verify_rounds_aggregated(round_Ns, table, None, rows, G)
        assert st == oracle
        a = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        b = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nfb = ctx.verify_rounds_aggregated_dev(round_Ns, d_tab.data_ptr(), None, B, d_rows.data_ptr(), d_ent.data_ptr(), a.data_ptr(), group=G)
        unfb = ctx.verify_batch_aggregated_dev(B, r.N, d_blob.data_ptr(), d_ent.data_ptr(), b.data_ptr(), group=G)
        torch.cuda.synchronize()
        assert a.cpu().tolist() == oracle and b.cpu().tolist() == oracle and nfb == unfb


# ---- 6. staging reuse in the _dev forms -----------------------------------------------------------------------------------------
def test_dev_calls_queued_on_one_lane(ctx, bbp, rounds):
    import torch
    rA = [rounds[i] for i in (0, 2, 3, 4, 5)]
    rB = [rounds[i] for i in (3, 1, 2)]  # another table, other offsets, the N = 8 rounds the other way round
    cA = _batch(rA, _interleaved(rA, 70, seed=21))
    cB = _batch(rB, _interleaved(rB, 33, seed=22))
    cC = _batch([rounds[1]], [(0, j % len(rounds[1].variants)) for j in range(9)])  # one round, round_of NULL
    dev = []
    for round_Ns, table, round_of, rows, oracle in (cA, cB, cC):
        B = len(oracle)
        dev.append((_put(table), _put(rows), torch.randint(0, 256, (32 * B,), dtype=torch.uint8, device="cuda"),
                    torch.full((B,), -7, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    s = ctx.verify_stream(1)
    for k, (round_Ns, table, round_of, rows, oracle) in enumerate((cA, cB, cC)):
        t, r, e, st = dev[k]
        ctx.verify_rounds_dev(round_Ns, t.data_ptr(), round_of if k < 2 else None, len(oracle), r.data_ptr(), e.data_ptr(), st.data_ptr(), stream=s)
    extra = torch.full((len(cA[4]),), -7, dtype=torch.int32, device="cuda")
    assert ctx.verify_rounds_aggregated_dev(cA[0], dev[0][0].data_ptr(), cA[2], len(cA[4]), dev[0][1].data_ptr(), dev[0][2].data_ptr(),
                                            extra.data_ptr(), group=7, stream=s, want_count=False) is None
    torch.cuda.synchronize()
    for k, c in enumerate((cA, cB, cC)):
        assert dev[k][3].cpu().tolist() == c[4], k
    assert extra.cpu().tolist() == cA[4]
    # BBP_STREAM_CONTEXT and a caller's stream
    st = torch.full((len(cB[4]),), -7, dtype=torch.int32, device="cuda")
    ctx.verify_rounds_dev(cB[0], dev[1][0].data_ptr(), cB[2], len(cB[4]), dev[1][1].data_ptr(), dev[1][2].data_ptr(), st.data_ptr())
    cs = torch.cuda.Stream()
    st2 = torch.full((len(cB[4]),), -7, dtype=torch.int32, device="cuda")
    cs.wait_stream(torch.cuda.current_stream())
    ctx.verify_rounds_dev(cB[0], dev[1][0].data_ptr(), cB[2], len(cB[4]), dev[1][1].data_ptr(), dev[1][2].data_ptr(), st2.data_ptr(),
                          stream=cs.cuda_stream)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == cB[4] and st2.cpu().tolist() == cB[4]


# ---- 7. screening -----------------------------------------------------------------------------------------------------------
def test_screening(ctx, bbp, rounds):
    import torch
    rnds = [rounds[1], rounds[2]]
    round_Ns, table, round_of, rows, oracle = _batch(rnds, [(0, 0), (1, 0), (0, 1), (1, 1)])
    B, R = 4, 2
    u32 = ctypes.c_uint32
    tab = (ctypes.c_uint8 * len(table)).from_buffer_copy(table)
    rws = (ctypes.c_uint8 * len(rows)).from_buffer_copy(rows)
    d_tab, d_rows = _put(table), _put(rows)
    d_ent = torch.zeros(32 * B, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B,), 55, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib, h = bbp.lib, ctx._h

    def call(R_, ns, of, B_=B, tab_=tab, rws_=rws, with_status=True, expect=BAD_ARG):
        """all four forms; status and *n_fallback must stay as they were"""
        ns_a = None if ns is None else (u32 * len(ns))(*ns)
        of_a = None if of is None else (u32 * len(of))(*of)
        st = (ctypes.c_int32 * B)(*([55] * B))
        nfb = u32(9)
        stp = st if with_status else None
        assert lib.bbp_verify_rounds(h, R_, ns_a, tab_, B_, of_a, rws_, stp) == expect
        assert lib.bbp_verify_rounds_aggregated(h, R_, ns_a, tab_, B_, of_a, rws_, stp, 0, ctypes.byref(nfb)) == expect
        assert list(st) == [55] * B and nfb.value == 0
        dt, dr = (d_tab.data_ptr() if tab_ is not None else None), (d_rows.data_ptr() if rws_ is not None else None)
        ds = d_st.data_ptr() if with_status else None
        nfb = u32(9)
        assert lib.bbp_verify_rounds_dev(h, R_, ns_a, dt, B_, of_a, dr, d_ent.data_ptr(), ds, None) == expect
        assert lib.bbp_verify_rounds_aggregated_dev(h, R_, ns_a, dt, B_, of_a, dr, d_ent.data_ptr(), ds, 0, ctypes.byref(nfb), None) == expect
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [55] * B and nfb.value == 0

    # 1. a NULL among the required pointers, whatever else is wrong (here: B == 0 and R == 0 as well)
    call(R, None, round_of)
    call(R, round_Ns, round_of, tab_=None)
    call(R, round_Ns, round_of, rws_=None)
    call(R, round_Ns, round_of, with_status=False)
    call(0, None, round_of, B_=0)
    assert lib.bbp_verify_rounds_dev(h, R, (u32 * 2)(*round_Ns), d_tab.data_ptr(), B, (u32 * 4)(*round_of), d_rows.data_ptr(), None,
                                     d_st.data_ptr(), None) == BAD_ARG
    # 2. B == 0 is OK before R, round_Ns and round_of are looked at
    call(0, [0, 999], [7], B_=0, expect=OK)
    # 3. R == 0
    call(0, round_Ns, round_of)
    # 4. a 0 anywhere in round_Ns decides before an entry above the maximum, and before round_of
    call(3, [203, 8, 0], [5, 5, 5, 5])
    # 5. an entry above BBP_MAX_ITEMS, also in a round that no row names, and before round_of
    call(3, [3, 8, 203], round_of, expect=GENS_LEN)
    call(3, [3, 8, 203], [0, 1, 3, 0], expect=GENS_LEN)
    # 6. round_of out of range; NULL with more than one round
    call(R, round_Ns, [0, 1, 2, 1])
    call(R, round_Ns, None)
    # and the same arguments go through untouched
    st = (ctypes.c_int32 * B)(*([55] * B))
    assert lib.bbp_verify_rounds(h, R, (u32 * 2)(*round_Ns), tab, B, (u32 * 4)(*round_of), rws, st) == OK
    assert list(st) == oracle
    assert lib.bbp_round_row_size(8) == bbp.record_size(8) + 64


# ---- 8. pool ----------------------------------------------------------------------------------------------------------------
def test_pool(ctx, bbp, rounds, agg_case):
    round_Ns, table, round_of, rows, oracle, _ = agg_case
    p = bbp.Pool([0, 0])
    try:
        assert p.verify_rounds(round_Ns, table, round_of, rows) == oracle
        st, nfb = p.verify_rounds_aggregated(round_Ns, table, round_of, rows, 7)
        assert st == oracle and nfb > 0
        r = rounds[2]
        one = _batch([r], [(0, j % len(r.variants)) for j in range(21)])
        assert p.verify_rounds(one[0], one[1], None, one[3]) == one[4]  # round_of NULL: both members' blocks are of round 0
        assert p.verify_round(r.N, r.seed, r.pub, one[3]) == one[4]
        for dev_call in (lambda: p.verify_rounds_dev(round_Ns, 1, round_of, len(round_of), 1, 1, 1),
                         lambda: p.verify_rounds_aggregated_dev(round_Ns, 1, round_of, len(round_of), 1, 1, 1)):
            with pytest.raises(bbp.BbpError) as e:
                dev_call()
            assert e.value.status == BAD_ARG
        assert p.health() == 0
    finally:
        p.close()


# ---- 9. host chunking -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 1])
def test_host_chunks_cut_inside_a_round(ctx, bbp, rounds, agg_case, monkeypatch, chunk):
    """BBP_HOST_CHUNK_VERIFY is read at every call.  70 rows in chunks of 14 (70 / ceil(70 / 16)): sorted by round, the rounds' runs of
    14, 14, 14, 14, 14 rows are shifted by one so that every chunk edge falls inside a run; chunks of one row as the extreme."""
    round_Ns, table, round_of, rows, oracle, _ = agg_case
    off = [0]
    for r in round_of:
        off.append(off[-1] + bbp.round_row_size(round_Ns[r]))
    order = sorted(range(70), key=lambda i: round_of[i])
    order = order[-1:] + order[:-1]
    s_of = [round_of[i] for i in order]
    s_rows = b"".join(rows[off[i]:off[i + 1]] for i in order)
    s_oracle = [oracle[i] for i in order]
    assert any(s_of[e - 1] == s_of[e] for e in range(14, 70, 14))
    monkeypatch.setenv("BBP_HOST_CHUNK_VERIFY", str(chunk))
    assert ctx.verify_rounds(round_Ns, table, s_of, s_rows) == s_oracle
    st, nfb = ctx.verify_rounds_aggregated(round_Ns, table, s_of, s_rows, 4)
    assert st == s_oracle
    one = rounds[1]
    c = _batch([one], [(0, j % len(one.variants)) for j in range(37)])
    assert ctx.verify_rounds(c[0], c[1], None, c[3]) == c[4]
    monkeypatch.delenv("BBP_HOST_CHUNK_VERIFY")
    assert ctx.verify_rounds(round_Ns, table, s_of, s_rows) == s_oracle
