"""GPU tier: a standing of a round (include/bbp.h bbp_standing_open, bbp_standing_offer, bbp_standing_read, bbp_standing_close,
bbp_debug_standing_offer).  Hook-backed tests hold the shipped kernels -- the family's keys, ids, selection, mark, settle and holders, and
round_standing.h's seed, displace, merge, leave and commit -- to the model of tests/round_standing_cases.py on made-up keys, ids and
verdicts, and bbp_standing_read to truth(); proof-backed tests hold the host form to the model applied to the statuses that
bbp_verify_rounds returns for all rows.  A call that ends BBP_ERR_INTERNAL (the flag word was raised) raises BbpError and fails its test."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc
from tests import round_standing_cases as sc

dc, bc = sc.dc, sc.bc
pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, INTERNAL, SKIPPED, DUPLICATE = 0, 1, 2, 3, 4, 6, -1, -2
L = sc.L
FILL = 0x6E
FILL_U32 = int.from_bytes(bytes([FILL]) * 4, "little")
T_X = 257  # byte offset of t_x in a record: the version byte, then eight points
TABLE8 = bytes(32 * 9)  # a round of N = 8 for standings that only the hook is offered to (nothing is verified)


@pytest.fixture(scope="module")
def sctx(ctx, bbp):
    """A context of this module's own (after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _check(got, want, cap, what):
    entered, n_entered, n_cand, n_exam, n_dup, status = want
    assert (got.entered, got.n_entered, got.n_candidates, got.n_examined, got.n_duplicates) == (entered[:cap], n_entered, n_cand, n_exam, n_dup), what
    assert got.status == status, what
    assert got.raw[min(n_entered, cap):] == [FILL_U32] * (cap - min(n_entered, cap)), what  # entries at or beyond min(n_entered, cap) are not written
    assert n_exam + n_dup <= n_cand, what


def _check_read(c, h, entries, offered, what):
    got = c.standing_read(h)
    assert (got.n_entries, got.n_offered) == (len(entries), offered), what
    assert list(zip(got.scores, got.z_imgs, got.serials)) == [(bc.b32(k), i, s) for k, i, s in entries], what


class Hooked:
    """a standing offered to through the hook, and the model beside it; every offer and the state after it are checked"""

    def __init__(self, c, floor, K):
        self.c, self.floor, self.K = c, floor, K
        self.h = c.standing_open(8, TABLE8, floor, K)
        self.model = sc.Standing(floor, K)
        self.keys, self.ids, self.verdicts = [], [], []

    def offer(self, keys, ids, verdicts, tranche, cap=None, what=None):
        cap = len(keys) if cap is None else cap
        got = self.c.debug_standing_offer(self.h, b"".join(bc.b32(k) for k in keys), b"".join(ids), verdicts, tranche, cap=cap, fill=FILL)
        want = self.model.offer(keys, ids, verdicts, tranche)
        _check(got, want, cap, what)
        self.keys += keys
        self.ids += ids
        self.verdicts += verdicts
        assert self.model.entries == sc.truth(self.keys, self.ids, self.verdicts, self.floor, self.K), what
        _check_read(self.c, self.h, self.model.entries, len(self.keys), what)
        return got

    def close(self):
        self.c.standing_close(self.h)


# ---- hook-backed ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 130, 1000])
def test_hook_sweep_against_the_model(sctx, B):
    n_cases = n_small_cap = n_dups = 0
    for p, n_ids in enumerate(dc.id_pools(B)):
        keys = (bc.keys_uniform, bc.keys_low_byte)[p % 2](B, 17 * B + p)  # the low-byte keys: ties, the serial orders them
        ids = dc.id_pool(B, n_ids, 19 * B + p)
        for vname, verdicts in (("ok", [OK] * B), ("third", bc.verdicts_top_third_bad(keys))):
            for K in (1, 3, 64, 65):
                for tranche in (1, 4, 0):
                    what = (B, n_ids, vname, K, tranche)
                    one = Hooked(sctx, 0, K)  # (a) one burst to a fresh standing: the one-shot call's answer
                    want = dc.model(keys, ids, verdicts, 0, K, tranche)
                    small = tranche == 4 and want[1] > 2
                    got = one.offer(keys, ids, verdicts, tranche, cap=2 if small else B, what=what)
                    assert (got.n_entered, got.n_candidates, got.n_examined, got.n_duplicates, got.status) == want[1:], what
                    assert got.entered == want[0][:2 if small else B], what
                    one.close()
                    n_small_cap += small
                    three = Hooked(sctx, 0, K)  # (b) three bursts, an offer of nothing between the first two
                    for sl in (slice(0, B // 3), slice(0, 0), slice(B // 3, 2 * B // 3), slice(2 * B // 3, B)):
                        r = three.offer(keys[sl], ids[sl], verdicts[sl], tranche, what=what + (sl,))
                        n_dups += r.n_duplicates > 0
                    assert three.model.entries == one.model.entries, what  # whatever the cuts
                    three.close()
                    n_cases += 1
    assert n_cases == 4 * 2 * 4 * 3 and (B < 63 or (n_small_cap > 0 and n_dups > 0))


def _ids(n, seed=1):
    return dc.id_pool(n, n, seed)


def test_hook_improvement_lower_copy_equal_key_eviction(sctx):
    a, b, c, d, e = _ids(5)
    st = Hooked(sctx, 0, 3)
    st.offer([90, 70, 50], [a, b, c], [OK] * 3, 1)
    # improvement: the identity held at rank 2 comes back with a later, higher key -- replaced, the size unchanged, the ranks re-ordered
    got = st.offer([80], [c], [OK], 1)
    assert got.entered == [0] and st.model.entries == [(90, a, 0), (80, c, 3), (70, b, 1)]
    # a lower-key copy of a held identity above the bar is a DUPLICATE; an equal key at a later serial loses: SKIPPED, the standing is full
    got = st.offer([75, 70, 70], [a, b, e], [OK] * 3, 1)
    assert got.status == [DUPLICATE, SKIPPED, SKIPPED] and got.n_examined == 0
    # eviction: a better row pushes the last entry out; it is forgotten, and its resend is SKIPPED
    got = st.offer([100], [d], [OK], 1)
    assert got.entered == [0] and [i for _, i, _ in st.model.entries] == [d, a, c]
    got = st.offer([70, 70], [b, b], [OK] * 2, 1)
    assert got.status == [SKIPPED] * 2 and got.n_candidates == 0
    st.close()
    # not full: an equal key at a later serial of a held identity is a DUPLICATE
    st = Hooked(sctx, 0, 3)
    st.offer([90], [a], [OK], 1)
    got = st.offer([90, 90], [a, b], [OK] * 2, 1)
    assert got.status == [DUPLICATE, OK] and st.model.entries == [(90, a, 0), (90, b, 2)]
    # a forged higher score on a held identity: examined, fails, changes nothing -- each time it is sent
    for _ in range(2):
        got = st.offer([L - 1], [a], [VERIFY], 1)
        assert got.status == [VERIFY] and got.n_examined == 1 and got.n_entered == 0
    st.close()


def test_hook_one_identity_on_both_sides_of_a_workgroup_boundary(sctx):
    """rows 63 and 64 of an offer share an identity: the last lane of one 64-lane workgroup and the first of the next, in the key kernels
    and -- with K = 130, one tranche -- in settle and holders"""
    B = 130
    for k63, k64, holder in ((2000, 3000, 64), (3000, 2000, 63), (2500, 2500, 63)):
        keys = [1000 + i for i in range(B)]
        keys[63], keys[64] = k63, k64
        ids = _ids(B, 3)
        ids[64] = ids[63]
        for K in (130, 3):
            st = Hooked(sctx, 0, K)
            got = st.offer(keys, ids, [OK] * B, 0, what=(k63, k64, K))
            assert holder in got.entered and (127 - holder) not in got.entered
            st.close()


def test_hook_K_1024(sctx):
    # B = 1000 < K: the standing is never full, every valid identity is held
    B = 1000
    keys = bc.keys_uniform(B, 31)
    ids = dc.id_pool(B, 700, 32)
    verdicts = bc.verdicts_top_third_bad(keys)
    st = Hooked(sctx, 0, 1024)
    st.offer(keys, ids, verdicts, 0)
    assert len(st.model.entries) == len({i for i, v in zip(ids, verdicts) if v == OK}) < 1024
    st.close()
    # 3 x 1000 rows of their own identities: the standing fills in the third burst -- the merge at its widest
    st = Hooked(sctx, 0, 1024)
    for n in range(3):
        keys = bc.keys_uniform(B, 40 + n)
        got = st.offer(keys, _ids(B, 50 + n), [OK if i % 2 else VERIFY for i in range(B)], 0, what=n)  # 500 valid rows a burst
        assert (len(st.model.entries) == 1024) == (n == 2)
    assert got.n_entered < got.n_examined  # some of the last burst fell out again
    st.close()


def test_hook_contention(sctx):
    """65 536 rows of 202 identities, all OK, K = 3, to a standing that already holds three of those identities.  The outputs are the
    model's; the call returns BBP_OK, so the flag word of the bounded loops stayed clear."""
    B = 65536
    keys = bc.keys_uniform(B, 8)
    ids = dc.id_pool(B, 202, 9)
    st = Hooked(sctx, 0, 3)
    mid = sorted(keys)[B // 2]
    st.offer([mid, mid + 1, mid + 2], [ids[0], ids[1], ids[2]], [OK] * 3, 0)
    got = st.offer(keys, ids, [OK] * B, 0, cap=3)
    assert got.n_entered == 3 and got.n_examined >= 3
    st.close()


def test_hook_two_standings_do_not_disturb_each_other(sctx):
    B = 200
    a, b = Hooked(sctx, 0, 5), Hooked(sctx, 7, 64)
    for n in range(4):
        for st, seed in ((a, 100 + n), (b, 200 + n)):
            keys = bc.keys_low_byte(B, seed)
            st.offer(keys, dc.id_pool(B, 40, seed), bc.verdicts_top_third_bad(keys), 1, what=(n, seed))
            # another best call of the context between two offers: it uses the scratch the offers work in
            keys = bc.keys_uniform(300, seed)
            sctx.debug_round_best_distinct(b"".join(bc.b32(k) for k in keys), b"".join(dc.id_pool(300, 9, seed)), [OK] * 300, 0, 3, 1)
    for st in (a, b):
        _check_read(sctx, st.h, sc.truth(st.keys, st.ids, st.verdicts, st.floor, st.K), 4 * B, "at the end")
        st.close()


def test_hook_failed_offer_leaves_the_standing_as_it_was(sctx, bbp):
    st = Hooked(sctx, 0, 3)
    st.offer([50, 40], _ids(2, 5), [OK, OK], 1)
    before = sctx.standing_read(st.h)
    keys = [100 - n for n in range(40)]
    ids = _ids(40, 6)
    verdicts = [OK, VERIFY, VERIFY] + [OK] * 37  # tranche 0 (three rows) merges one row; tranche 1 would merge more
    sctx.debug_standing_trip(st.h, 2)  # the flag word is raised behind the second merge: no device fault is involved
    with pytest.raises(bbp.BbpError) as e:
        sctx.debug_standing_offer(st.h, b"".join(bc.b32(k) for k in keys), b"".join(ids), verdicts, 1)
    assert e.value.status == INTERNAL
    assert sctx.standing_read(st.h) == before and before.n_offered == 2 and before.n_entries == 2
    got = st.offer(keys, ids, verdicts, 1)  # the same rows again: the model's outputs, serials from 2
    assert got.n_examined > 3 and st.model.entries[0] == (100, ids[0], 2)
    st.close()


def test_refusals(sctx, bbp):
    lib, h = bbp.lib, sctx.handle
    n, s = ctypes.c_uint32(7), ctypes.c_uint32(99)
    r = ctypes.byref(n)
    one, four = bytes(64), bytes(128)
    out = (ctypes.c_int32 * 4)()
    v = (ctypes.c_int32 * 4)(OK, OK, OK, VERIFY)
    # bbp_standing_open: a NULL pointer, N == 0, N > BBP_MAX_ITEMS, K, in this order
    for N, K, rc_ in ((0, 0, BAD_ARG), (203, 0, GENS_LEN), (203, 1025, GENS_LEN), (8, 0, BAD_ARG), (8, 1025, BAD_ARG)):
        assert lib.bbp_standing_open(h, N, TABLE8, one, K, ctypes.byref(s)) == rc_ and s.value == 99, (N, K)
    assert lib.bbp_standing_open(h, 0, None, one, 0, ctypes.byref(s)) == BAD_ARG and lib.bbp_standing_open(h, 203, TABLE8, one, 1, None) == BAD_ARG
    # 64 open, the 65th refused; a closed handle is handed out again
    handles = [sctx.standing_open(8, TABLE8, 0, 1 + i) for i in range(64)]
    assert handles == list(range(64))
    assert lib.bbp_standing_open(h, 8, TABLE8, one, 1, ctypes.byref(s)) == BAD_ARG
    sctx.standing_close(5)
    assert sctx.standing_open(8, TABLE8, 0, 1024) == 5
    for x in handles[1:]:
        sctx.standing_close(x)
    # closed and never-opened handles, before the NULL check
    for bad in (1, 63, 64, 0xffffffff):
        assert lib.bbp_standing_offer(h, bad, 1, None, 0, 0, None, None, None, None, None, None) == BAD_ARG
        assert lib.bbp_debug_standing_offer(h, bad, 1, None, None, None, 0, 0, None, None, None, None, None, None) == BAD_ARG
        assert lib.bbp_standing_read(h, bad, 0, None, None, None, r, None) == BAD_ARG
        assert lib.bbp_standing_close(h, bad) == BAD_ARG
        assert lib.bbp_debug_standing_trip(h, bad, 1) == BAD_ARG
    # handle 0 is open: a NULL pointer, then B
    top = bbp.SELECT_MAX_BIDS
    assert lib.bbp_standing_offer(h, 0, top + 1, None, 0, 0, None, r, r, r, r, out) == BAD_ARG
    assert lib.bbp_standing_offer(h, 0, 1, one, 0, 1, None, r, r, r, r, out) == BAD_ARG      # entered_out with cap > 0
    assert lib.bbp_standing_offer(h, 0, 1, one, 0, 0, None, r, r, r, None, out) == BAD_ARG   # n_duplicates
    assert lib.bbp_standing_offer(h, 0, top + 1, one, 0, 0, None, r, r, r, r, out) == BAD_ARG
    n.value = 7
    assert lib.bbp_standing_offer(h, 0, 0, one, 0, 0, None, r, r, r, r, out) == OK and n.value == 0  # B == 0: zero counts, nothing changes
    assert lib.bbp_debug_standing_offer(h, 0, 4, four, None, v, 0, 0, None, r, r, r, r, out) == BAD_ARG  # ids
    assert lib.bbp_debug_standing_offer(h, 0, top + 1, four, four, v, 0, 0, None, r, r, r, r, out) == BAD_ARG
    assert lib.bbp_debug_standing_offer(h, 0, 1, one, one, (ctypes.c_int32 * 1)(DUPLICATE), 0, 0, None, r, r, r, r, out) == BAD_ARG  # a verdict outside the three
    assert lib.bbp_debug_standing_trip(h, 0, 0) == BAD_ARG
    got = sctx.standing_read(0)
    assert (got.n_entries, got.n_offered) == (0, 0)
    # cap below the count truncates; any output except n_entries may be NULL
    sctx.debug_standing_offer(0, bc.b32(9), bytes(32), [OK])
    sctx.standing_close(0)
    st = sctx.standing_open(8, TABLE8, 0, 4)
    assert st == 0 and sctx.standing_read(0).n_entries == 0  # a reused handle starts empty
    sctx.debug_standing_offer(0, bc.b32(9) + bc.b32(8), bytes(32) + bytes([1]) * 32, [OK, OK])
    got = sctx.standing_read(0, cap=1)
    assert (got.n_entries, got.n_offered, got.serials, got.scores) == (2, 2, [0], [bc.b32(9)])
    assert lib.bbp_standing_read(h, 0, 4, None, None, None, r, None) == OK and n.value == 2
    sctx.standing_close(0)
    # a pool refuses the hooks
    pool = bbp.Pool([0, 0])
    try:
        ph = pool.standing_open(8, TABLE8, 0, 2)
        assert lib.bbp_debug_standing_offer(pool.handle, ph, 1, one, one, out, 0, 0, None, r, r, r, r, out) == BAD_ARG
        assert lib.bbp_debug_standing_trip(pool.handle, ph, 1) == BAD_ARG
        pool.standing_close(ph)
    finally:
        pool.close()


# ---- proof-backed, N = 8 -----------------------------------------------------------------------------------------------------------------
N8 = 8


def _field(row, N, which):
    at = 1121 + 32 * (4 + N) + (32 if which == "z_img" else 0)
    return at, int.from_bytes(row[at:at + 32], "little")


def _set(row, N, which, value):
    at, _ = _field(row, N, which)
    return row[:at] + bc.b32(value) + row[at + 32:]


class Case:
    """Six bids with distinct k, proved twice under different entropy (the same score and z_img, different record bytes), a byte-equal
    resend, and three rows that must not enter: a flipped record byte, the top identity's z_img under a forged higher score, z_img + l."""

    def __init__(self, c, bbp):
        N = self.N = N8
        r = rc.honest(N, 6, 71)
        size = self.size = bbp.round_row_size(N)
        proved = []
        for tag in (71, 72):
            rows, _, st = c.prove_round(N, r.table, r.bid_bytes, rc.entropy(tag, 6, N))
            assert st == [OK] * 6
            proved.append([rows[size * i:size * (i + 1)] for i in range(6)])
        first, again = proved
        assert all(a != b and a[-64:] == b[-64:] for a, b in zip(first, again))
        top = max(range(6), key=lambda i: _field(first[i], N, "score")[1])
        flipped = bytearray(again[(top + 1) % 6])
        flipped[T_X] ^= 0x01
        borrowed = _set(first[top], N, "score", L - 1)
        shifted = _set(first[(top + 2) % 6], N, "z_img", _field(first[(top + 2) % 6], N, "z_img")[1] + L)
        # the forged row arrives in the first burst, ahead of most of the honest ones
        self.row_list = again[:3] + [borrowed] + first + again[3:] + [first[top], bytes(flipped), shifted]
        self.B = len(self.row_list)
        self.table = r.table
        self.keys = [_field(x, N, "score")[1] for x in self.row_list]
        self.ids = [x[-32:] for x in self.row_list]
        self.verdicts = c.verify_rounds([N], self.table, None, b"".join(self.row_list))
        self.bursts = (slice(0, 5), slice(5, 11), slice(11, self.B))


@pytest.fixture(scope="module")
def case(sctx, bbp):
    c = Case(sctx, bbp)
    assert c.verdicts.count(OK) == c.B - 3 and c.verdicts[3] == VERIFY and c.verdicts[-2:] == [VERIFY, FORMAT]
    return c


def _offers_against_verify_rounds(c, case, K, tranche):
    h = c.standing_open(case.N, case.table, 0, K)
    model = sc.Standing(0, K)
    try:
        for sl in case.bursts + (slice(0, case.B),):  # ... and a fourth burst that resends every row
            rows = case.row_list[sl]
            got = c.standing_offer(h, case.N, b"".join(rows), tranche, fill=FILL)
            want = model.offer(case.keys[sl], case.ids[sl], case.verdicts[sl], tranche)
            _check(got, want, len(rows), (K, tranche, sl))
            resend = sl.stop - sl.start == case.B
            upto = case.B if resend else sl.stop
            truth = sc.truth(case.keys[:upto], case.ids[:upto], case.verdicts[:upto], 0, K)
            assert [(k, i) for k, i, _ in model.entries] == [(k, i) for k, i, _ in truth]
            read = c.standing_read(h)
            assert (read.n_entries, read.n_offered, read.serials) == (len(model.entries), model.offered, [s for _, _, s in model.entries])
            every = case.row_list + case.row_list  # serial -> row: the first pass, then the resend
            assert read.scores == [every[s][-64:-32] for s in read.serials] and read.z_imgs == [every[s][-32:] for s in read.serials]
            assert len(set(read.z_imgs)) == len(read.z_imgs) and all((case.verdicts * 2)[s] == OK for s in read.serials)
            if resend:  # only rows whose verdict is not OK are verified again; nothing enters
                assert got.n_entered == 0 and all(s in (SKIPPED, DUPLICATE) for s, v in zip(got.status, case.verdicts) if v == OK)
                assert got.n_examined == sum(1 for s in got.status if s not in (SKIPPED, DUPLICATE)) <= 3
        assert len(model.entries) == min(K, 6)
    finally:
        c.standing_close(h)


@pytest.mark.parametrize("K,tranche", [(1, 1), (1, 0), (3, 1), (3, 0)])
def test_host_form_against_verify_rounds(sctx, case, K, tranche):
    _offers_against_verify_rounds(sctx, case, K, tranche)


def test_pool(sctx, bbp, case):
    pool = bbp.Pool([0, 0])
    try:
        for K, tranche in ((1, 1), (1, 0), (3, 1), (3, 0)):
            _offers_against_verify_rounds(pool, case, K, tranche)
    finally:
        pool.close()
