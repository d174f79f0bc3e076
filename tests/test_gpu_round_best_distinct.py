"""GPU tier: the best proofs of a round, one per bidder (include/bbp.h bbp_verify_round_best_distinct, its _dev form,
bbp_debug_round_best_distinct).  Hook-backed tests hold the shipped key, identity, selection, mark, settle, holder, drop and ranking
kernels to the model of tests/round_best_distinct_cases.py on made-up keys, ids and verdicts; proof-backed tests hold the public forms
to the model applied to the statuses that bbp_verify_rounds returns for all rows.  A hook call that ends BBP_ERR_INTERNAL (a bounded loop
of the identity table ran out) raises BbpError and fails its test."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc
from tests import round_best_distinct_cases as dc

bc = dc.bc
pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG, SKIPPED, DUPLICATE = 0, 1, 3, 4, -1, -2
L = dc.L
FILL = 0x6E
FILL_U32 = int.from_bytes(bytes([FILL]) * 4, "little")
T_X = 257  # byte offset of t_x in a record: the version byte, then eight points


@pytest.fixture(scope="module")
def bctx(ctx, bbp):
    """A context of this module's own (after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _check(got, want, cap, what):
    best, n_best, n_cand, n_exam, n_dup, status = want
    assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.n_duplicates) == (best[:cap], n_best, n_cand, n_exam, n_dup), what
    if got.status is not None:
        assert got.status == status, what
    assert got.raw[min(n_best, cap):] == [FILL_U32] * (cap - min(n_best, cap)), what  # entries at or beyond min(n_best, cap) are not written


def tightest_log2(verdicts):
    """the least table_log2 the hook takes: 2^t > the number of OK verdicts"""
    t = 1
    while (1 << t) <= verdicts.count(OK):
        t += 1
    return t


def _hook(c, keys, ids, verdicts, floor, K, tranche, cap, table_log2=0):
    return c.debug_round_best_distinct(b"".join(bc.b32(k) for k in keys), b"".join(ids), verdicts, floor, K, tranche, cap=cap, table_log2=table_log2, fill=FILL)


# ---- hook-backed: identities, selection and bookkeeping only -----------------------------------------------------------------------------
def _ok_count_one_below_a_power_of_two(B):
    """OK on 2^m - 1 rows (the most that fit), VERIFY on the rest: the tightest table then has exactly one slot more than OK rows"""
    m = 1
    while (1 << (m + 1)) - 1 <= B:
        m += 1
    n = (1 << m) - 1
    return [OK] * n + [VERIFY] * (B - n)


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 130, 1000])
def test_hook_against_the_model(bctx, B):
    n_cases = n_one_empty = n_dups = 0
    for p, n_ids in enumerate(dc.id_pools(B)):
        keys = (bc.keys_uniform, bc.keys_low_byte)[p % 2](B, 11 * B + p)  # the low-byte keys: ties, the index orders them
        ids = dc.id_pool(B, n_ids, 13 * B + p)
        for vname, verdicts in (("ok", [OK] * B), ("third", bc.verdicts_top_third_bad(keys)), ("pow2m1", _ok_count_one_below_a_power_of_two(B))):
            tight = tightest_log2(verdicts)
            for tranche in (1, 4, 0):
                for K in sorted({0, 1, 3, B}):
                    want = dc.model(keys, ids, verdicts, 0, K, tranche)
                    cap = 2 if (K == 0 and tranche == 4) else (K or B)  # one arm with less room than answers
                    for table_log2 in (0, tight):
                        what = (B, n_ids, vname, tranche, K, table_log2)
                        _check(_hook(bctx, keys, ids, verdicts, 0, K, tranche, cap, table_log2), want, cap, what)
                        n_cases += 1
                    assert want[3] + want[4] <= want[2] and len({ids[i] for i in want[0]}) == want[1], what
                    n_dups += want[4] > 0
                    # one empty slot for real: every OK row of its own identity, all of them examined
                    n_one_empty += vname == "pow2m1" and n_ids == B and K == 0 and (1 << tight) == want[1] + 1
    assert n_cases == 4 * 3 * 3 * len({0, 1, 3, B}) * 2 and n_one_empty >= 3 and (B < 63 or n_dups > 0)


def test_hook_one_identity_on_both_sides_of_a_wave_and_workgroup_boundary(bctx):
    """B = 130, K = 0: one tranche whose rows the settle launch takes in index order, one lane each -- rows 63 and 64 are the last lane of
    workgroup 0 and the first of workgroup 1.  They share an identity, both are OK, the higher key sits on the higher index: row 64 holds."""
    B = 130
    keys = [1000 + i for i in range(B)]
    ids = dc.id_pool(B, B, 3)
    ids[64] = ids[63]
    want = dc.model(keys, ids, [OK] * B, 0, 0, 1)
    assert 64 in want[0] and 63 not in want[0] and want[1] == B - 1 and want[5] == [OK] * B
    for table_log2 in (0, 8):
        _check(_hook(bctx, keys, ids, [OK] * B, 0, 0, 1, B, table_log2), want, B, table_log2)
    keys[63], keys[64] = keys[64], keys[63]  # ... and the other way round
    want = dc.model(keys, ids, [OK] * B, 0, 0, 1)
    assert 63 in want[0] and 64 not in want[0]
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 0, 1, B), want, B, "swapped")
    keys[63] = keys[64]  # ... and equal keys: the lower index
    want = dc.model(keys, ids, [OK] * B, 0, 0, 1)
    assert 63 in want[0] and 64 not in want[0]
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 0, 1, B), want, B, "equal keys")


def test_hook_ids_equal_in_31_bytes(bctx):
    """identities that differ in byte 0 only, or in byte 31 only, are different bidders"""
    rnd = random.Random(4)
    base = rnd.randbytes(32)
    near = [base, bytes([base[0] ^ 1]) + base[1:], base[:31] + bytes([base[31] ^ 0x80]), base[:31] + bytes([base[31] ^ 1])]
    B = 70
    keys = bc.keys_uniform(B, 5)
    ids = [near[i % 4] for i in range(B)]
    for K, tranche in ((0, 1), (4, 1), (3, 4), (5, 1)):
        want = dc.model(keys, ids, [OK] * B, 0, K, tranche)
        assert want[1] == (min(K, 4) if K else 4)
        _check(_hook(bctx, keys, ids, [OK] * B, 0, K, tranche, K or B), want, K or B, (K, tranche))
        _check(_hook(bctx, keys, ids, [OK] * B, 0, K, tranche, K or B, 7), want, K or B, (K, tranche, "tight"))


def test_hook_every_row_one_identity(bctx):
    B = 200
    keys = bc.keys_low_byte(B, 6)
    ids = [bytes(range(32))] * B
    # K = 0: one tranche, every row verified and OK, one winner -- the first in candidate order
    want = dc.model(keys, ids, [OK] * B, 0, 0, 1)
    assert (want[1], want[3], want[4], want[5]) == (1, B, 0, [OK] * B)
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 0, 1, B), want, B, "K = 0")
    # K = 2 can never be met: after tranche 0 (two rows) every candidate that is left is a duplicate, and nothing more is verified
    want = dc.model(keys, ids, [OK] * B, 0, 2, 1)
    assert (want[1], want[2], want[3], want[4]) == (1, B, 2, B - 2) and want[5].count(DUPLICATE) == B - 2
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 2, 1, 2), want, 2, "all duplicates")
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 2, 1, 2, 8), want, 2, "all duplicates, explicit table")
    # K = 1 is met by tranche 0: the call stops, the rest stays SKIPPED -- no drop pass after the last tranche
    want = dc.model(keys, ids, [OK] * B, 0, 1, 4)
    assert (want[1], want[3], want[4]) == (1, 4, 0) and want[5].count(SKIPPED) == B - 4
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 1, 4, 1), want, 1, "stop")
    # the top row forged under the victim's identity: it settles nothing, the victim's row stays live and wins
    verdicts = [OK] * B
    top = want[0][0]
    verdicts[top] = VERIFY
    want = dc.model(keys, ids, verdicts, 0, 1, 1)
    assert want[0] != [top] and want[1] == 1 and want[5][top] == VERIFY and want[4] == 0
    _check(_hook(bctx, keys, ids, verdicts, 0, 1, 1, 1), want, 1, "forged top")


def test_hook_contention(bctx):
    """B = 65 536 rows of 202 identities, all OK, K = 0: one tranche, 65 536 inserts that meet on 202 slots.  The outputs are the
    model's; the call returns BBP_OK, so the flag word of the bounded loops stayed clear."""
    B = 65536
    keys = bc.keys_uniform(B, 8)
    ids = dc.id_pool(B, 202, 9)
    want = dc.model(keys, ids, [OK] * B, 0, 0, 0)
    assert (want[1], want[3], want[4]) == (202, B, 0)
    _check(_hook(bctx, keys, ids, [OK] * B, 0, 0, 0, B), want, B, "contention")


def test_hook_refuses_bad_input(bctx, bbp):
    one, n = bytes(32), ctypes.c_uint32()
    v = (ctypes.c_int32 * 4)(OK, OK, OK, VERIFY)
    four = bytes(128)
    out = (ctypes.c_int32 * 4)()
    r = ctypes.byref(n)
    h = bctx.handle
    f = bbp.lib.bbp_debug_round_best_distinct
    assert f(h, 4, four, four, v, one, 1, 1, 1, 0, out, r, r, r, r, out) == OK
    assert f(h, 4, four, four, v, one, 1, 1, 1, 2, out, r, r, r, r, out) == OK        # 4 slots > 3 OK verdicts
    assert f(h, 4, four, four, v, one, 1, 1, 1, 1, out, r, r, r, r, out) == BAD_ARG   # 2 slots
    assert f(h, 4, four, four, v, one, 1, 1, 1, 21, out, r, r, r, r, out) == OK
    assert f(h, 4, four, four, v, one, 1, 1, 1, 22, out, r, r, r, r, out) == BAD_ARG
    assert f(h, 0, four, four, v, one, 1, 1, 1, 0, out, r, r, r, r, out) == BAD_ARG
    assert f(h, bbp.SELECT_MAX_BIDS + 1, four, four, v, one, 1, 1, 1, 0, out, r, r, r, r, out) == BAD_ARG
    assert f(h, 1, one, one, (ctypes.c_int32 * 1)(DUPLICATE), one, 1, 1, 1, 0, out, r, r, r, r, out) == BAD_ARG
    assert f(h, 4, four, None, v, one, 1, 1, 1, 0, out, r, r, r, r, out) == BAD_ARG
    assert f(h, 4, four, four, v, one, 1, 1, 1, 0, out, r, r, r, None, out) == BAD_ARG  # n_duplicates


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
    resend, and three rows that must not win: a flipped record byte, the top identity's z_img under a higher claimed score, z_img + l."""

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
        assert all(a != b and a[-64:] == b[-64:] for a, b in zip(first, again))  # fresh blindings: other bytes, the same score || z_img
        assert len({x[-32:] for x in first}) == 6
        top = max(range(6), key=lambda i: _field(first[i], N, "score")[1])
        flipped = bytearray(again[(top + 1) % 6])
        flipped[T_X] ^= 0x01
        borrowed = _set(first[top], N, "score", L - 1)
        shifted = _set(first[(top + 2) % 6], N, "z_img", _field(first[(top + 2) % 6], N, "z_img")[1] + L)
        self.row_list = again[:3] + first + again[3:] + [first[top], bytes(flipped), borrowed, shifted]
        self.B = len(self.row_list)
        self.bad = {self.B - 3: VERIFY, self.B - 2: VERIFY, self.B - 1: FORMAT}
        self.table, self.rows = r.table, b"".join(self.row_list)
        self.keys = [_field(x, N, "score")[1] for x in self.row_list]
        self.ids = [x[-32:] for x in self.row_list]
        self.verdicts = c.verify_rounds([N], self.table, None, self.rows)

    def want(self, K, tranche):
        return dc.model(self.keys, self.ids, self.verdicts, 0, K, tranche)


@pytest.fixture(scope="module")
def case(bctx, bbp):
    c = Case(bctx, bbp)
    # what bbp_verify_rounds says of the three rows that must not win -- a z_img that is not canonical is BBP_ERR_FORMAT, never BBP_OK,
    # which is why comparing identities as bytes is exact (csrc/round_best.h)
    assert [c.verdicts[i] for i in sorted(c.bad)] == [c.bad[i] for i in sorted(c.bad)] and c.verdicts.count(OK) == c.B - 3
    assert c.ids[c.B - 1] not in c.ids[:c.B - 1]
    return c


def _dev_form(c, case, K, tranche, cap, offset=0):
    import torch
    buf = torch.frombuffer(bytearray(bytes(offset) + case.rows), dtype=torch.uint8).cuda()
    tab = torch.frombuffer(bytearray(case.table), dtype=torch.uint8).cuda()
    ent = torch.frombuffer(bytearray(random.Random(case.B + offset).randbytes(32 * case.B)), dtype=torch.uint8).cuda()
    status = torch.full((4 * case.B,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = c.verify_round_best_distinct_dev(case.N, tab.data_ptr(), case.B, buf.data_ptr() + offset, ent.data_ptr(), status.data_ptr(), 0, K, tranche, cap=cap,
                                           stream=s.cuda_stream, fill=FILL)
    s.synchronize()
    raw = bytes(status.cpu().numpy().tobytes())
    return got._replace(status=[int.from_bytes(raw[4 * i:4 * i + 4], "little", signed=True) for i in range(case.B)])


def _distinct(case, got):
    assert len({case.ids[i] for i in got.best}) == len(got.best)  # no two rows of best carry one z_img
    assert all(case.verdicts[i] == OK for i in got.best)


@pytest.mark.parametrize("K,tranche", [(1, 1), (1, 0), (3, 1), (3, 0), (0, 1), (0, 0)])
def test_all_forms_against_verify_rounds(bctx, bbp, case, K, tranche):
    c = case
    want = c.want(K, tranche)
    cap = K or c.B
    assert want[1] == (K or 6) and want[5][c.B - 2] == VERIFY and (K or want[5][c.B - 1] == FORMAT)  # six bidders; the borrowed z_img is examined first and fails
    for what, got in (("host", bctx.verify_round_best_distinct(c.N, c.table, c.rows, 0, K, tranche, fill=FILL)), ("dev", _dev_form(bctx, c, K, tranche, cap)),
                      ("dev + 1", _dev_form(bctx, c, K, tranche, cap, offset=1))):
        _check(got, want, cap, what)
        _distinct(c, got)


def test_the_existing_call_returns_copies(bctx, bbp, case):
    """what the new calls are for: with K = 3 bbp_verify_round_best's answer holds one bidder more than once"""
    c = case
    old = bctx.verify_round_best(c.N, c.table, c.rows, 0, 3, 1, fill=FILL)
    assert old.n_best == 3 and len({c.ids[i] for i in old.best}) < 3
    new = bctx.verify_round_best_distinct(c.N, c.table, c.rows, 0, 3, 1, fill=FILL)
    assert new.n_best == 3 and len({c.ids[i] for i in new.best}) == 3 and new.best[0] == old.best[0]


def test_pool(bctx, bbp, case):
    import torch
    c = case
    pool = bbp.Pool([0, 0])
    try:
        for K in (1, 3, 0):
            for tranche in (1, 0):
                got = pool.verify_round_best_distinct(c.N, c.table, c.rows, 0, K, tranche, fill=FILL)
                _check(got, c.want(K, tranche), K or c.B, ("pool", K, tranche))
                _distinct(c, got)
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        one, n = bytes(64), ctypes.c_uint32()
        r = ctypes.byref(n)
        out = (ctypes.c_int32 * 4)()
        assert bbp.lib.bbp_verify_round_best_distinct_dev(pool.handle, 8, p, 1, p, p, one, 1, 1, 1, out, r, r, r, r, p, None) == BAD_ARG
        assert bbp.lib.bbp_debug_round_best_distinct(pool.handle, 1, one, one, out, one, 1, 1, 1, 0, out, r, r, r, r, out) == BAD_ARG
    finally:
        pool.close()


def test_screening_order(bctx, bbp):
    import torch
    lib, h = bbp.lib, bctx.handle
    n = ctypes.c_uint32(7)
    r = ctypes.byref(n)
    one = bytes(64)
    out = (ctypes.c_int32 * 4)()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    top = bbp.SELECT_MAX_BIDS
    for N, B, rc_ in ((0, top + 1, BAD_ARG), (203, top + 1, 2), (8, top + 1, BAD_ARG), (203, 0, 2), (0, 0, BAD_ARG)):
        assert lib.bbp_verify_round_best_distinct(h, N, one, B, one, one, 1, 1, 1, out, r, r, r, r, out) == rc_, (N, B)
        assert lib.bbp_verify_round_best_distinct_dev(h, N, p, B, p, p, one, 1, 1, 1, out, r, r, r, r, p, None) == rc_, (N, B)
    n.value = 7
    assert lib.bbp_verify_round_best_distinct(h, 8, one, 0, one, one, 1, 1, 1, out, r, r, r, r, out) == OK and n.value == 0  # B == 0: all counts zero
    n.value = 7
    assert lib.bbp_verify_round_best_distinct_dev(h, 8, p, 0, p, p, one, 1, 1, 1, out, r, r, r, r, p, None) == OK and n.value == 0
    assert lib.bbp_verify_round_best_distinct(h, 8, one, 1, one, one, 1, 1, 1, None, r, r, r, r, out) == BAD_ARG   # best_out with cap > 0
    assert lib.bbp_verify_round_best_distinct(h, 8, one, 1, one, one, 1, 1, 1, out, r, r, r, None, out) == BAD_ARG  # n_duplicates
    assert lib.bbp_verify_round_best_distinct_dev(h, 8, p, 1, p, p, one, 1, 1, 1, out, r, r, r, None, p, None) == BAD_ARG
