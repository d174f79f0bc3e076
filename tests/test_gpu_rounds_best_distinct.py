"""GPU tier: the best proofs of many rounds, one per bidder (include/bbp.h bbp_verify_rounds_best_distinct, its _dev form,
bbp_debug_rounds_best_distinct).  Hook-backed tests hold the shipped kernels of csrc/rounds_best_distinct.h to the model of
tests/rounds_best_distinct_cases.py on made-up keys, ids and verdicts; proof-backed tests hold both public forms to (a) the model applied
to the statuses that bbp_verify_rounds returns for all rows and (b) one existing bbp_verify_round_best_distinct call per round."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc
from tests import round_best_cases as bc
from tests import rounds_best_cases as mc
from tests import rounds_best_distinct_cases as mdc
from tests.test_gpu_rounds_best import KEY_KINDS, KS, TAMPER37, TRANCHES, VERDICTS, Rounds, _tamper, _verdicts

pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, SKIPPED, DUPLICATE = 0, 1, 2, 3, 4, -1, -2
L = bc.L
FILL = 0x6E
FILL_U32 = int.from_bytes(bytes([FILL]) * 4, "little")


@pytest.fixture(scope="module")
def bctx(ctx, bbp):
    """A context of this module's own (after `ctx`, so torch's HIP runtime is initialised first); health flags 0 at teardown."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


def _check(got, want, cap, what):
    best, n_best, n_cand, n_exam, n_dups, steps, status = want[:7]
    assert (got.n_best, got.n_candidates, got.n_examined, got.n_duplicates, got.n_steps) == (n_best, n_cand, n_exam, n_dups, steps), what
    assert got.best == [b[:cap] for b in best], what
    if got.status is not None:
        assert got.status == status, what
    for r, raw in enumerate(got.raw):  # entries at or beyond min(n_best[r], cap) of every round's part are not written
        assert raw[min(n_best[r], cap):] == [FILL_U32] * (cap - min(n_best[r], cap)), (what, r)


def _tightest(verdicts):
    """the least table_log2 the hook accepts: 2^s slots, more than there are BBP_OK verdicts"""
    return max(1, verdicts.count(OK).bit_length())


def _hook(c, R, ro, keys, ids, verdicts, floors, K, tranche, cap=None, table_log2=0):
    return c.debug_rounds_best_distinct(R, ro, b"".join(bc.b32(k) for k in keys), b"".join(ids), verdicts, floors, K, tranche, cap=cap, table_log2=table_log2,
                                        fill=FILL)


# ---- hook-backed: identities, segments, selection and bookkeeping only ---------------------------------------------------------------------
# R = 1: the delegated single-round driver; 64 | 65: a wave of per-round lanes; 257: the scan's workgroup; 1000 x 1000: a row per round
@pytest.mark.parametrize("R,B", [(1, 1000), (2, 1000), (64, 1000), (65, 1000), (257, 1000), (1000, 1000), (300, 5000), (3, 1), (3, 65)])
def test_hook_against_the_model(bctx, R, B):
    n = 0
    seen, dropped, uneven = set(), 0, 0
    kinds = list(KEY_KINDS.items())
    for mname, make in mc.MAPS.items():
        ro = make(B, R)
        for scheme, n_ids in mdc.id_arms(B):
            for _ in range(2 if B <= 1000 else 1):
                kind, keygen = kinds[n % 4]
                keys = keygen(B, 7 * B + R + n)
                if mname == "holes" and n % 2:  # ... and a round that holds only keys >= l
                    keys = [L + i if ro[i] == ro[0] else k for i, k in enumerate(keys)]
                ids = mdc.make_ids(B, R, ro, scheme, n_ids, 11 * B + R + n)
                vname, K, tranche = VERDICTS[n % 4], KS[(n // 4) % 3], TRANCHES[(n // 12) % 3]
                floors = mc.floors_alternating(R, ro, keys) if n % 2 else None
                n += 1
                seen.add((vname, K, tranche))
                verdicts = _verdicts(vname, R, ro, keys, floors, K, tranche)
                log2 = _tightest(verdicts) if n % 3 == 0 else 0
                what = (R, B, mname, scheme, n_ids, kind, vname, K, tranche, floors is not None, log2)
                want = mdc.model(R, ro, keys, ids, verdicts, floors, K, tranche)
                cap = 2 if (K == 0 and tranche == 4) else (K or B)  # one arm with less room than answers
                got = _hook(bctx, R, ro, keys, ids, verdicts, floors, K, tranche, cap, log2)
                _check(got, want, cap, what)
                assert all(e + d <= c for e, d, c in zip(got.n_examined, got.n_duplicates, got.n_candidates)), what
                dropped += sum(got.n_duplicates) > 0
                uneven += len({t for t in want[7] if t}) > 1
    assert len(seen) >= (24 if B > 1000 or B < 100 else 36)
    if B >= 10 * R:  # rounds of some size: some arm drops rows (K = 3 only: K = 1 stops at the first identity), and rounds stop at different steps
        assert dropped >= 1 and (R == 1 or uneven >= 1), (dropped, uneven)


def test_hook_one_identity_in_every_one_of_1000_rounds(bctx):
    """the same 32 bytes in every round, the tightest table: 1000 identities, every round has its own winner"""
    R, B = 1000, 2000
    ro = mc.map_mod(B, R)
    keys = bc.keys_uniform(B, 5)
    ids = [b"\x5a" * 32] * B
    for K, tranche in ((0, 1), (1, 1), (2, 1)):
        verdicts = [OK] * B
        want = mdc.model(R, ro, keys, ids, verdicts, None, K, tranche)
        assert want[1] == [1] * R and want[0] == [[max((r, r + R), key=lambda i: (keys[i], -i))] for r in range(R)]
        assert want[4] == [0] * R and want[5] == 1  # K = 1 stops every round; K = 0 and K = 2 examine both rows of every round in one step
        _check(_hook(bctx, R, ro, keys, ids, verdicts, None, K, tranche, None, _tightest(verdicts)), want, K or B, (K, tranche))


def test_hook_flood_of_one_identity(bctx):
    """one round where every one of 1025 rows carries one identity and all are OK, beside two one-row rounds: with K = 0 one step inserts
    all of them (1024 exchanges at most for the last to get in: the bound is the step's size), with K = 3 the first step settles it and
    the drop pass takes the other 1022"""
    B, R = 1027, 3
    ro = mc.map_skewed(B, R)
    ids = [b"\x11" * 32] * 1025 + [b"\x11" * 32, b"\x22" * 32]
    for kind in ("uniform", "equal"):
        keys = KEY_KINDS[kind](B, 31)
        top = min(range(1025), key=lambda i: (-keys[i], i))
        for K, tranche, log2 in ((0, 1, 0), (0, 1, 11), (3, 1, 0), (3, 1, 11)):
            want = mdc.model(R, ro, keys, ids, [OK] * B, None, K, tranche)
            assert want[0] == [[top], [1025], [1026]] and want[5] == 1
            assert (want[3], want[4]) == (([1025, 1, 1], [0, 0, 0]) if K == 0 else ([3, 1, 1], [1022, 0, 0]))
            _check(_hook(bctx, R, ro, keys, ids, [OK] * B, None, K, tranche, None, log2), want, K or B, (kind, K, log2))


def test_hook_a_stopped_round_beside_running_ones(bctx):
    """hand case 3, scaled: round 0 settles its K identities in step 0 and stops; its 130 leftover rows carry settled identities, straddle
    a wave boundary of the drop pass, and stay SKIPPED while round 1 -- whose top claims fail -- runs on for more steps and drops its own"""
    B, R = 2 * 133, 2
    ro = mc.map_mod(B, R)
    keys = [10 ** 6 - i for i in range(B)]
    a, b, c = b"A" * 32, b"B" * 32, b"C" * 32
    for K in (1, 2):
        ids = [(a, b)[(i // 2) % 2] if i % 2 == 0 else a for i in range(B)]  # round 0: A, B, A, B, ... from the top; round 1: A throughout
        ids[2 * 40 + 1] = c                                                 # ... but for one row of another bidder deep in round 1
        verdicts = [OK] * B
        for j in range(6):                             # round 1's first two tranches fail entirely (T_0 = K, then 2 K)
            verdicts[2 * j + 1] = VERIFY
        want = mdc.model(R, ro, keys, ids, verdicts, None, K, 1)
        best, n_best, n_cand, n_exam, n_dups, steps, status, ran = want
        assert ran[0] == 1 and ran[1] > 2 and n_exam[0] == K and n_dups[0] == 0
        assert [status[i] for i in range(2 * K, B, 2)] == [SKIPPED] * (133 - K) and 133 - K > 64
        if K == 2:
            assert n_dups[1] == 133 - 14 - 1 and best[1] == [2 * 6 + 1, 2 * 40 + 1]  # round 1 drops the resent rows and reaches the other bidder
        for log2 in (0, _tightest(verdicts)):
            _check(_hook(bctx, R, ro, keys, ids, verdicts, None, K, 1, None, log2), want, K, (K, log2))
    for (verdicts, K, tranche), hand in mdc.HAND_CASES:  # ... and the hand cases themselves
        best, n_cand, n_exam, n_dups, steps, status = hand
        _check(_hook(bctx, 2, mdc.HAND_ROUND_OF, mdc.HAND_KEYS, mdc.HAND_IDS, verdicts, None, K, tranche), (best, [len(x) for x in best], n_cand, n_exam,
                                                                                                             n_dups, steps, status), K, ("hand", K))


@pytest.mark.parametrize("R,B", [(2, 1000), (65, 1000), (300, 5000)])
def test_hook_all_ids_distinct_is_the_plain_call(bctx, R, B):
    n = 0
    for mname, make in mc.MAPS.items():
        ro = make(B, R)
        keys = KEY_KINDS[("uniform", "equal", "low_byte", "edges")[n % 4]](B, B + R)
        kb = b"".join(bc.b32(k) for k in keys)
        ids = [i.to_bytes(4, "little") * 8 for i in range(B)]
        for vname in VERDICTS:
            K, tranche = KS[n % 3], TRANCHES[(n // 3) % 3]
            floors = mc.floors_alternating(R, ro, keys) if n % 2 else None
            n += 1
            verdicts = _verdicts(vname, R, ro, keys, floors, K, tranche)
            plain = bctx.debug_rounds_best(R, ro, kb, verdicts, floors, K, tranche, fill=FILL)
            got = bctx.debug_rounds_best_distinct(R, ro, kb, b"".join(ids), verdicts, floors, K, tranche, fill=FILL)
            assert got.n_duplicates == [0] * R
            assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.n_steps, got.status, got.raw) == tuple(plain), (mname, vname, K, tranche)


def test_hook_refuses_bad_input(bctx, bbp):
    lib, h = bbp.lib, bctx.handle
    one = bytes(64)
    ro = (ctypes.c_uint32 * 2)(0, 1)
    v = (ctypes.c_int32 * 2)(OK, OK)
    out = (ctypes.c_uint32 * 8)()
    st = (ctypes.c_int32 * 2)()
    steps = ctypes.c_uint32()
    s = ctypes.byref(steps)

    def call(handle=h, R=2, B=2, ro=ro, keys=one, ids=one, v=v, floors=one, best=out, nb=out, nc=out, ne=out, nd=out, steps=s, status=st, cap=1, log2=0):
        return lib.bbp_debug_rounds_best_distinct(handle, R, B, ro, keys, ids, v, floors, 1, 1, cap, log2, best, nb, nc, ne, nd, steps, status)

    assert call() == OK and call(floors=None) == OK and call(steps=None) == OK and call(best=None, cap=0) == OK
    for null in ("keys", "ids", "v", "best", "nb", "nc", "ne", "nd", "status"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(ro=None) == BAD_ARG and call(R=1, ro=None) == OK          # round_of may be NULL with one round only
    assert call(B=0) == BAD_ARG and call(B=bbp.SELECT_MAX_BIDS + 1) == BAD_ARG
    assert call(R=0) == BAD_ARG and call(R=bbp.BEST_MAX_ROUNDS + 1) == BAD_ARG
    assert call(ro=(ctypes.c_uint32 * 2)(0, 2)) == BAD_ARG
    for bad in (SKIPPED, DUPLICATE, 2, BAD_ARG):
        assert call(v=(ctypes.c_int32 * 2)(OK, bad)) == BAD_ARG
    # table_log2: above 21, or 2^table_log2 not above the number of BBP_OK verdicts (two here), with one round and with two
    for R_, ro_ in ((2, ro), (1, None)):
        assert call(R=R_, ro=ro_, log2=22) == BAD_ARG and call(R=R_, ro=ro_, log2=1) == BAD_ARG
        assert call(R=R_, ro=ro_, log2=2) == OK and call(R=R_, ro=ro_, log2=21) == OK
        assert call(R=R_, ro=ro_, log2=1, v=(ctypes.c_int32 * 2)(OK, VERIFY)) == OK
    pool = bbp.Pool([0, 0])
    try:
        assert call(handle=pool.handle) == BAD_ARG
    finally:
        pool.close()


# ---- proof-backed ------------------------------------------------------------------------------------------------------------------------
class DistinctRounds(Rounds):
    """tests/test_gpu_rounds_best.py's rows -- four proved bids per round, repeated, so duplicates are built in -- with `reprove`: {row:
    tag}, rows whose bid is proved a second time under other entropy (the same z_img in other bytes).  TAMPER37's "top" rows are the
    forgeries: a victim's z_img under a raised score."""

    def __init__(self, c, bbp, Ns, n_bids, B, tag, tamper, round_of=None, reprove=()):
        super().__init__(c, bbp, Ns, n_bids, B, tag, tamper, round_of)
        seen = [0] * self.R
        for i in range(B):
            r = self.round_of[i]
            if i in reprove:
                N, size = Ns[r], bbp.round_row_size(Ns[r])
                hr = rc.honest(N, n_bids, tag + r)
                rows, _, st = c.prove_round(N, hr.table, hr.bid_bytes, rc.entropy(reprove[i], n_bids, N))
                k = seen[r] % n_bids
                again = rows[size * k:size * (k + 1)]
                assert st == [OK] * n_bids and again != self.row_list[i] and again[-64:] == self.row_list[i][-64:]
                self.row_list[i] = again
            seen[r] += 1
        self.rows = b"".join(self.row_list)
        self.ids = [x[-32:] for x in self.row_list]
        self.verdicts = c.verify_rounds(self.Ns, self.table, self.round_of, self.rows)

    def want(self, floors, K, tranche, verdicts=None):
        return mdc.model(self.R, self.round_of, self.keys, self.ids, verdicts or self.verdicts, floors, K, tranche)[:7]

    def per_round(self, c, floors, K, tranche):
        """(b): one existing bbp_verify_round_best_distinct call per round, indices mapped back; the steps from the model's simulation"""
        best, n_best, n_cand, n_exam, n_dups, status = [], [], [], [], [], [None] * self.B
        for r, N in enumerate(self.Ns):
            mine = [i for i in range(self.B) if self.round_of[i] == r]
            got = c.verify_round_best_distinct(N, self.tables[r], b"".join(self.row_list[i] for i in mine), floors[r] if floors else 0, K, tranche, cap=self.B)
            best.append([mine[j] for j in got.best])
            n_best.append(got.n_best), n_cand.append(got.n_candidates), n_exam.append(got.n_examined), n_dups.append(got.n_duplicates)
            for j, i in enumerate(mine):
                status[i] = got.status[j]
        return best, n_best, n_cand, n_exam, n_dups, status


@pytest.fixture(scope="module")
def rounds37(bctx, bbp):
    c = DistinctRounds(bctx, bbp, (8, 1, 25), 4, 37, 70, TAMPER37, reprove={18: 170})  # row 18: round 0's seventh row, bid 2 again
    assert [c.verdicts[i] for i in sorted(TAMPER37)] == [VERIFY, VERIFY, FORMAT, FORMAT, VERIFY, VERIFY, FORMAT, FORMAT]
    assert c.verdicts.count(OK) == 37 - len(TAMPER37) and c.verdicts[18] == OK
    assert c.ids[18] == c.ids[6] and c.row_list[18] != c.row_list[6]            # the same bidder in other bytes
    for forged in (5, 21):                                                      # a victim's z_img under a raised score: fails, settles nothing
        victims = [i for i in range(37) if c.round_of[i] == c.round_of[forged] and c.ids[i] == c.ids[forged] and c.verdicts[i] == OK]
        assert c.keys[forged] == L - 1 and victims
    c.bidders = [len({c.ids[i] for i in range(37) if c.round_of[i] == r and c.verdicts[i] == OK}) for r in range(3)]  # with a valid row
    assert c.bidders == [4, 1, 4]  # (a list of one item holds one bid: all of round 1's rows are one bidder's)
    return c


def _dev_form(c, bbp, case, floors, K, tranche, cap, offset=0, table=None):
    import torch
    buf = torch.frombuffer(bytearray(bytes(offset) + case.rows), dtype=torch.uint8).cuda()
    tab = torch.frombuffer(bytearray(table or case.table), dtype=torch.uint8).cuda()
    ent = torch.frombuffer(bytearray(random.Random(case.B + offset).randbytes(32 * case.B)), dtype=torch.uint8).cuda()
    status = torch.full((4 * case.B,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = c.verify_rounds_best_distinct_dev(case.Ns, tab.data_ptr(), case.round_of, case.B, buf.data_ptr() + offset, ent.data_ptr(), status.data_ptr(), floors, K,
                                            tranche, cap=cap, stream=s.cuda_stream, fill=FILL)
    s.synchronize()
    raw = bytes(status.cpu().numpy().tobytes())
    return got._replace(status=[int.from_bytes(raw[4 * i:4 * i + 4], "little", signed=True) for i in range(case.B)])


def _host_form(c, case, floors, K, tranche, cap, table=None):
    return c.verify_rounds_best_distinct(case.Ns, table or case.table, case.round_of, case.rows, floors, K, tranche, cap=cap, fill=FILL)


@pytest.mark.parametrize("K,tranche", [(0, 1), (1, 1), (2, 1), (2, 4), (3, 0)])
def test_both_forms_against_verify_rounds_and_the_single_round_call(bctx, bbp, rounds37, K, tranche):
    c = rounds37
    honest = sorted(k for k, v in zip(c.keys, c.verdicts) if v == OK)
    for floors in (None, [honest[len(honest) // 2], 0, honest[len(honest) // 3]]):
        want = c.want(floors, K, tranche)
        best, n_best, n_cand, n_exam, n_dups, steps, status = want
        assert c.per_round(bctx, floors, K, tranche) == (best, n_best, n_cand, n_exam, n_dups, status), ("(a) against (b)", floors)
        cap = K or c.B
        for what, got in (("host", _host_form(bctx, c, floors, K, tranche, cap)), ("dev", _dev_form(bctx, bbp, c, floors, K, tranche, cap))):
            _check(got, want, cap, (what, floors))
            for r in range(c.R):  # no two rows of a round's best carry one z_img, and every one verified
                assert len({c.ids[i] for i in got.best[r]}) == len(got.best[r]) and all(c.verdicts[i] == OK for i in got.best[r])
    want = c.want(None, K, tranche)
    assert want[6][5] == VERIFY and want[6][21] == VERIFY                    # the forged rows: examined first, and they fail
    if K == 0:                                                               # every bidder once, the forgeries' victims among them; nothing dropped
        assert want[1] == c.bidders and sum(want[4]) == 0
        assert all(c.ids[forged] in {c.ids[i] for i in want[0][c.round_of[forged]]} for forged in (5, 21))
    if K == 2 and tranche == 1:
        assert sum(want[4]) > 0                                             # rows left the candidates unverified


def test_the_plain_call_returns_copies(bctx, bbp, rounds37):
    """what the new calls are for: with K = 3 bbp_verify_rounds_best's answer holds one bidder more than once"""
    c = rounds37
    old = bctx.verify_rounds_best(c.Ns, c.table, c.round_of, c.rows, None, 3, 1, fill=FILL)
    new = _host_form(bctx, c, None, 3, 1, 3)
    assert any(len({c.ids[i] for i in old.best[r]}) < len(old.best[r]) for r in range(c.R))
    assert all(len({c.ids[i] for i in new.best[r]}) == min(3, c.bidders[r]) == new.n_best[r] for r in range(c.R))
    assert [b[0] for b in new.best] == [b[0] for b in old.best]


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_dev_form_rows_at_any_alignment(bctx, bbp, rounds37, offset):
    c = rounds37
    for K, tranche, cap in ((1, 1, 1), (3, 1, 1), (0, 1, c.B)):
        _check(_dev_form(bctx, bbp, c, None, K, tranche, cap, offset=offset), c.want(None, K, tranche), cap, (offset, K))


def test_steps_in_engine_calls_of_a_few_rows(bctx, bbp, rounds37, monkeypatch):
    """BBP_HOST_CHUNK_VERIFY (read at every call) cuts a step into engine calls whose first row sits inside a round: parts of 5, both forms"""
    c = rounds37
    monkeypatch.setenv("BBP_HOST_CHUNK_VERIFY", "5")
    for K, tranche in ((0, 1), (3, 2)):
        want = c.want(None, K, tranche)
        _check(_host_form(bctx, c, None, K, tranche, K or c.B), want, K or c.B, ("host", K))
        _check(_dev_form(bctx, bbp, c, None, K, tranche, K or c.B, offset=1), want, K or c.B, ("dev", K))


def test_n202_rows_beside_an_n1_row_through_the_gather(bctx, bbp):
    """one round at N = 202 (7 777-byte rows) beside one at N = 1: the mixed-size gather.  The N = 202 round's top claim is a forgery of
    bid 0's z_img, and bid 0's honest row is there twice"""
    c = DistinctRounds(bctx, bbp, (202, 1), 2, 5, 81, {0: "top"}, round_of=[0, 1, 0, 0, 0])
    assert bbp.round_row_size(202) == 7777 and c.verdicts == [VERIFY, OK, OK, OK, OK]
    assert c.ids[0] == c.ids[3] and c.ids[2] == c.ids[4] and c.ids[0] != c.ids[2]
    for K, tranche in ((2, 1), (1, 1), (0, 1), (3, 1)):
        want = c.want(None, K, tranche)
        assert K == 1 or sorted(want[0][0]) == [2, 3]  # one row per bidder: the forgery fails, the resent row 4 does not win twice
        _check(_host_form(bctx, c, None, K, tranche, K or c.B), want, K or c.B, ("host", K))
        for offset in ((0, 1, 3) if K == 2 else (2,)):
            _check(_dev_form(bctx, bbp, c, None, K, tranche, K or c.B, offset=offset), want, K or c.B, ("dev", K, offset))


def test_non_canonical_seed_in_one_round(bctx, bbp, rounds37):
    """round 1's seed + l: every candidate of that round is examined and gets FORMAT, nothing settles, nothing is dropped there"""
    c = rounds37
    at = 32 * (1 + c.Ns[0])
    table = c.table[:at] + bc.b32(int.from_bytes(c.table[at:at + 32], "little") + L) + c.table[at + 32:]
    verdicts = bctx.verify_rounds(c.Ns, table, c.round_of, c.rows)
    assert all(v == FORMAT for i, v in enumerate(verdicts) if c.round_of[i] == 1)
    want = c.want(None, 2, 1, verdicts)
    assert want[1][1] == 0 and want[3][1] == want[2][1] > 0 and want[4][1] == 0
    clean = c.want(None, 2, 1)
    assert [want[k][r] for k in range(5) for r in (0, 2)] == [clean[k][r] for k in range(5) for r in (0, 2)]
    _check(_host_form(bctx, c, None, 2, 1, 2, table=table), want, 2, "host")
    _check(_dev_form(bctx, bbp, c, None, 2, 1, 2, table=table), want, 2, "dev")


def test_screening_order(bctx, bbp):
    import torch
    lib, h = bbp.lib, bctx.handle
    cnt = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    dup = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    steps = ctypes.c_uint32(7)
    s = ctypes.byref(steps)
    one = bytes(64)
    out = (ctypes.c_int32 * 4)()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    top, rmax = bbp.SELECT_MAX_BIDS, bbp.BEST_MAX_ROUNDS
    u = lambda *v: (ctypes.c_uint32 * len(v))(*v)

    def host(R, Ns, B, ro, best=out, cap=1, rows=one, nd=dup):
        return lib.bbp_verify_rounds_best_distinct(h, R, Ns, one, B, ro, rows, None, 1, 1, cap, best, cnt, cnt, cnt, nd, s, out)

    def dev(R, Ns, B, ro, best=out, cap=1, ent=p, status=p, nd=dup):
        return lib.bbp_verify_rounds_best_distinct_dev(h, R, Ns, p, B, ro, p, ent, None, 1, 1, cap, best, cnt, cnt, cnt, nd, s, status, None)

    for form in (host, dev):
        assert form(0, u(8), top + 1, u(5)) == BAD_ARG                   # R == 0 before everything else
        assert form(rmax + 1, u(0), 1, u(0)) == BAD_ARG                  # R above the limit: round_Ns is not looked at
        assert form(2, u(203, 0), top + 1, u(5, 5)) == BAD_ARG           # a 0 in round_Ns decides before an entry above BBP_MAX_ITEMS
        assert form(2, u(203, 8), top + 1, u(5, 5)) == GENS_LEN          # ... which decides before B
        assert form(2, u(8, 8), top + 1, u(5, 5)) == BAD_ARG             # B before round_of
        assert form(2, u(203, 8), 0, None) == GENS_LEN                   # the table is screened before B == 0 returns
        assert form(2, u(8, 8), 2, None) == BAD_ARG                      # round_of NULL with R > 1
        assert form(2, u(8, 8), 2, u(0, 2)) == BAD_ARG                   # round_of[i] >= R
        assert form(2, None, 1, u(0)) == BAD_ARG and form(2, u(8, 8), 1, u(0), best=None) == BAD_ARG
        assert form(2, u(8, 8), 1, u(0), nd=None) == BAD_ARG             # n_duplicates is a required pointer
        for k in range(4):
            cnt[k] = dup[k] = 7
        steps.value = 7
        assert form(2, u(8, 8), 0, None) == OK and list(cnt)[:2] == [0, 0] and list(dup)[:3] == [0, 0, 7] and steps.value == 0  # B == 0: zeros
    assert host(2, u(8, 8), 1, u(0), rows=None) == BAD_ARG
    assert dev(2, u(8, 8), 1, u(0), ent=None) == BAD_ARG and dev(2, u(8, 8), 1, u(0), status=None) == BAD_ARG


def test_pool(bctx, bbp, rounds37):
    import torch
    c = rounds37
    pool = bbp.Pool([0, 0])
    try:
        for K, tranche in ((1, 1), (3, 1), (0, 1)):
            got = pool.verify_rounds_best_distinct(c.Ns, c.table, c.round_of, c.rows, None, K, tranche, fill=FILL)
            assert got == _host_form(bctx, c, None, K, tranche, K or c.B)
            _check(got, c.want(None, K, tranche), K or c.B, ("pool", K))
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        cnt = (ctypes.c_uint32 * 4)()
        out = (ctypes.c_int32 * 4)()
        ns, ro = (ctypes.c_uint32 * 2)(8, 8), (ctypes.c_uint32 * 1)(0)
        assert bbp.lib.bbp_verify_rounds_best_distinct_dev(pool.handle, 2, ns, p, 1, ro, p, p, None, 1, 1, 1, out, cnt, cnt, cnt, cnt, None, p, None) == BAD_ARG
    finally:
        pool.close()
