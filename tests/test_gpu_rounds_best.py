"""GPU tier: the best valid proofs of many rounds (include/bbp.h bbp_verify_rounds_best, bbp_verify_rounds_best_dev,
bbp_debug_rounds_best).  Hook-backed tests hold the shipped kernels of csrc/rounds_best.h to the model of tests/rounds_best_cases.py on
made-up keys and verdicts; proof-backed tests hold both public forms to (a) the model applied to the statuses that bbp_verify_rounds
returns for all rows and (b) one existing bbp_verify_round_best call per round."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc
from tests import round_best_cases as bc
from tests import rounds_best_cases as mc
from tests.test_gpu_round_best import _score, _tamper

pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, SKIPPED = 0, 1, 2, 3, 4, -1
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
    best, n_best, n_cand, n_exam, steps, status = want
    assert (got.n_best, got.n_candidates, got.n_examined, got.n_steps) == (n_best, n_cand, n_exam, steps), what
    assert got.best == [b[:cap] for b in best], what
    if got.status is not None:
        assert got.status == status, what
    for r, raw in enumerate(got.raw):  # entries at or beyond min(n_best[r], cap) of every round's part are not written
        assert raw[min(n_best[r], cap):] == [FILL_U32] * (cap - min(n_best[r], cap)), (what, r)


# ---- hook-backed: segments, selection and bookkeeping only -------------------------------------------------------------------------------
KEY_KINDS = {"uniform": bc.keys_uniform, "equal": lambda B, seed: [bc.keys_uniform(1, seed)[0]] * B, "low_byte": bc.keys_low_byte,
             "edges": bc.keys_edges}
VERDICTS = ("ok", "bad", "third", "uneven")
KS, TRANCHES = (0, 1, 3), (1, 4, 64)


def _verdicts(name, R, ro, keys, floors, K, tranche):
    if name == "ok":
        return [OK] * len(keys)
    if name == "bad":
        return [(VERIFY, FORMAT)[i % 2] for i in range(len(keys))]
    if name == "third":
        return mc.verdicts_top_third_bad(R, ro, keys, floors)
    return mc.verdicts_first_tranches_bad(R, ro, keys, floors, K, tranche)


# R = 1: the delegated single-round driver; 64 | 65: a wave of per-round lanes; 257: the scan's workgroup; 1000 x 1000: a row per round
@pytest.mark.parametrize("R,B", [(1, 1000), (2, 1000), (64, 1000), (65, 1000), (257, 1000), (1000, 1000), (300, 5000), (3, 1), (3, 65)])
def test_hook_against_the_model(bctx, R, B):
    n = 0
    seen = set()
    for mname, make in mc.MAPS.items():
        ro = make(B, R)
        for kind, keygen in KEY_KINDS.items():
            keys = keygen(B, 7 * B + R + len(kind))
            if mname == "holes":  # ... and a round that holds only keys >= l
                keys = [L + i if ro[i] == ro[0] else k for i, k in enumerate(keys)]
            key_bytes = b"".join(bc.b32(k) for k in keys)
            for _ in range(3 if B <= 1000 else 2):
                vname, K, tranche = VERDICTS[n % 4], KS[(n // 4) % 3], TRANCHES[(n // 12) % 3]
                floors = mc.floors_alternating(R, ro, keys) if n % 2 else None
                n += 1
                seen.add((vname, K, tranche))
                what = (R, B, mname, kind, vname, K, tranche, floors is not None)
                verdicts = _verdicts(vname, R, ro, keys, floors, K, tranche)
                want = mc.model(R, ro, keys, verdicts, floors, K, tranche)
                cap = 2 if (K == 0 and tranche == 4) else (K or B)  # one arm with less room than answers
                got = bctx.debug_rounds_best(R, ro, key_bytes, verdicts, floors, K, tranche, cap=cap, fill=FILL)
                _check(got, want, cap, what)
                if vname == "uneven":  # rounds stop at different steps: n_steps is the most, an early stopper examined its own tranches only
                    ran = [mc.tranches_run(c, e, K, tranche) for c, e in zip(got.n_candidates, got.n_examined)]
                    assert got.n_steps == max(ran), what
                    for r in range(R):
                        T0 = max(tranche, K) if K else got.n_candidates[r]
                        assert got.n_examined[r] == bc.examined_after(got.n_candidates[r], T0, ran[r]), (what, r)
    assert len(seen) >= (24 if B > 1000 else 36)


@pytest.mark.parametrize("n0", [255, 256, 257, 1025])
def test_hook_one_large_segment_beside_small_ones(bctx, n0):
    """skewed: round 0 holds n0 candidates (one workgroup walks them: the spans of 256 lanes), rounds 1 and 2 one row each"""
    B, R = n0 + 2, 3
    ro = mc.map_skewed(B, R)
    for kind in ("uniform", "equal", "low_byte"):
        keys = KEY_KINDS[kind](B, n0)
        kb = b"".join(bc.b32(k) for k in keys)
        for K, tranche, vname in ((1, 1, "uneven"), (3, 64, "third"), (0, 4, "ok"), (3, 4, "bad")):
            verdicts = _verdicts(vname, R, ro, keys, None, K, tranche)
            _check(bctx.debug_rounds_best(R, ro, kb, verdicts, None, K, tranche, fill=FILL), mc.model(R, ro, keys, verdicts, None, K, tranche), K or B,
                   (n0, kind, K, tranche))


def test_hook_refuses_bad_input(bctx, bbp):
    lib, h = bbp.lib, bctx.handle
    one = bytes(64)
    ro = (ctypes.c_uint32 * 2)(0, 1)
    v = (ctypes.c_int32 * 2)(OK, OK)
    out = (ctypes.c_uint32 * 8)()
    st = (ctypes.c_int32 * 2)()
    steps = ctypes.c_uint32()
    s = ctypes.byref(steps)

    def call(handle=h, R=2, B=2, ro=ro, keys=one, v=v, floors=one, best=out, nb=out, nc=out, ne=out, steps=s, status=st, cap=1):
        return lib.bbp_debug_rounds_best(handle, R, B, ro, keys, v, floors, 1, 1, cap, best, nb, nc, ne, steps, status)

    assert call() == OK and call(floors=None) == OK and call(steps=None) == OK and call(best=None, cap=0) == OK
    for null in ("keys", "v", "best", "nb", "nc", "ne", "status"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(ro=None) == BAD_ARG and call(R=1, ro=None) == OK          # round_of may be NULL with one round only
    assert call(B=0) == BAD_ARG and call(B=bbp.SELECT_MAX_BIDS + 1) == BAD_ARG
    assert call(R=0) == BAD_ARG and call(R=bbp.BEST_MAX_ROUNDS + 1) == BAD_ARG
    assert call(ro=(ctypes.c_uint32 * 2)(0, 2)) == BAD_ARG
    for bad in (SKIPPED, 2, BAD_ARG):
        assert call(v=(ctypes.c_int32 * 2)(OK, bad)) == BAD_ARG
    pool = bbp.Pool([0, 0])
    try:
        assert call(handle=pool.handle) == BAD_ARG
    finally:
        pool.close()


# ---- proof-backed ------------------------------------------------------------------------------------------------------------------------
class Rounds:
    """B rows over the rounds of list lengths Ns, row i in round i mod R, laid out by repetition of at most n_bids proved bids per round
    (so there are ties), some tampered; `verdicts` is what the existing bbp_verify_rounds says of every row."""

    def __init__(self, c, bbp, Ns, n_bids, B, tag, tamper, round_of=None):
        self.Ns, self.R, self.B = list(Ns), len(Ns), B
        self.round_of = round_of or [i % self.R for i in range(B)]
        self.tables, base = [], []
        for r, N in enumerate(Ns):
            hr = rc.honest(N, n_bids, tag + r)
            rows, _, st = c.prove_round(N, hr.table, hr.bid_bytes, rc.entropy(tag + r, n_bids, N))
            assert st == [OK] * n_bids
            size = bbp.round_row_size(N)
            base.append([rows[size * i:size * (i + 1)] for i in range(n_bids)])
            self.tables.append(hr.table)
        self.table = b"".join(self.tables)
        seen = [0] * self.R
        self.row_list = []
        for i in range(B):
            r = self.round_of[i]
            self.row_list.append(base[r][seen[r] % n_bids])
            seen[r] += 1
        for i, kind in tamper.items():
            self.row_list[i] = _tamper(self.row_list[i], Ns[self.round_of[i]], kind)
        self.rows = b"".join(self.row_list)
        self.keys = [_score(x, Ns[self.round_of[i]]) for i, x in enumerate(self.row_list)]
        self.verdicts = c.verify_rounds(self.Ns, self.table, self.round_of, self.rows)

    def want(self, floors, K, tranche, verdicts=None):
        return mc.model(self.R, self.round_of, self.keys, verdicts or self.verdicts, floors, K, tranche)

    def per_round(self, c, floors, K, tranche):
        """(b): one existing bbp_verify_round_best call per round, indices mapped back"""
        best, n_best, n_cand, n_exam, status, steps = [], [], [], [], [None] * self.B, 0
        for r, N in enumerate(self.Ns):
            mine = [i for i in range(self.B) if self.round_of[i] == r]
            got = c.verify_round_best(N, self.tables[r], b"".join(self.row_list[i] for i in mine), floors[r] if floors else 0, K, tranche, cap=self.B)
            best.append([mine[j] for j in got.best])
            n_best.append(got.n_best), n_cand.append(got.n_candidates), n_exam.append(got.n_examined)
            for j, i in enumerate(mine):
                status[i] = got.status[j]
            steps = max(steps, mc.tranches_run(got.n_candidates, got.n_examined, K, tranche))
        return best, n_best, n_cand, n_exam, steps, status


TAMPER37 = {0: "flip", 5: "top", 9: "score_l", 13: "scalar_l", 16: "flip", 21: "top", 30: "scalar_l", 36: "score_l"}


@pytest.fixture(scope="module")
def rounds37(bctx, bbp):
    c = Rounds(bctx, bbp, (8, 1, 25), 4, 37, 70, TAMPER37)
    assert [c.verdicts[i] for i in sorted(TAMPER37)] == [VERIFY, VERIFY, FORMAT, FORMAT, VERIFY, VERIFY, FORMAT, FORMAT]
    assert c.verdicts.count(OK) == 37 - len(TAMPER37)
    return c


def _dev_form(c, bbp, case, floors, K, tranche, cap, offset=0, table=None):
    import torch
    buf = torch.frombuffer(bytearray(bytes(offset) + case.rows), dtype=torch.uint8).cuda()
    tab = torch.frombuffer(bytearray(table or case.table), dtype=torch.uint8).cuda()
    ent = torch.frombuffer(bytearray(random.Random(case.B + offset).randbytes(32 * case.B)), dtype=torch.uint8).cuda()
    status = torch.full((4 * case.B,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = c.verify_rounds_best_dev(case.Ns, tab.data_ptr(), case.round_of, case.B, buf.data_ptr() + offset, ent.data_ptr(), status.data_ptr(), floors, K, tranche,
                                   cap=cap, stream=s.cuda_stream, fill=FILL)
    s.synchronize()
    raw = bytes(status.cpu().numpy().tobytes())
    return got._replace(status=[int.from_bytes(raw[4 * i:4 * i + 4], "little", signed=True) for i in range(case.B)])


def _host_form(c, case, floors, K, tranche, cap, table=None):
    return c.verify_rounds_best(case.Ns, table or case.table, case.round_of, case.rows, floors, K, tranche, cap=cap, fill=FILL)


@pytest.mark.parametrize("K,tranche", [(0, 1), (0, 4), (1, 1), (1, 4), (2, 1), (2, 4)])
def test_both_forms_against_verify_rounds_and_the_single_round_call(bctx, bbp, rounds37, K, tranche):
    c = rounds37
    honest = sorted(k for k, v in zip(c.keys, c.verdicts) if v == OK)
    for floors in (None, [honest[len(honest) // 2], 0, honest[len(honest) // 3]]):
        want = c.want(floors, K, tranche)
        assert c.per_round(bctx, floors, K, tranche) == want, ("(a) against (b)", floors)
        cap = K or c.B
        _check(_host_form(bctx, c, floors, K, tranche, cap), want, cap, ("host", floors))
        _check(_dev_form(bctx, bbp, c, floors, K, tranche, cap), want, cap, ("dev", floors))
    want = c.want(None, K, tranche)
    assert want[5][9] == FORMAT and want[5][36] == FORMAT                   # a score >= l: FORMAT, never examined
    assert want[5][5] == VERIFY and want[5][21] == VERIFY                    # the raised scores: examined first
    if K == 1 and tranche == 1:
        assert len(set(mc.tranches_run(a, b, K, tranche) for a, b in zip(want[2], want[3]))) > 1  # the rounds stop at different steps


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_dev_form_rows_at_any_alignment(bctx, bbp, rounds37, offset):
    c = rounds37
    for K, tranche, cap in ((1, 1, 1), (2, 4, 1), (0, 1, c.B)):
        _check(_dev_form(bctx, bbp, c, None, K, tranche, cap, offset=offset), c.want(None, K, tranche), cap, (offset, K))


def test_steps_in_engine_calls_of_a_few_rows(bctx, bbp, rounds37, monkeypatch):
    """BBP_HOST_CHUNK_VERIFY (read at every call) cuts a step into engine calls whose first row sits inside a round: parts of 5, both forms"""
    c = rounds37
    monkeypatch.setenv("BBP_HOST_CHUNK_VERIFY", "5")
    for K, tranche in ((0, 1), (2, 16)):
        want = c.want(None, K, tranche)
        _check(_host_form(bctx, c, None, K, tranche, K or c.B), want, K or c.B, ("host", K))
        _check(_dev_form(bctx, bbp, c, None, K, tranche, K or c.B, offset=1), want, K or c.B, ("dev", K))


def test_n202_rows_beside_an_n1_row_through_the_gather(bctx, bbp):
    """one round at N = 202 with two rows (7 777 bytes each) beside one at N = 1 with one row: the mixed-size gather; the N = 202 round's
    top claim is forged, so it runs a second step alone"""
    c = Rounds(bctx, bbp, (202, 1), 2, 3, 81, {0: "top"}, round_of=[0, 1, 0])
    assert bbp.round_row_size(202) == 7777 and c.verdicts == [VERIFY, OK, OK]
    want = c.want(None, 1, 1)
    assert want[:5] == ([[2], [1]], [1, 1], [2, 1], [2, 1], 2)
    _check(_host_form(bctx, c, None, 1, 1, 1), want, 1, "host")
    for offset in (0, 1, 3):
        _check(_dev_form(bctx, bbp, c, None, 1, 1, 1, offset=offset), want, 1, ("dev", offset))
    _check(_dev_form(bctx, bbp, c, None, 0, 1, 3, offset=2), c.want(None, 0, 1), 3, "dev, K = 0")


def test_non_canonical_seed_in_one_round(bctx, bbp, rounds37):
    """round 1's seed + l: every candidate of that round is examined and gets FORMAT; the other rounds are unaffected"""
    c = rounds37
    at = 32 * (1 + c.Ns[0])
    table = c.table[:at] + bc.b32(int.from_bytes(c.table[at:at + 32], "little") + L) + c.table[at + 32:]
    verdicts = bctx.verify_rounds(c.Ns, table, c.round_of, c.rows)
    assert all(v == FORMAT for i, v in enumerate(verdicts) if c.round_of[i] == 1)
    assert [v for i, v in enumerate(verdicts) if c.round_of[i] != 1] == [v for i, v in enumerate(c.verdicts) if c.round_of[i] != 1]
    want = c.want(None, 1, 4, verdicts)
    assert want[1][1] == 0 and want[3][1] == want[2][1] > 0
    clean = c.want(None, 1, 4)
    assert [want[k][r] for k in range(4) for r in (0, 2)] == [clean[k][r] for k in range(4) for r in (0, 2)]
    _check(_host_form(bctx, c, None, 1, 4, 1, table=table), want, 1, "host")
    _check(_dev_form(bctx, bbp, c, None, 1, 4, 1, table=table), want, 1, "dev")


def test_screening_order(bctx, bbp):
    import torch
    lib, h = bbp.lib, bctx.handle
    cnt = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    steps = ctypes.c_uint32(7)
    s = ctypes.byref(steps)
    one = bytes(64)
    out = (ctypes.c_int32 * 4)()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    top, rmax = bbp.SELECT_MAX_BIDS, bbp.BEST_MAX_ROUNDS
    u = lambda *v: (ctypes.c_uint32 * len(v))(*v)

    def host(R, Ns, B, ro, best=out, cap=1, rows=one):
        return lib.bbp_verify_rounds_best(h, R, Ns, one, B, ro, rows, None, 1, 1, cap, best, cnt, cnt, cnt, s, out)

    def dev(R, Ns, B, ro, best=out, cap=1, ent=p, status=p):
        return lib.bbp_verify_rounds_best_dev(h, R, Ns, p, B, ro, p, ent, None, 1, 1, cap, best, cnt, cnt, cnt, s, status, None)

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
        for k in range(4):
            cnt[k] = 7
        steps.value = 7
        assert form(2, u(8, 8), 0, None) == OK and list(cnt)[:2] == [0, 0] and steps.value == 0   # B == 0: every count of every round zero
    assert host(2, u(8, 8), 1, u(0), rows=None) == BAD_ARG
    assert dev(2, u(8, 8), 1, u(0), ent=None) == BAD_ARG and dev(2, u(8, 8), 1, u(0), status=None) == BAD_ARG


def test_pool(bctx, bbp, rounds37):
    import torch
    c = rounds37
    pool = bbp.Pool([0, 0])
    try:
        for K, tranche in ((1, 1), (2, 4), (0, 1)):
            got = pool.verify_rounds_best(c.Ns, c.table, c.round_of, c.rows, None, K, tranche, fill=FILL)
            assert got == _host_form(bctx, c, None, K, tranche, K or c.B)
            _check(got, c.want(None, K, tranche), K or c.B, ("pool", K))
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        cnt = (ctypes.c_uint32 * 4)()
        out = (ctypes.c_int32 * 4)()
        ns, ro = (ctypes.c_uint32 * 2)(8, 8), (ctypes.c_uint32 * 1)(0)
        assert bbp.lib.bbp_verify_rounds_best_dev(pool.handle, 2, ns, p, 1, ro, p, p, None, 1, 1, 1, out, cnt, cnt, cnt, None, p, None) == BAD_ARG
    finally:
        pool.close()
