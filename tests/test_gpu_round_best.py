"""GPU tier: the best valid proofs of a round (include/bbp.h bbp_verify_round_best, bbp_verify_round_best_dev, bbp_debug_round_best).
Hook-backed tests hold the shipped key, selection, mark and ranking kernels to the model of tests/round_best_cases.py on made-up keys
and verdicts; proof-backed tests hold both public forms to the model applied to the statuses that bbp_verify_rounds returns for all
rows (existing tests hold that call to the oracle)."""
import ctypes
import random

import pytest

from tests import prove_round_cases as rc
from tests import round_best_cases as bc

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG, SKIPPED = 0, 1, 3, 4, -1
L = bc.L
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
    best, n_best, n_cand, n_exam, status = want
    assert (got.best, got.n_best, got.n_candidates, got.n_examined) == (best[:cap], n_best, n_cand, n_exam), what
    if got.status is not None:
        assert got.status == status, what
    assert got.raw[min(n_best, cap):] == [FILL_U32] * (cap - min(n_best, cap)), what  # entries at or beyond min(n_best, cap) are not written


# ---- hook-backed: selection and bookkeeping only -----------------------------------------------------------------------------------------
KEY_KINDS = {"uniform": bc.keys_uniform, "equal": lambda B, seed: [bc.keys_uniform(1, seed)[0]] * B, "low_byte": bc.keys_low_byte,
             "edges": bc.keys_edges}


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025, 5000])  # 1025 crosses the first workgroup span of the selection
def test_hook_against_the_model(bctx, B):
    n_cases = 0
    for kind, make in KEY_KINDS.items():
        keys = make(B, 7 * B + len(kind))
        key_bytes = b"".join(bc.b32(k) for k in keys)
        floor = sorted(keys)[B // 3] if kind == "uniform" else 0  # the uniform keys: a floor that turns a third of the rows away
        for vname, verdicts in (("ok", [OK] * B), ("bad", [(VERIFY, FORMAT)[i % 2] for i in range(B)]), ("third", bc.verdicts_top_third_bad(keys, floor))):
            for tranche in (1, 4, 64):
                for K in sorted({0, 1, 3, B}):
                    what = (B, kind, vname, tranche, K)
                    want = bc.model(keys, verdicts, floor, K, tranche)
                    cap = 2 if (K == 0 and tranche == 4) else (K or B)  # one arm with less room than answers
                    got = bctx.debug_round_best(key_bytes, verdicts, floor, K, tranche, cap=cap, fill=FILL)
                    _check(got, want, cap, what)
                    n_cases += 1
                    if vname == "bad":  # everything is examined, in exactly the number of tranches the header's bound gives
                        T0 = max(tranche, K) if K else want[2]
                        t = bc.max_tranches(want[2], T0)
                        assert got.n_examined == got.n_candidates and got.n_best == 0, what
                        assert bc.examined_after(want[2], T0, t) == want[2] and (t == 0 or bc.examined_after(want[2], T0, t - 1) < want[2]), what
                    if vname == "ok" and K:
                        assert got.n_examined == min(max(tranche, K), got.n_candidates), what  # honest traffic: exactly T_0 rows
    assert n_cases == 4 * 3 * 3 * len({0, 1, 3, B})


def test_hook_default_tranche_and_floors(bctx, bbp):
    B = 300
    keys = bc.keys_edges(B, 5)
    kb = b"".join(bc.b32(k) for k in keys)
    bad = [VERIFY] * B
    got = bctx.debug_round_best(kb, [OK] * B, 0, 1, 0, fill=FILL)  # tranche 0: the default
    _check(got, bc.model(keys, [OK] * B, 0, 1, 0), 1, "default tranche")
    assert got.n_examined == bbp.BEST_TRANCHE_DEFAULT and keys[got.best[0]] == L - 1
    for floor in (L - 1, L, bc.ALL_ONES):  # l - 1 admits the two rows at l - 1; a floor >= l none, and a key >= l stays FORMAT
        got = bctx.debug_round_best(kb, bad, floor, 1, 1, fill=FILL)
        _check(got, bc.model(keys, bad, floor, 1, 1), 1, floor)
        assert got.n_candidates == (2 if floor == L - 1 else 0) and got.status.count(FORMAT) == 3


def test_hook_refuses_bad_input(bctx, bbp):
    one, n = bytes(32), ctypes.c_uint32()
    v = (ctypes.c_int32 * 1)(OK)
    out = (ctypes.c_int32 * 4)()
    r = ctypes.byref(n)
    h = bctx.handle
    lib = bbp.lib
    assert lib.bbp_debug_round_best(h, 1, one, v, one, 1, 1, 1, out, r, r, r, out) == OK
    assert lib.bbp_debug_round_best(h, 0, one, v, one, 1, 1, 1, out, r, r, r, out) == BAD_ARG
    assert lib.bbp_debug_round_best(h, bbp.SELECT_MAX_BIDS + 1, one, v, one, 1, 1, 1, out, r, r, r, out) == BAD_ARG
    for bad in (SKIPPED, 2, BAD_ARG):
        assert lib.bbp_debug_round_best(h, 1, one, (ctypes.c_int32 * 1)(bad), one, 1, 1, 1, out, r, r, r, out) == BAD_ARG
    for args in ((None, v, one, out, r, out), (one, None, one, out, r, out), (one, v, None, out, r, out), (one, v, one, None, r, out),
                 (one, v, one, out, None, out), (one, v, one, out, r, None)):
        k, vv, f, b, rr, s = args
        assert lib.bbp_debug_round_best(h, 1, k, vv, f, 1, 1, 1, b, rr, rr, rr, s) == BAD_ARG


# ---- proof-backed ------------------------------------------------------------------------------------------------------------------------
def _set_score(row, N, value):
    rs_ = 1121 + 32 * (4 + N)
    return row[:rs_] + bc.b32(value) + row[rs_ + 32:]


def _score(row, N):
    rs_ = 1121 + 32 * (4 + N)
    return int.from_bytes(row[rs_:rs_ + 32], "little")


def _tamper(row, N, kind):
    b = bytearray(row)
    if kind == "flip":        # a flipped record byte (t_x): VERIFY
        b[T_X] ^= 0x01
        return bytes(b)
    if kind == "top":         # a claimed score raised to l - 1: VERIFY, and the first row examined
        return _set_score(row, N, L - 1)
    if kind == "score_l":     # a score >= l: FORMAT, never examined
        return _set_score(row, N, _score(row, N) + L)
    if kind == "scalar_l":    # a non-canonical record scalar (t_x + l): FORMAT when examined
        b[T_X:T_X + 32] = (int.from_bytes(b[T_X:T_X + 32], "little") + L).to_bytes(32, "little")
        return bytes(b)
    raise KeyError(kind)


class Case:
    """B rows of one round laid out by repetition of at most 8 proved bids (so there are ties), some tampered; `verdicts` is what the
    existing bbp_verify_rounds says of every row."""

    def __init__(self, c, bbp, N, n_bids, B, tag, tamper):
        r = rc.honest(N, n_bids, tag)
        rows, _, st = c.prove_round(N, r.table, r.bid_bytes, rc.entropy(tag, n_bids, N))
        assert st == [OK] * n_bids
        size = bbp.round_row_size(N)
        base = [rows[size * i:size * (i + 1)] for i in range(n_bids)]
        self.N, self.B, self.size, self.table = N, B, size, r.table
        self.row_list = [base[i % n_bids] for i in range(B)]
        for i, kind in tamper.items():
            self.row_list[i] = _tamper(self.row_list[i], N, kind)
        self.rows = b"".join(self.row_list)
        self.keys = [_score(x, N) for x in self.row_list]
        self.verdicts = c.verify_rounds([N], self.table, None, self.rows)

    def want(self, floor, K, tranche):
        return bc.model(self.keys, self.verdicts, floor, K, tranche)


TAMPER37 = {0: "flip", 5: "top", 9: "score_l", 13: "scalar_l", 16: "flip", 21: "top", 30: "scalar_l", 36: "score_l"}


@pytest.fixture(scope="module", params=[1, 3])
def case37(request, bctx, bbp):
    N = request.param
    c = Case(bctx, bbp, N, 8, 37, 50 + N, TAMPER37)
    assert [c.verdicts[i] for i in sorted(TAMPER37)] == [VERIFY, VERIFY, FORMAT, FORMAT, VERIFY, VERIFY, FORMAT, FORMAT]
    assert c.verdicts.count(OK) == 37 - len(TAMPER37)
    return c


def _dev_form(c, bbp, case, floor, K, tranche, cap, offset=0, table=None):
    import torch
    buf = torch.frombuffer(bytearray(bytes(offset) + case.rows), dtype=torch.uint8).cuda()
    tab = torch.frombuffer(bytearray(table or case.table), dtype=torch.uint8).cuda()
    ent = torch.frombuffer(bytearray(random.Random(case.B + offset).randbytes(32 * case.B)), dtype=torch.uint8).cuda()
    status = torch.full((4 * case.B,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = c.verify_round_best_dev(case.N, tab.data_ptr(), case.B, buf.data_ptr() + offset, ent.data_ptr(), status.data_ptr(), floor, K, tranche, cap=cap,
                                  stream=s.cuda_stream, fill=FILL)
    s.synchronize()
    raw = bytes(status.cpu().numpy().tobytes())
    return got._replace(status=[int.from_bytes(raw[4 * i:4 * i + 4], "little", signed=True) for i in range(case.B)])


@pytest.mark.parametrize("K,tranche", [(1, 1), (1, 4), (3, 1), (3, 4), (0, 1), (37, 4)])
def test_both_forms_against_verify_rounds(bctx, bbp, case37, K, tranche):
    c = case37
    honest = sorted(k for k, v in zip(c.keys, c.verdicts) if v == OK)
    for floor in (0, honest[len(honest) // 2]):
        want = c.want(floor, K, tranche)
        cap = K or c.B
        _check(bctx.verify_round_best(c.N, c.table, c.rows, floor, K, tranche, fill=FILL), want, cap, ("host", floor))
        _check(_dev_form(bctx, bbp, c, floor, K, tranche, cap), want, cap, ("dev", floor))
    want = c.want(0, K, tranche)
    assert want[4][9] == FORMAT and want[4][36] == FORMAT                     # a score >= l: FORMAT, never examined
    assert want[4][5] == VERIFY and want[4][21] == VERIFY and want[3] >= 3       # the raised scores: examined first
    assert all(s == c.verdicts[i] or s == SKIPPED for i, s in enumerate(want[4]))


@pytest.mark.parametrize("offset", [1, 3])
def test_dev_form_rows_at_any_alignment(bctx, bbp, case37, offset):
    c = case37
    for K, tranche, cap in ((1, 1, 1), (3, 4, 2), (0, 1, c.B)):
        _check(_dev_form(bctx, bbp, c, 0, K, tranche, cap, offset=offset), c.want(0, K, tranche), cap, (offset, K))


def test_tranches_in_engine_calls_of_a_few_rows(bctx, bbp, case37, monkeypatch):
    """BBP_HOST_CHUNK_VERIFY (read at every call) cuts a tranche into engine calls: 37 candidates in parts of 5, both forms"""
    c = case37
    monkeypatch.setenv("BBP_HOST_CHUNK_VERIFY", "5")
    for K, tranche in ((0, 1), (3, 16)):
        want = c.want(0, K, tranche)
        _check(bctx.verify_round_best(c.N, c.table, c.rows, 0, K, tranche, fill=FILL), want, K or c.B, ("host", K))
        _check(_dev_form(bctx, bbp, c, 0, K, tranche, K or c.B, offset=1), want, K or c.B, ("dev", K))


def test_n202_rows_through_the_gather(bctx, bbp):
    """N = 202, B = 5: 7 777-byte rows at odd offsets; the top claim is forged, so a second tranche runs"""
    c = Case(bctx, bbp, 202, 3, 5, 61, {1: "top", 3: "flip"})
    assert c.size == 7777 and c.verdicts == [OK, VERIFY, OK, VERIFY, OK]
    want = c.want(0, 1, 1)
    assert want[3] == 3  # the forged top claim, then a tranche of two
    _check(bctx.verify_round_best(c.N, c.table, c.rows, 0, 1, 1, fill=FILL), want, 1, "host")
    for offset in (0, 1):
        _check(_dev_form(bctx, bbp, c, 0, 1, 1, 1, offset=offset), want, 1, ("dev", offset))
    _check(_dev_form(bctx, bbp, c, 0, 0, 1, 5, offset=3), c.want(0, 0, 1), 5, "dev, K = 0")


def test_non_canonical_seed(bctx, bbp, case37):
    c = case37
    table = bc.b32(int.from_bytes(c.table[:32], "little") + L) + c.table[32:]
    assert bctx.verify_rounds([c.N], table, None, c.rows) == [FORMAT] * c.B
    n_cand = sum(1 for k in c.keys if k < L)
    for got in (bctx.verify_round_best(c.N, table, c.rows, 0, 1, 4, fill=FILL), _dev_form(bctx, bbp, c, 0, 1, 4, 1, table=table)):
        assert (got.best, got.n_best, got.n_candidates, got.n_examined) == ([], 0, n_cand, n_cand)
        assert got.status == [FORMAT] * c.B and got.raw == [FILL_U32]


def test_settings_and_stats(bctx, bbp, case37):
    """entropy source DEVICE and verify mixing off change nothing; the combiner's counters are not disturbed"""
    c = case37
    want = c.want(0, 3, 4)
    sharing, batching = bctx.verify_round_sharing_stats(), bctx.batching_stats()
    try:
        bctx.set_entropy_source("device")
        bctx.set_verify_mixing(False)
        _check(bctx.verify_round_best(c.N, c.table, c.rows, 0, 3, 4, fill=FILL), want, 3, "device entropy, mixing off")
    finally:
        bctx.set_entropy_source("os")
        bctx.set_verify_mixing(True)
    assert bctx.verify_round_sharing_stats() == sharing and bctx.batching_stats() == batching


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
        assert lib.bbp_verify_round_best(h, N, one, B, one, one, 1, 1, 1, out, r, r, r, out) == rc_, (N, B)
        assert lib.bbp_verify_round_best_dev(h, N, p, B, p, p, one, 1, 1, 1, out, r, r, r, p, None) == rc_, (N, B)
    n.value = 7
    assert lib.bbp_verify_round_best(h, 8, one, 0, one, one, 1, 1, 1, out, r, r, r, out) == OK and n.value == 0  # B == 0: all counts zero
    n.value = 7
    assert lib.bbp_verify_round_best_dev(h, 8, p, 0, p, p, one, 1, 1, 1, out, r, r, r, p, None) == OK and n.value == 0
    assert lib.bbp_verify_round_best(h, 8, None, 1, one, one, 1, 1, 1, out, r, r, r, out) == BAD_ARG
    assert lib.bbp_verify_round_best(h, 8, one, 1, one, one, 1, 1, 1, None, r, r, r, out) == BAD_ARG   # best_out with cap > 0
    assert lib.bbp_verify_round_best_dev(h, 8, p, 1, p, None, one, 1, 1, 1, out, r, r, r, p, None) == BAD_ARG
    assert lib.bbp_verify_round_best_dev(h, 8, p, 1, p, p, one, 1, 1, 1, out, r, r, r, None, None) == BAD_ARG


def test_secret_wiping(bbp, ctx, case37):
    c = case37
    want = c.want(0, 3, 1)
    k = bbp.Context(0)
    try:
        plain = k.verify_round_best(c.N, c.table, c.rows, 0, 3, 1, fill=FILL)
        k.set_secret_wipe(True)
        got = k.verify_round_best(c.N, c.table, c.rows, 0, 3, 1, fill=FILL)
        assert got == plain
        _check(got, want, 3, "wiping on")
        _check(_dev_form(k, bbp, c, 0, 3, 1, 3, offset=1), want, 3, "wiping on, dev")
        assert k.debug_secret_residue()[:2] == (0, 0), k.debug_secret_residue()
        assert k.health() == 0
    finally:
        k.close()


def test_pool(bctx, bbp, case37):
    import torch
    c = case37
    pool = bbp.Pool([0, 0])
    try:
        for K, tranche in ((1, 1), (3, 4), (0, 1)):
            assert pool.verify_round_best(c.N, c.table, c.rows, 0, K, tranche, fill=FILL) == bctx.verify_round_best(c.N, c.table, c.rows, 0, K, tranche, fill=FILL)
            _check(pool.verify_round_best(c.N, c.table, c.rows, 0, K, tranche, fill=FILL), c.want(0, K, tranche), K or c.B, ("pool", K))
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = d.data_ptr()
        one, n = bytes(64), ctypes.c_uint32()
        r = ctypes.byref(n)
        out = (ctypes.c_int32 * 4)()
        assert bbp.lib.bbp_verify_round_best_dev(pool.handle, 8, p, 1, p, p, one, 1, 1, 1, out, r, r, r, p, None) == BAD_ARG
        assert bbp.lib.bbp_debug_round_best(pool.handle, 1, one, out, one, 1, 1, 1, out, r, r, r, out) == BAD_ARG
    finally:
        pool.close()
