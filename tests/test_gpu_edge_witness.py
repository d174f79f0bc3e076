"""GPU tier of the edge-witness cases (tests/edge_witness_cases.py; the CPU tier, tests/test_edge_witness_host.py, shows that the C
oracle proves and accepts every case and that each holds the edge it is named for).  The shipped prover and verifier kernels see what
the hash-stream witnesses of every other test never are: commitments that are the identity (32 zero bytes in the record), the values
0, 1 and l - 1 through the commitment comb, blindings that are not reduced, a score of zero, lists whose items are all equal.  Every
comparison is byte or status equality with the C oracle, or with the big-int oracle's records in tests/golden/proofs_edge.json."""
import os

import pytest

from oracle.ref_py import ristretto as rs
from tests import edge_witness_cases as ew
from tests import forgery_cases as fc
from tests import oracle_c
from tests import prove_round_cases as rc
from tests import round_best_cases as bc
from tests import round_select_cases as sc
from tests.test_gpu_prove_verify import _synth_batch

pytestmark = pytest.mark.gpu
OK, VERIFY, FORMAT, BAD_ARG, SKIPPED = 0, 1, 3, 4, -1
L = ew.L
THREADS = 8


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def ectx(ctx, bbp):
    """A context of this module's own: checking is switched on and off here (after `ctx`, so torch's HIP runtime is initialised first)."""
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def enc_B(golden):
    return bytes.fromhex(golden("setup_kat.json")["B"])


class Batch:
    """Rows of one list length, edge rows (a row of the case table) and ordinary ones (None: the next row of _synth_batch) in the
    given order, with the C oracle's records."""

    def __init__(self, ctx, oc, N, pattern, seed):
        n_ord = sum(1 for p in pattern if p is None)
        ins, ents, vins = _synth_batch(ctx, n_ord, N, seed=seed) if n_ord else ([], [], [])
        self.N, self.B = N, len(pattern)
        self.names, self.ins, self.ents, self.tails = [], [], [], []
        k = 0
        for p in pattern:
            if p is None:
                self.names.append("ordinary %d" % k)
                self.ins.append(ins[k])
                self.ents.append(ents[k])
                self.tails.append(b"".join(vins[k]))
                k += 1
            else:
                self.names.append(p["name"])
                self.ins.append(ew.prove_row(p))
                self.ents.append(p["ent"])
                self.tails.append(ew.tail(p))
        self.inputs, self.entropy = b"".join(self.ins), b"".join(self.ents)
        self.records, st = oc.prove_many(self.inputs, self.entropy, self.B, N, threads=THREADS)
        assert st == [OK] * self.B
        self.size = len(self.records) // self.B

    def record(self, i, blob=None):
        return (self.records if blob is None else blob)[self.size * i:self.size * (i + 1)]

    def check(self, out, st, what=""):
        assert st == [OK] * self.B, (what, [(n, s) for n, s in zip(self.names, st) if s])
        bad = [n for i, n in enumerate(self.names) if self.record(i, out) != self.record(i)]
        assert not bad, "%s records differ from the oracle's: %s" % (what, bad)

    def verify_rows(self):
        return b"".join(self.record(i) + self.tails[i] for i in range(self.B))


def _alternate(rows):
    return [p for r in rows for p in (r, None)]


@pytest.fixture(scope="module")
def mixed3(ctx, oc):
    """Every N = 3 row of the table, each followed by an ordinary row: 18 rows, edge and ordinary lanes in one wavefront."""
    b = Batch(ctx, oc, 3, _alternate(ew.all_rows(oc, 3)), seed=20261)
    assert b.B == 18 and b.names[0] == "zero" and b.names[1] == "ordinary 0"
    return b


def test_witness_kernel_at_the_edges(ctx, oc):
    rows = [ew.b32(d) + ew.b32(k) + ew.b32(s) for d in (0, 1, 2**64 - 1, 2**64, L - 1) for k in (0, 1, L - 1, ew.P7778) for s in (0, 1, L - 1)]
    assert len(rows) == 60
    out = ctx.witness_batch(b"".join(rows))
    for i, r in enumerate(rows):
        assert out[192 * i:192 * i + 192] == oc.witness(r), (i, r.hex())


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_prove_matches_the_edge_golden_bytes(ctx, golden, idx):
    """Big-int oracle == device (the CPU tier holds the C oracle to the same file): record and Fiat-Shamir challenges."""
    c = golden("proofs_edge.json")["edge"][idx]
    assert (c["case"], c["N"], c["toggle"]) == ew.GOLDEN[idx]
    s7 = b"".join(bytes.fromhex(c[k]) for k in ["d", "k", "y", "y_inv", "q", "z_img", "seed"])
    pub = b"".join(bytes.fromhex(p) for p in c["pub_list"])
    rec = ctx.prove(s7, pub, c["toggle"], bytes.fromhex(c["entropy"]))
    ch = ctx.debug_challenges(1, c["N"], 0)
    for k in ["y", "z", "u", "x", "w"]:
        assert ch[k] == c["trace"][k], k
    assert [ch["t%d" % i] for i in range(1, 7)] == c["trace"]["t_coeffs"]
    assert rec.hex() == c["record"]
    assert ctx.verify(rec, bytes.fromhex(c["q"]), bytes.fromhex(c["z_img"]), bytes.fromhex(c["seed"]), pub) == OK


def test_mixed_batch_n3(ectx, mixed3):
    out, st = ectx.prove_batch(mixed3.B, 3, mixed3.inputs, mixed3.entropy)
    mixed3.check(out, st)
    assert ectx.verify_batch(mixed3.B, 3, mixed3.verify_rows()) == [OK] * mixed3.B


@pytest.mark.parametrize("N,shape", [(8, "eoeo"), (1, "e"), (1, "oeo"), (202, "e")])
def test_mixed_batch_other_list_lengths(ectx, ctx, oc, N, shape):
    edge = ew.all_rows(oc, N)
    pattern = [edge[sum(1 for s in shape[:i] if s == "e") % len(edge)] if ch == "e" else None for i, ch in enumerate(shape)]
    assert {p["name"] for p in pattern if p} == {r["name"] for r in edge}
    b = Batch(ctx, oc, N, pattern, seed=20262 + N)
    out, st = ectx.prove_batch(b.B, N, b.inputs, b.entropy)
    b.check(out, st, (N, shape))
    assert ectx.verify_batch(b.B, N, b.verify_rows()) == [OK] * b.B


@pytest.mark.parametrize("knob,value", [("BBP_COMMIT_SPLIT_BELOW", "0"), ("BBP_WITNESS_NATIVE", "0"), ("BBP_MSM_SMALL", "0"), ("BBP_TAIL_ROUND", "12"),
                                        ("BBP_RNG_COOP", "0"), ("BBP_TR_WAVE_BELOW", "0"), ("BBP_TAIL_SMALL_BELOW", "0"), ("BBP_FOLD_HALF_FROM", "1")])
def test_paths_give_the_same_bytes(bbp, mixed3, knob, value):
    """The one-lane comb, the interpreted gates, the 1024-bucket MSM kernels, the all-MSM IPA, the one-lane rng chain and transcript,
    the folded-generator tail and the half-wavefront fold, each on a context of its own, over the mixed N = 3 batch."""
    old = os.environ.get(knob)
    os.environ[knob] = value
    try:
        c2 = bbp.Context(0)
    finally:
        if old is None:
            os.environ.pop(knob, None)
        else:
            os.environ[knob] = old
    try:
        out, st = c2.prove_batch(mixed3.B, 3, mixed3.inputs, mixed3.entropy)
        mixed3.check(out, st, knob)
        assert c2.health() == 0
    finally:
        c2.close()


def test_checked_proving_returns_the_same_bytes_and_reproves_nothing(ectx, mixed3):
    n0 = ectx.prove_check_stats()
    ectx.set_prove_check(True)
    try:
        out, st = ectx.prove_batch(mixed3.B, 3, mixed3.inputs, mixed3.entropy)
    finally:
        ectx.set_prove_check(False)
    n1 = ectx.prove_check_stats()
    mixed3.check(out, st, "checked")
    assert n1[0] - n0[0] == mixed3.B and n1[1:] == n0[1:]  # every row checked; none refused, none proved again
    assert ectx.health() == 0


# ---- verifiers ------------------------------------------------------------------------------------------------------------------------------
def _vrow(r, record, t=None):
    """(record, score, z_img, seed, pub_list): a row of tests/forgery_cases.py"""
    t = ew.tail(r) if t is None else t
    return (record, t[:32], t[32:64], t[64:96], t[96:])


class VCases:
    """Per list length: the oracle's record of every edge row, then the tampered copies of each, with the oracle's status of every row
    and whether an aggregated verifier rejects it before its group's sum."""

    def __init__(self, oc, enc_B):
        self.labels, self.rows, self.exp, self.early, self.n_valid = {}, {}, {}, {}, {}
        for N in (1, 3, 8, 202):
            edge = ew.all_rows(oc, N)
            recs, st = oc.prove_many(b"".join(ew.prove_row(r) for r in edge), b"".join(r["ent"] for r in edge), len(edge), N, threads=THREADS)
            assert st == [OK] * len(edge)
            size = len(recs) // len(edge)
            recs = [recs[size * i:size * (i + 1)] for i in range(len(edge))]
            labels = [r["name"] for r in edge]
            rows = [_vrow(r, rec) for r, rec in zip(edge, recs)]
            base = list(rows)
            for r, rec in zip(edge, recs):
                for label, rec2, t in ew.tampered(r, rec, enc_B):
                    labels.append("%s: %s" % (r["name"], label))
                    rows.append(_vrow(r, rec2, t))
                    base.append(_vrow(r, rec))
            exp = oc.verify_many(b"".join(fc.join(x) for x in rows), len(rows), N, threads=THREADS)
            assert exp[:len(edge)] == [OK] * len(edge) and OK not in exp[len(edge):], N
            self.labels[N], self.rows[N], self.exp[N], self.n_valid[N] = labels, rows, exp, len(edge)
            self.early[N] = [fc.rejected_before_the_sum(x, s, rs.decode, b) for x, s, b in zip(rows, exp, base)]

    def blob(self, N, idx=None):
        return b"".join(fc.join(self.rows[N][i]) for i in (range(len(self.rows[N])) if idx is None else idx))

    def diff(self, N, got, idx=None):
        idx = list(range(len(self.rows[N]))) if idx is None else idx
        return [(self.labels[N][i], g, self.exp[N][i]) for g, i in zip(got, idx) if g != self.exp[N][i]]


@pytest.fixture(scope="module")
def vcases(oc, enc_B):
    return VCases(oc, enc_B)


@pytest.mark.parametrize("N", [1, 3, 8, 202])
def test_plain_and_aggregated_verifiers_match_the_oracle(ectx, vcases, N):
    B, blob, exp, early = len(vcases.rows[N]), vcases.blob(N), vcases.exp[N], vcases.early[N]
    valid = list(range(vcases.n_valid[N]))
    assert ectx.verify_batch(len(valid), N, vcases.blob(N, valid)) == [OK] * len(valid)
    assert not vcases.diff(N, ectx.verify_batch(B, N, blob))
    for group in (0, 7):
        got, nfb = ectx.verify_batch_aggregated(len(valid), N, vcases.blob(N, valid), group)
        assert got == [OK] * len(valid) and nfb == 0, group                        # identity commitments pass the group check
        got, nfb = ectx.verify_batch_aggregated(B, N, blob, group)
        assert not vcases.diff(N, got), group
        assert nfb == fc.expected_fallback(exp, early, group or 32), group
    assert ectx.health() == 0


def test_one_tampered_row_among_untampered_edge_rows_of_its_group(ectx, vcases):
    """Nine valid edge rows and one tampered copy in one group: the group check fails, the per-proof pass gives each row its verdict."""
    N = 3
    labels = vcases.labels[N]
    for what in ("zero: V2 = identity", "zero: V0 = B", "zero: score = 1", "zero_blind: V4 = B"):
        idx = list(range(vcases.n_valid[N]))
        idx.insert(4, labels.index(what))
        assert not vcases.early[N][idx[4]] and vcases.exp[N][idx[4]] == VERIFY
        for group in (0, 7):
            got, nfb = ectx.verify_batch_aggregated(len(idx), N, vcases.blob(N, idx), group)
            assert not vcases.diff(N, got, idx), (what, group)
            assert got == [OK] * 4 + [VERIFY] + [OK] * 5 and nfb == (10 if group == 0 else 7), (what, group)
    idx = list(range(vcases.n_valid[N]))
    idx.insert(4, labels.index("zero: V4 bit0"))                                  # not an encoding: decided before the sum, no fallback
    got, nfb = ectx.verify_batch_aggregated(len(idx), N, vcases.blob(N, idx), 0)
    assert got == [OK] * 4 + [VERIFY] + [OK] * 5 and nfb == 0


def test_mixed_aggregated_verifier_over_three_list_lengths(ectx, bbp, vcases):
    order = []
    for k in range(max(len(vcases.rows[n]) for n in (1, 3, 8))):
        order += [(n, k) for n in (1, 3, 8) if k < len(vcases.rows[n])]
    rows = [vcases.rows[n][k] for n, k in order]
    exp = [vcases.exp[n][k] for n, k in order]
    early = [vcases.early[n][k] for n, k in order]
    Ns, blob = bbp.pack_mixed_rows(rows)
    assert Ns[:3] == [1, 3, 8]
    got = ectx.verify_batch_mixed(Ns, blob)
    assert got == exp, [(vcases.labels[n][k], g, e) for (n, k), g, e in zip(order, got, exp) if g != e]
    for group in (0, 7):
        got, nfb = ectx.verify_batch_mixed_aggregated(Ns, blob, group)
        assert got == exp, (group, [(vcases.labels[n][k], g, e) for (n, k), g, e in zip(order, got, exp) if g != e])
        assert nfb == fc.expected_fallback(exp, early, group or 32), group
    assert ectx.health() == 0


def test_round_verifiers_group_the_rows_that_share_seed_and_list(ectx, bbp, vcases):
    """Every edge row's (seed, list) is a round; its rows are the valid record and its tampered copies (a tampered score is a row's)."""
    rounds, round_of, rows, exp, early, labels = [], [], [], [], [], []
    for N in (3, 1, 8, 202):
        index = {}
        for x, e, ea, lab in zip(vcases.rows[N], vcases.exp[N], vcases.early[N], vcases.labels[N]):
            key = (x[3], x[4])
            if key not in index:
                index[key] = len(rounds)
                rounds.append(key)
            round_of.append(index[key])
            rows.append(x[0] + x[1] + x[2])
            exp.append(e)
            early.append(ea)
            labels.append(lab)
    round_Ns, table = bbp.pack_rounds(rounds)
    assert len(rounds) == 13 and len(rows) > 2 * len(rounds)
    got = ectx.verify_rounds(round_Ns, table, round_of, b"".join(rows))
    assert got == exp, [(l, g, e) for l, g, e in zip(labels, got, exp) if g != e]
    for group in (0, 7):
        got, nfb = ectx.verify_rounds_aggregated(round_Ns, table, round_of, b"".join(rows), group)
        assert got == exp, (group, [(l, g, e) for l, g, e in zip(labels, got, exp) if g != e])
        assert nfb == fc.expected_fallback(exp, early, group or 32), group
    pick = [i for i, l in enumerate(labels) if l.startswith("same_items")]
    r = rounds[round_of[pick[0]]]
    assert len(pick) > 3 and len(set(r[1][32 * j:32 * j + 32] for j in range(8))) == 1
    assert ectx.verify_round(8, r[0], r[1], b"".join(rows[i] for i in pick)) == [exp[i] for i in pick] == [OK] + [VERIFY] * (len(pick) - 1)
    assert ectx.health() == 0


# ---- rounds from raw bids -------------------------------------------------------------------------------------------------------------------
def _w(oc, d, k, seed):
    w = oc.witness(ew.b32(d) + ew.b32(k) + ew.b32(seed))
    return dict(zip(("m", "x", "y", "y_inv", "q", "z_img"), (ew.sc(w[32 * j:32 * j + 32]) for j in range(6))))


def _round(oc, N, seed, bids, items, tag):
    """items: per list index a bid's index (its x), None (an item from the stream) or 32 bytes.  A bid whose x is in no item is refused
    (BAD_ARG); an accepted one has the LOWEST matching index as its toggle."""
    ws = [_w(oc, d, k, seed) for d, k in bids]
    lst = [ew.b32(ws[it]["x"]) if isinstance(it, int) else it if it is not None else ew.b32(ew._scalar("round%d" % tag, j, b"item"))
           for j, it in enumerate(items)]
    assert len(lst) == N
    expect = []
    for w in ws:
        at = [j for j, it in enumerate(lst) if fc.bits_value(it) == w["x"]]
        expect.append((OK, at[0], w) if at else (BAD_ARG, 0, None))
    return rc.Round(N, ew.b32(seed), lst, bids, expect)


def _round_entropy(r, tag, zero_rows=()):
    es = 32 * (4 + r.N) + 32
    ent = rc.entropy(tag, r.B, r.N)
    return b"".join(bytes(es) if i in zero_rows else ent[es * i:es * (i + 1)] for i in range(r.B))


def _oracle_rows(oc, r, ent):
    recs, st = oc.prove_many(r.in_rows(), ent, r.B, r.N, threads=THREADS)
    assert all(s == OK for s, want in zip(st, r.status) if want == OK)
    return r.rows(recs)


ORD = [(0x1D2C3B4A59687766, 3**150 % L), (77, L - 2), (2**63 + 5, 2**200 + 9), (2**40, 12345), (99991, 5**100 % L)]


@pytest.mark.parametrize("which", ["seed0", "seed_l-1", "all_items_x"])
def test_prove_round_at_the_edges(ectx, oc, bbp, which):
    if which == "seed0":      # the d = 0, k = 0 bid under zero entropy: V_0, V_1 and both untoggled bits are the identity
        r = _round(oc, 3, 0, [(0, 0), ORD[0]], [1, None, 0], 1)
        ent, want_toggles = _round_entropy(r, 41, zero_rows=(0,)), [2, 0]
    elif which == "seed_l-1":
        r = _round(oc, 3, L - 1, [(0, 0), (2**64 - 1, L - 1), (1, 1)], [2, 1, 0], 2)
        ent, want_toggles = _round_entropy(r, 42), [2, 1, 0]
    else:                     # every item is bid 0's x: the lowest index; bid 1 is in no item
        r = _round(oc, 8, ORD[1][1], [ORD[2], ORD[3]], [0] * 8, 3)
        ent, want_toggles = _round_entropy(r, 43, zero_rows=(0,)), [0, 0]
        assert r.status == [OK, BAD_ARG]
    assert r.toggles == want_toggles
    rows, toggles, st = ectx.prove_round(r.N, r.table, r.bid_bytes, ent)
    assert (st, toggles) == (r.status, r.toggles)
    want = _oracle_rows(oc, r, ent)
    row = bbp.round_row_size(r.N)
    assert [i for i in range(r.B) if rows[row * i:row * (i + 1)] != want[row * i:row * (i + 1)]] == []
    ok = [i for i in range(r.B) if r.status[i] == OK]
    assert ectx.verify_round(r.N, r.seed, b"".join(r.items), b"".join(rows[row * i:row * (i + 1)] for i in ok)) == [OK] * len(ok)
    if which == "seed0":
        assert ew.identity_slots(rows[:bbp.record_size(3)], 3) == {0, 1, 4, 5} and rows[bbp.record_size(3):bbp.record_size(3) + 32] == bytes(32)
    assert ectx.health() == 0


@pytest.fixture(scope="module")
def score_round(oc):
    """N = 8, six bids: bid 2 has d = 0 (score zero), bid 4 is in no item, the others are ordinary."""
    bids = [ORD[0], ORD[1], (0, 7**90 % L), ORD[2], ORD[3], ORD[4]]
    r = _round(oc, 8, 11**70 % L, bids, [5, None, 3, 2, None, 1, 0, None], 4)
    assert r.status == [OK, OK, OK, OK, BAD_ARG, OK] and r.expect[2][2]["q"] == 0
    return r


@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("K", [0, 2, 5])
def test_select_with_a_zero_score(ectx, oc, bbp, score_round, floor, K):
    """include/bbp.h: Q = { i : status[i] == OK and score[i] >= floor } -- floor 0 admits the zero score, floor 1 does not."""
    r = score_round
    scores = [e[2]["q"] if e[0] == OK else 0 for e in r.expect]
    want_sel, n_sel, n_q = sc.model(scores, r.status, floor, K)
    assert n_q == (5 if floor == 0 else 4) and (2 in want_sel) == (floor == 0 and K in (0, 5))
    ent = _round_entropy(rc.subset(r, want_sel), 50 + K, zero_rows=(want_sel.index(2),) if 2 in want_sel else ())
    got = ectx.prove_round_select(r.N, r.table, r.bid_bytes, floor, K, cap=len(want_sel), entropy=ent, want_scores=True)
    assert (got.sel, got.n_sel, got.n_qualified) == (want_sel, n_sel, n_q)
    assert got.status == r.status and got.scores == b"".join(ew.b32(s) for s in scores)
    sub = rc.subset(r, want_sel)
    assert got.toggles == sub.toggles and got.rows == _oracle_rows(oc, sub, ent)
    assert ectx.verify_round(r.N, r.seed, b"".join(r.items), got.rows) == [OK] * n_sel
    assert ectx.health() == 0


def test_round_best_with_a_zero_score(ectx, oc, bbp, score_round):
    """The score-0 record among the rows of bbp_verify_round_best, K = 2: with the four highest claims forged the walk reaches it, and
    it is the second best at floor 0 and below the floor at floor 1."""
    r = rc.subset(score_round, [0, 1, 2, 3, 5])
    ent = _round_entropy(r, 60, zero_rows=(2,))
    row, rs_ = bbp.round_row_size(8), bbp.record_size(8)
    packed = _oracle_rows(oc, r, ent)
    rows = [bytearray(packed[row * i:row * (i + 1)]) for i in range(r.B)]
    keys = [e[2]["q"] for e in r.expect]
    assert keys[2] == 0 and ew.identity_slots(bytes(rows[2][:rs_]), 8) == {0} | {4 + j for j in range(8) if j != r.toggles[2]}
    by_score = sorted(range(r.B), key=lambda i: -keys[i])
    assert by_score[-1] == 2
    for i in by_score[:3]:
        rows[i][257] ^= 1  # t_x
    blob = b"".join(bytes(x) for x in rows)
    verdicts = oc.verify_many(b"".join(bytes(x) + r.table for x in rows), r.B, 8, threads=THREADS)
    assert verdicts == [VERIFY if i in by_score[:3] else OK for i in range(r.B)]
    assert ectx.verify_round(8, r.seed, b"".join(r.items), blob) == verdicts
    for floor, K, tranche in ((0, 2, 1), (1, 2, 1), (0, 0, 0), (0, 1, 1), (0, 5, 0)):
        best, n_best, n_cand, n_exam, status = bc.model(keys, verdicts, floor, K, tranche)
        got = ectx.verify_round_best(8, r.table, blob, floor, K, tranche)
        assert (got.best, got.n_best, got.n_candidates, got.n_examined, got.status) == (best, n_best, n_cand, n_exam, status), (floor, K, tranche)
    best = bc.model(keys, verdicts, 0, 2, 1)
    assert best[0] == [by_score[3], 2] and best[3] == 5                       # the zero score is reached and ranks second
    best = bc.model(keys, verdicts, 1, 2, 1)
    assert best[0] == [by_score[3]] and best[4][2] == SKIPPED and best[2] == 4  # below the floor: not a candidate
    assert ectx.health() == 0
