"""GPU tier: one offer to many standings (include/bbp.h bbp_standings_offer, bbp_debug_standings_offer).  Hook-backed tests hold the shipped
kernels -- the many-rounds family's keys, ids, segments, selection, mark, settle and holders, and standings.h's seed, enter, displace,
merge, leave, plan and commit -- to the model of tests/standings_cases.py (S instances of the single standing's model) on made-up keys,
ids and verdicts, and to the shipped single-standing call on twin standings; proof-backed tests hold the host form to the model applied
to the statuses that bbp_verify_rounds returns.  A call that ends BBP_ERR_INTERNAL raises BbpError and fails its test."""
import ctypes
import random

import pytest

from tests import poison_cases as pc
from tests import prove_round_cases as rc
from tests import standings_cases as mc

sc = mc.sc
dc, bc = sc.dc, sc.bc
pytestmark = pytest.mark.gpu
OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, INTERNAL, SKIPPED, DUPLICATE = 0, 1, 2, 3, 4, 6, -1, -2
L = sc.L
FILL = 0x6E
FILL_U32 = int.from_bytes(bytes([FILL]) * 4, "little")
T_X = 257  # byte offset of t_x in a record: the version byte, then eight points
TABLE8 = bytes(32 * 9)  # a round of N = 8 for standings that only the hook is offered to (nothing is verified)


def _own_context(bbp):
    c = bbp.Context(0)
    yield c
    flags = c.health()
    c.close()
    assert flags == 0, "engine health flags %#x" % flags


@pytest.fixture(scope="module")
def sctx(ctx, bbp):
    """A context of this module's own (after `ctx`, so torch's HIP runtime is initialised first)."""
    yield from _own_context(bbp)


@pytest.fixture(scope="module")
def tctx(ctx, bbp):
    """... and one for the twin standings, which the shipped single-standing call is offered to: a handle holds 64 standings"""
    yield from _own_context(bbp)


def _kb(keys):
    return b"".join(bc.b32(k) for k in keys)


def _check(got, want, steps, status, cap, what):
    """a StandingsOffer against the model's (per standing [entered, ne, nc, nx, nd], n_steps, statuses)"""
    S = len(want)
    assert got.n_entered == [w[1] for w in want] and got.n_candidates == [w[2] for w in want], what
    assert got.n_examined == [w[3] for w in want] and got.n_duplicates == [w[4] for w in want], what
    assert got.entered == [w[0][:cap] for w in want] and got.n_steps == steps and got.status == status, what
    for s in range(S):  # entries at or beyond min(n_entered, cap) are not written
        assert got.raw[s][min(want[s][1], cap):] == [FILL_U32] * (cap - min(want[s][1], cap)), (what, s)
        assert want[s][3] + want[s][4] <= want[s][2]


def _check_read(c, h, entries, offered, what):
    got = c.standing_read(h)
    assert (got.n_entries, got.n_offered) == (len(entries), offered), what
    assert list(zip(got.scores, got.z_imgs, got.serials)) == [(bc.b32(k), i, s) for k, i, s in entries], what


class Group:
    """S open standings offered to in ONE call through the hook, the model beside them, and -- twins -- S standings opened alike on
    another context that the shipped single-standing hook is offered to, standing by standing"""

    def __init__(self, c, Ks, floors=None, twins=None):
        self.c, self.t, self.Ks = c, twins, Ks
        self.floors = floors or [0] * len(Ks)
        self.h = [c.standing_open(8, TABLE8, f, K) for K, f in zip(Ks, self.floors)]
        self.th = [twins.standing_open(8, TABLE8, f, K) for K, f in zip(Ks, self.floors)] if twins else None
        self.models = [sc.Standing(f, K) for K, f in zip(Ks, self.floors)]

    def offer(self, standing_of, keys, ids, verdicts, tranche, cap=None, what=None, wrap=lambda call: call()):
        S, B = len(self.h), len(keys)
        cap = B if cap is None else cap
        so = None if S == 1 and B % 2 else standing_of  # (one standing: standing_of may be NULL)
        got = wrap(lambda: self.c.debug_standings_offer(self.h, so, _kb(keys), b"".join(ids), verdicts, tranche, cap=cap, fill=FILL))
        want, steps, status = mc.offer(self.models, standing_of, keys, ids, verdicts, tranche)
        _check(got, want, steps, status, cap, what)
        for s in range(S):
            rows = [i for i in range(B) if standing_of[i] == s]
            _check_read(self.c, self.h[s], self.models[s].entries, self.models[s].offered, (what, s))
            if self.t:  # the shipped single call on the twin: every count, status and entry, and the same standing afterwards
                one = self.t.debug_standing_offer(self.th[s], _kb([keys[i] for i in rows]), b"".join(ids[i] for i in rows), [verdicts[i] for i in rows], tranche,
                                                  cap=cap, fill=FILL)
                assert [rows[j] for j in one.entered] == got.entered[s] and one.status == [got.status[i] for i in rows], (what, s)
                assert (one.n_entered, one.n_candidates, one.n_examined, one.n_duplicates) == (got.n_entered[s], got.n_candidates[s], got.n_examined[s],
                                                                                                got.n_duplicates[s]), (what, s)
                assert self.t.standing_read(self.th[s]) == self.c.standing_read(self.h[s]), (what, s)
        return got

    def close(self):
        for h in self.h:
            self.c.standing_close(h)
        for h in self.th or []:
            self.t.standing_close(h)


def _mixed_Ks(S):
    return [3] if S == 1 else [(3, 1, 1024)[s % 3] for s in range(S)]


def _hook_case(c, twins, S, B, wrap=lambda call: call()):
    """three offers in sequence with resends; rows interleaved over the standings, so a wavefront holds rows of several; K mixed within
    the call; the last standing receives no row in the first two offers"""
    rnd = random.Random(1000 * S + B)
    g = Group(c, _mixed_Ks(S), twins=twins)
    pool = [rnd.randbytes(32) for _ in range(max(2, B // 3))]  # shared by the standings: one z_img in several of them
    sent, n_dups, n_steps = [], 0, 0
    try:
        for n, (tranche, small) in enumerate(((1, False), (0, True), (4, False))):
            active = S if n == 2 or S == 1 else S - 1
            so = [(i + (S - 1 if n == 2 else n)) % active for i in range(B)]  # (the third offer's row 0 goes to the last standing)
            keys = [L + rnd.randrange(2) if rnd.random() < 0.02 else rnd.randrange(1, 1 << 10) for _ in range(B)]  # ties: the serial orders them
            ids = [rnd.choice(pool) for _ in range(B)]
            verdicts = [OK if rnd.random() < (0.5 if k > 700 else 0.85) else rnd.choice((VERIFY, FORMAT)) for k in keys]  # the top claims fail more often
            for j in range(B):
                if sent and rnd.random() < 0.3:  # a resend, mostly to the standing that saw the row before
                    s0, keys[j], ids[j], verdicts[j] = rnd.choice(sent)
                    so[j] = s0 if rnd.random() < 0.8 else so[j]
            if n == 2:
                so[0] = S - 1  # (whatever the resends did: the last standing is offered a row at last)
            sent += list(zip(so, keys, ids, verdicts))
            got = g.offer(so, keys, ids, verdicts, tranche, cap=2 if small else B, what=(S, B, n), wrap=wrap)
            n_dups += sum(got.n_duplicates)
            n_steps = max(n_steps, got.n_steps)
        assert S == 1 or g.models[S - 1].offered > 0
    finally:
        g.close()
    return n_dups, n_steps


# ---- 1. the hook against the model and against the shipped single call ----------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 64])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 130, 1000])
def test_hook_against_the_model_and_the_single_call(sctx, tctx, S, B):
    n_dups, n_steps = _hook_case(sctx, tctx, S, B)
    assert B < 63 or n_dups > 0  # the leave pass turned rows away as duplicates ...
    assert B < 63 or n_steps > 1 or (S, B) == (3, 1000) or (S == 64 and B < 130)  # ... and some standing ran more than one step


# ---- 2. one z_img offered to every standing enters every one ---------------------------------------------------------------------------
def test_one_z_img_in_every_standing(sctx):
    S = 64
    g = Group(sctx, _mixed_Ks(S))
    z = b"Z" * 32
    try:
        got = g.offer(list(range(S)), [500 + s for s in range(S)], [z] * S, [OK] * S, 0)
        assert got.n_entered == [1] * S and got.entered == [[s] for s in range(S)] and got.n_duplicates == [0] * S
        got = g.offer(list(range(S)) * 2, [500 + s for s in range(S)] + [400] * S, [z] * (2 * S), [OK] * (2 * S), 0)  # resent, and a lower copy
        assert got.n_entered == [0] * S and got.n_examined == [0] * S and set(got.status) <= {SKIPPED, DUPLICATE}
        assert all(m.entries == [(500 + s, z, 0)] for s, m in enumerate(g.models))
    finally:
        g.close()


# ---- 3. one identity of one standing on both sides of a 256-row boundary ---------------------------------------------------------------
@pytest.mark.parametrize("at", [251, 255])  # working rows 255 | 256 (sum K = 4 entry slots in front), and rows 255 | 256 of the call
def test_identity_on_both_sides_of_a_256_row_boundary(sctx, at):
    B = 520
    a, q, cc, x, f1, f2 = (bytes([n]) * 32 for n in range(1, 7))
    g = Group(sctx, [3, 1])
    try:
        g.offer([0, 0, 0, 1], [7000, 5400, 1800, 50], [a, q, cc, x], [OK] * 4, 1)
        so = [i % 2 for i in range(B)]
        keys = [2000 + i for i in range(B)]  # standing 0's fill: candidates that the bar turns away after the first step
        ids = dc.id_pool(B, B, 77)
        verdicts = [OK] * B
        for i, (s, k, z, v) in {0: (0, 9000, f1, VERIFY), 2: (0, 8000, f2, VERIFY), at: (0, 5500, x, OK), at + 1: (0, 5450, x, OK), 400: (0, 5300, x, OK),
                                1: (1, 5500, x, OK), at + 2: (1, 5450, x, OK)}.items():
            so[i], keys[i], ids[i], verdicts[i] = s, k, z, v
        # step 0 of standing 0 (T_0 = 3): two forged rows and the identity's first row, which enters above q; its copy just across the
        # boundary is above the bar and leaves as a DUPLICATE; the lower copy behind it is below the bar and stays SKIPPED
        got = g.offer(so, keys, ids, verdicts, 1, what=at)
        mine = [got.status[i] for i in range(B) if so[i] == 0]
        assert mine.count(DUPLICATE) == 1 and got.status[at] == OK and got.status[at + 1] == DUPLICATE and got.status[400] == SKIPPED
        assert got.n_duplicates[0] == 1 and got.entered[0] == [at] and [i for _, i, _ in g.models[0].entries] == [a, x, q]
    finally:
        g.close()


# ---- 4. atomic failure ------------------------------------------------------------------------------------------------------------------
def test_a_failure_in_one_standing_leaves_all_as_they_were(sctx, bbp):
    g = Group(sctx, [3, 3, 1])
    ids = dc.id_pool(60, 60, 5)
    try:
        g.offer([0, 1, 2, 0, 1], [50, 40, 30, 20, 10], ids[:5], [OK] * 5, 1)
        before = [sctx.standing_read(h) for h in g.h]
        assert [b.n_entries for b in before] == [2, 2, 1] and [b.n_offered for b in before] == [2, 2, 1]
        so = [i % 3 for i in range(45)]
        keys = [100 + i for i in range(45)]
        verdicts = [OK] * 45
        sctx.debug_standing_trip(g.h[1], 1)  # the flag word is raised behind the middle standing's first merge: no device fault is involved
        with pytest.raises(bbp.BbpError) as e:
            sctx.debug_standings_offer(g.h, so, _kb(keys), b"".join(ids[5:50]), verdicts, 1)
        assert e.value.status == INTERNAL
        assert [sctx.standing_read(h) for h in g.h] == before
        got = g.offer(so, keys, ids[5:50], verdicts, 1)  # the same call again: the trip is consumed, the model's outputs, serials go on
        assert got.n_entered == [3, 3, 1] and g.models[1].entries[0][2] == 2 + 14
    finally:
        g.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(sctx, bbp):
    lib, h = bbp.lib, sctx.handle
    g = Group(sctx, [2, 2, 2])
    g.offer([0, 1, 2], [9, 8, 7], dc.id_pool(3, 3, 1), [OK] * 3, 0)
    before = [sctx.standing_read(x) for x in g.h]
    n = ctypes.c_uint32(7)
    r = (ctypes.c_uint32 * 64)(*([7] * 64))
    u32s = lambda v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    hs, so, rows = u32s(g.h), u32s([0, 1, 2, 0]), bytes(4 * bbp.round_row_size(8))
    k4, out, ent = bytes(128), (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 12)()
    v = (ctypes.c_int32 * 4)(OK, OK, OK, VERIFY)
    top = bbp.SELECT_MAX_BIDS

    def public(S=3, handles=hs, B=4, of=so, rws=rows, cap=4, e=ent, counts=(r, r, r, r), steps=ctypes.byref(n), st=out):
        return lib.bbp_standings_offer(h, S, handles, B, of, rws, 0, cap, e, *counts, steps, st)

    def hook(S=3, handles=hs, B=4, of=so, keys=k4, ids=k4, vd=v, cap=4, e=ent, counts=(r, r, r, r), steps=ctypes.byref(n), st=out):
        return lib.bbp_debug_standings_offer(h, S, handles, B, of, keys, ids, vd, 0, cap, e, *counts, steps, st)

    try:
        for call in (public, hook):
            # a NULL pointer; entered_out may be NULL only when cap == 0, standing_of only when S == 1
            assert call(handles=None) == BAD_ARG and call(st=None) == BAD_ARG and call(e=None) == BAD_ARG and call(of=None) == BAD_ARG
            for k in range(4):
                assert call(counts=tuple(None if j == k else r for j in range(4))) == BAD_ARG
            # S; an unknown or closed handle; the same handle twice -- each before B is looked at
            assert call(S=0) == BAD_ARG and call(S=65, handles=u32s(list(range(65)))) == BAD_ARG
            for bad in (63, 64, 0xffffffff):
                assert call(handles=u32s([g.h[0], bad, g.h[2]]), B=0) == BAD_ARG
            assert call(handles=u32s([g.h[0], g.h[1], g.h[0]]), B=0) == BAD_ARG
            # B; standing_of
            assert call(B=top + 1) == BAD_ARG
            r[0] = r[1] = r[2] = 7
            n.value = 7
            assert call(B=0) == OK and list(r)[:3] == [0, 0, 0] and n.value == 0  # B == 0: zero counts, nothing changed
            assert call(of=u32s([0, 1, 3, 0])) == BAD_ARG
            assert [sctx.standing_read(x) for x in g.h] == before, call
        assert public(rws=None) == BAD_ARG and hook(keys=None) == BAD_ARG and hook(ids=None) == BAD_ARG and hook(vd=None) == BAD_ARG
        assert hook(vd=(ctypes.c_int32 * 4)(OK, OK, DUPLICATE, OK)) == BAD_ARG  # what bbp_debug_standing_offer refuses: a verdict outside the three
        assert hook(S=1, of=None, vd=(ctypes.c_int32 * 4)(OK, OK, 9, OK)) == BAD_ARG
        assert public(steps=None, B=0) == OK and hook(steps=None, cap=0, e=None, B=0) == OK  # n_steps may be NULL
        assert [sctx.standing_read(x) for x in g.h] == before
    finally:
        g.close()
    pool = bbp.Pool([0, 0])  # a pool refuses the hook
    try:
        ph = [pool.standing_open(8, TABLE8, 0, 2) for _ in range(2)]
        assert lib.bbp_debug_standings_offer(pool.handle, 2, u32s(ph), 4, u32s([0, 1, 0, 1]), k4, k4, v, 0, 4, ent, r, r, r, r, ctypes.byref(n), out) == BAD_ARG
        for x in ph:
            assert pool.standing_read(x).n_offered == 0
            pool.standing_close(x)
    finally:
        pool.close()


# ---- 6. the host form on real proofs ----------------------------------------------------------------------------------------------------
def _field(row, N, which):
    at = 1121 + 32 * (4 + N) + (32 if which == "z_img" else 0)
    return at, int.from_bytes(row[at:at + 32], "little")


def _set(row, N, which, value):
    at, _ = _field(row, N, which)
    return row[:at] + bc.b32(value) + row[at + 32:]


class Case:
    """As Case of tests/test_gpu_round_standing.py, for any N: six bids with distinct k, proved twice under different entropy, a
    byte-equal resend, and three rows that must not enter: a flipped record byte, the top identity's z_img under a forged higher score,
    z_img + l."""

    def __init__(self, c, bbp, N, tag):
        self.N = N
        r = rc.honest(N, 6, tag)
        size = self.size = bbp.round_row_size(N)
        proved = []
        for t in (tag, tag + 1):
            rows, _, st = c.prove_round(N, r.table, r.bid_bytes, rc.entropy(t, 6, N))
            assert st == [OK] * 6
            proved.append([rows[size * i:size * (i + 1)] for i in range(6)])
        first, again = proved
        assert all(a != b and a[-64:] == b[-64:] for a, b in zip(first, again))
        top = max(range(6), key=lambda i: _field(first[i], N, "score")[1])
        flipped = bytearray(again[(top + 1) % 6])
        flipped[T_X] ^= 0x01
        borrowed = _set(first[top], N, "score", L - 1)
        shifted = _set(first[(top + 2) % 6], N, "z_img", _field(first[(top + 2) % 6], N, "z_img")[1] + L)
        self.row_list = again[:3] + [borrowed] + first + again[3:] + [first[top], bytes(flipped), shifted]
        self.B = len(self.row_list)
        self.table = r.table
        self.keys = [_field(x, N, "score")[1] for x in self.row_list]
        self.ids = [x[-32:] for x in self.row_list]
        self.verdicts = c.verify_rounds([N], self.table, None, b"".join(self.row_list))
        assert self.verdicts.count(OK) == self.B - 3 and self.verdicts[3] == VERIFY and self.verdicts[-2:] == [VERIFY, FORMAT]


@pytest.fixture(scope="module")
def cases(sctx, bbp):
    """three standings over two values of N: standings 0 and 2 follow the round of N = 8 (each its own standing), standing 1 one of N = 6"""
    a, b = Case(sctx, bbp, 8, 71), Case(sctx, bbp, 6, 81)
    return [a, b, a]


def _host_form(c, cases, K, tranche, wrap=lambda call: call()):
    S, B1 = len(cases), cases[0].B
    h = [c.standing_open(x.N, x.table, 0, K) for x in cases]
    models = [sc.Standing(0, K) for _ in cases]
    bursts = (slice(0, 5), slice(5, 11), slice(11, B1), slice(0, B1))  # ... and a fourth burst that resends every row
    try:
        for sl in bursts:
            idx = [(s, j) for j in range(sl.start, sl.stop) for s in range(S)]  # interleaved: row j of every standing, then row j + 1
            so = [s for s, _ in idx]
            rows = b"".join(cases[s].row_list[j] for s, j in idx)
            got = wrap(lambda: c.standings_offer(h, [x.N for x in cases], so, rows, tranche, fill=FILL))
            want, steps, status = mc.offer(models, so, [cases[s].keys[j] for s, j in idx], [cases[s].ids[j] for s, j in idx],
                                           [cases[s].verdicts[j] for s, j in idx], tranche)
            _check(got, want, steps, status, len(idx), (K, tranche, sl))
            resend = sl.stop - sl.start == B1
            upto = B1 if resend else sl.stop
            for s, x in enumerate(cases):
                truth = sc.truth(x.keys[:upto], x.ids[:upto], x.verdicts[:upto], 0, K)
                assert [(k, i) for k, i, _ in models[s].entries] == [(k, i) for k, i, _ in truth]
                read = c.standing_read(h[s])
                assert (read.n_entries, read.n_offered, read.serials) == (len(models[s].entries), models[s].offered, [n for _, _, n in models[s].entries])
                every = x.row_list + x.row_list  # serial -> row: the first pass, then the resend
                assert read.scores == [every[n][-64:-32] for n in read.serials] and read.z_imgs == [every[n][-32:] for n in read.serials]
            if resend:  # only rows whose verdict is not OK are verified again; nothing enters
                assert got.n_entered == [0] * S
                assert all(st in (SKIPPED, DUPLICATE) for st, (s, j) in zip(got.status, idx) if cases[s].verdicts[j] == OK)
                assert sum(got.n_examined) == sum(1 for st in got.status if st not in (SKIPPED, DUPLICATE)) <= 3 * S
        assert all(len(m.entries) == min(K, 6) for m in models)
    finally:
        for x in h:
            c.standing_close(x)


@pytest.mark.parametrize("K,tranche", [(1, 1), (3, 0)])
def test_host_form_against_verify_rounds(sctx, cases, K, tranche):
    _host_form(sctx, cases, K, tranche)


def test_pool(sctx, bbp, cases):
    pool = bbp.Pool([0, 0])
    try:
        for K, tranche in ((1, 1), (3, 0)):
            _host_form(pool, cases, K, tranche)
    finally:
        pool.close()


# ---- 7. scratch discipline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", pc.WORDS)
def test_over_poisoned_scratch(sctx, cases, word):
    """cases 1 (S = 3, B = 130) and 6 with every scratch buffer of the context filled before each call under test: the standings' own
    entries are exempt and persist (csrc/secret_map.h), everything the call works in is not"""
    def poisoned(call):
        with pc.Poisoned(sctx, word):
            return call()

    for _ in range(pc.WARM_CALLS):  # the calls under test themselves, to standings that are closed again
        _hook_case(sctx, None, 3, 130)
    _hook_case(sctx, None, 3, 130, wrap=poisoned)
    for _ in range(pc.WARM_CALLS):
        _host_form(sctx, cases, 3, 0)
    _host_form(sctx, cases, 3, 0, wrap=poisoned)
