"""Rows, launches and expected outputs for the SHIPPED variable-base kernels of the verifier (csrc/verifier.inc k_varbase, k_varprep +
k_varsum; csrc/verifier_mixed.inc k_varbase_mx, k_varprep_mx + k_varsum_mx), run through bbp_debug_varbase by
tests/test_gpu_varbase_kernels.py.  tests/test_varbase_cases_host.py asserts the ledger over what is built here, without a GPU and
without the oracle, so that the battery cannot quietly lose an edge.

A row is one verification's variable-base part: np = 6 + m + 5 + 22 point slots (m = 4 + N) and the scalars the kernels derive the
slots' scalars from.  The scalar of slot k, as the kernels' algebra gives it:

    0..2      x, x^2, x^3
    3..5      the same times u          (a one-phase row skips these slots: active index a >= 3 is slot a + 3)
    6..5+m    wv[k - 6] r x^2
    next 5    r x^e, e = 1, 3, 4, 5, 6
    next 11   u_j^2
    last 11   (u_j^-1)^2                (an input of its own: the kernels do not relate it to u_j)
    with agg  everything times rho

The expected sum of a row is sum s_k P_k over its active slots whose point decodes, from oracle/ref_py/ristretto.py; k_varbase's lane
q of Q owns the active indices q, q + Q, ..  Arbitrary digit strings travel through the wv slots with x = r = 1: the whole scalar
battery of tests/scalarmul_cases.py, on the points its own items put them on (one oracle product serves both files), and every nibble
at every digit position.  Most other slots carry the scalar 1, which costs the oracle one addition.  The digits are those of the
offset recoding: sp = s + 0x88..8, digit j = nibble_j(sp) - 8."""
import collections
import functools
import random
import time

from oracle.ref_py import ristretto as rs
from tests import scalarmul_cases as sm

L = rs.L
OK, ERR_VERIFY = 0, 1  # BBP_OK, BBP_ERR_VERIFY
LANES, PREP_SUM, MX_LANES, MX_PREP_SUM = 0, 1, 2, 3  # bbp_debug_varbase forms
FORM_NAMES = {LANES: "k_varbase", PREP_SUM: "k_varprep+k_varsum", MX_LANES: "k_varbase_mx", MX_PREP_SUM: "k_varprep_mx+k_varsum_mx"}
ZERO_DIGITS = [0x88888888] * 8  # all 64 digits zero
UNWRITTEN = [0] * 8             # a slot no kernel touched (bbp_debug_varbase zeroes the digit buffer)
QS = (1, 2, 7, 64)
Q_BEYOND = 300                  # more lanes than any row has active points (at most 239)
BS = (1, 2, 3, 5)
NS = (1, 8, 202)
CLASSES = ("A1", "A2", "wv", "T", "L", "R")


def n_points(n):
    return 6 + (4 + n) + 5 + 22


# ---- points: sm.points() by index, then encodings that do not decode ----------------------------------------------------------
N_GOOD = len(sm.points())  # 0 the identity, 1 the basepoint, 2.., sm.NEG2 = -points[2]


def _first_even_off_curve():
    s = 2
    while rs.decode(s.to_bytes(32, "little")) is not None:
        s += 2
    return s


BAD_ENCODINGS = [
    (1).to_bytes(32, "little"),                         # negative (odd)
    (rs.P + 1).to_bytes(32, "little"),                  # not canonical: >= p
    ((1 << 255) | 2).to_bytes(32, "little"),            # bit 255 set
    _first_even_off_curve().to_bytes(32, "little"),     # canonical and even, not on the curve
]
BAD0 = N_GOOD  # point index of BAD_ENCODINGS[0]
assert all(rs.decode(e) is None for e in BAD_ENCODINGS)


def encoding(i):
    return sm.encodings()[i] if i < N_GOOD else BAD_ENCODINGS[i - N_GOOD]


def decodes(i):
    return i < N_GOOD


# ---- the model -----------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "name n ver pidx x r u rho wv uj uji")
Launch = collections.namedtuple("Launch", "name group rows Q agg")  # rows: indices into rows()


def slot_class(n, k):
    m = 4 + n
    return "A1" if k < 3 else "A2" if k < 6 else "wv" if k < 6 + m else "T" if k < 11 + m else "L" if k < 22 + m else "R"


def slot_scalar(row, k, agg):
    m, x, r = 4 + row.n, row.x, row.r
    if k < 6:
        s = pow(x, k % 3 + 1, L)
        if k >= 3:
            s = s * row.u % L
    elif k < 6 + m:
        s = row.wv[k - 6] * r * x * x % L
    elif k < 11 + m:
        s = r * pow(x, (1, 3, 4, 5, 6)[k - 6 - m], L) % L
    elif k < 22 + m:
        s = pow(row.uj[k - 11 - m], 2, L)
    else:
        s = pow(row.uji[k - 22 - m], 2, L)
    return s * row.rho % L if agg else s


def active_slots(row):
    """slot of every active index a, in order: what `k = (one_phase && a >= 3) ? a + 3 : a` must give"""
    return [0, 1, 2] + ([3, 4, 5] if row.ver else []) + list(range(6, n_points(row.n)))


def lane_share(row, Q, q):
    return active_slots(row)[q::Q]


def is_uniform(launch):
    rr = [rows()[i] for i in launch.rows]
    return len({(r.n, r.ver) for r in rr}) == 1


def forms_of(launch):
    return (LANES, PREP_SUM, MX_LANES, MX_PREP_SUM) if is_uniform(launch) else (MX_LANES, MX_PREP_SUM)


@functools.lru_cache(maxsize=None)
def expected(ri, agg):
    """(status, digit words per slot, terms) of row ri; terms: [(slot, scalar, point index)] of the active slots whose point decodes"""
    row = rows()[ri]
    digits = [UNWRITTEN] * n_points(row.n)
    status, terms = OK, []
    for k in active_slots(row):
        if not decodes(row.pidx[k]):
            status, digits[k] = ERR_VERIFY, ZERO_DIGITS
            continue
        s = slot_scalar(row, k, agg)
        digits[k] = sm.offset_words(s)[0]
        terms.append((k, s, row.pidx[k]))
    return status, digits, terms


ORACLE_SECONDS = [0.0]  # time spent in the oracle's scalar multiplications and encodings, for the report


def product(s, i):
    if s == 0:
        return rs.IDENT
    if s == 1:
        return sm.points()[i]
    t = time.perf_counter()
    p = sm.pt_mul(s, i)  # cached, and shared with the scalar-multiplication tests
    ORACLE_SECONDS[0] += time.perf_counter() - t
    return p


@functools.lru_cache(maxsize=None)
def _encode(p):
    t = time.perf_counter()
    e = rs.encode(p)
    ORACLE_SECONDS[0] += time.perf_counter() - t
    return e


@functools.lru_cache(maxsize=None)
def lane_sums(ri, agg, Q):
    """the Q partial sums of row ri as encodings (Q = 1: the row's sum)"""
    row = rows()[ri]
    where = {k: a for a, k in enumerate(active_slots(row))}
    acc = [rs.IDENT] * Q
    for k, s, i in expected(ri, agg)[2]:
        q = where[k] % Q
        acc[q] = rs.pt_add(acc[q], product(s, i))
    return [_encode(p) for p in acc]


# ---- the digit strings -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def digit_pairs():
    """[(s, point index)]: the scalar battery as sm.mul_items() pairs it, then every nibble at every digit position below 63"""
    bat = sm.scalar_battery()
    pairs = list(sm.mul_items()[:len(bat)])
    assert [s for s, _ in pairs] == list(bat)
    have = set(bat)
    for j in range(63):
        for n in range(1, 16):
            s = n << (4 * j)
            if s not in have:
                have.add(s)
                pairs.append((s, sm.WORK[(j + n) % len(sm.WORK)]))
    return pairs


def _row(name, n, ver, pairs=(), seed=0, bad_skipped=False, **kw):
    """wv slots from `pairs` (then 1s), every other scalar 1 unless given, the other points dealt from the good ones by `seed`"""
    m, npts = 4 + n, n_points(n)
    pidx = [(seed + 5 * k) % N_GOOD for k in range(npts)]
    wv = [1] * m
    assert len(pairs) <= m
    for j, (s, i) in enumerate(pairs):
        wv[j], pidx[6 + j] = s, i
    if bad_skipped:
        assert not ver
        pidx[3:6] = [BAD0 + (seed + k) % len(BAD_ENCODINGS) for k in range(3)]
    for k, i in kw.pop("points", {}).items():
        pidx[k] = i
    f = dict(x=1, r=1, u=1, rho=1, uj=(1,) * 11, uji=(1,) * 11)
    f.update(kw)
    return Row(name, n, ver, tuple(pidx), f["x"], f["r"], f["u"], f["rho"], tuple(f.get("wv", wv)), tuple(f["uj"]), tuple(f["uji"]))


CANCEL_Q, CANCEL_LANE = 64, 10  # k_varbase lane 10 of 64 on the first N = 202 row: four wv slots, two cancelling pairs


@functools.lru_cache(maxsize=None)
def _built():
    """(rows, launches)"""
    rnd = random.Random(0x7a6b)
    pairs = list(digit_pairs())
    out, launches = [], []

    def add(row):
        out.append(row)
        return len(out) - 1

    def take(count):
        got = pairs[:count]
        del pairs[:count]
        return got

    # -- the three rows of N = 202 (206 wv slots each).  Row a, two-phase: lane CANCEL_LANE of CANCEL_Q owns slots 10, 74, 138, 202,
    # all wv slots, holding s, l - s on one point and t, l - t on another
    s, t = sm.scalar_classes()["random"][5], sm.NAMED["all_9"]
    a_pairs = take(202)
    for j, pr in ((4, (s, 2)), (68, (L - s, 2)), (132, (t, 3)), (196, (L - t, 3))):
        a_pairs.insert(j, pr)
    big_a = add(_row("n202.a", 202, 1, a_pairs, seed=1))
    big_b = add(_row("n202.b", 202, 0, take(206), seed=2, bad_skipped=True))
    big_c = add(_row("n202.c", 202, 1, take(206), seed=3))
    # -- N = 1 rows (5 wv slots), both versions
    small = {0: [], 1: []}
    for j in range(10):
        ver = j % 2
        small[ver].append(add(_row("n1.%d" % j, 1, ver, take(5), seed=4 + j, bad_skipped=(ver == 0 and j % 4 == 0))))
    # -- N = 8 rows (12 wv slots) for the rest: a block of one-phase rows, then a block of two-phase rows
    n8 = -(-len(pairs) // 12)
    mid = {0: [], 1: []}
    for j in range(n8):
        ver = 0 if j < n8 // 2 else 1
        mid[ver].append(add(_row("n8.%d" % j, 8, ver, take(12), seed=j, bad_skipped=(ver == 0 and j % 2 == 0))))
    assert not pairs

    # -- everything cancels: N = 1, two-phase, 19 pairs (P, -P with scalar 1; s, l - s on one point) and identities
    neg = sm.NEG2
    cancel = add(_row("cancel", 1, 1, [(s, 3), (L - s, 3), (t, 4), (L - t, 4), (0, 5)],
                      points=dict([(k, (2, neg)[k % 2]) for k in range(6)] + [(11 + k, (2, neg, 2, neg, 0)[k]) for k in range(5)]
                                  + [(16 + k, (2, neg)[k % 2] if k < 10 else 0) for k in range(11)]
                                  + [(27 + k, (2, neg)[k % 2] if k < 10 else 0) for k in range(11)])))
    # -- points that do not decode, in every slot class; the scalar they would have had is not 1
    r1 = rnd.randrange(L)
    bad_wv = add(_row("bad.wv", 8, 0, [(r1, 2), (7, 3), (r1, 4)], seed=5, bad_skipped=True, points={8: BAD0}))
    bad_a2 = add(_row("bad.a2", 8, 1, [(r1, 2)], seed=6, points={4: BAD0 + 1}, u=3))
    bad_tr = add(_row("bad.t+r", 1, 0, [(r1, 3)], seed=7, points={6 + 5 + 2: BAD0 + 2, n_points(1) - 1: BAD0 + 3}, r=5, uji=(9,) * 11))
    bad_a1 = add(_row("bad.a1+l", 1, 1, [], seed=8, points={0: BAD0 + 3, 6 + 5 + 5: BAD0}, x=2, uj=(4,) * 11))

    # -- the other slot classes' algebra
    def some(count, special):
        return tuple(special) + tuple(rnd.randrange(L) for _ in range(count - len(special)))
    alg = [
        add(_row("alg.minus1", 1, 1, seed=2, x=L - 1, r=L - 1, u=L - 1, wv=(1, L - 1, 2, 0, rnd.randrange(L)),
                 uj=some(11, (L - 1, 1, 0, 1 << 126)), uji=some(11, (1, 0, L - 1, (1 << 126) + 1)))),
        add(_row("alg.2^126", 1, 0, seed=3, x=1 << 126, r=1 << 126, u=rnd.randrange(L), wv=some(5, (1, 0)), uj=some(11, (2,)), uji=some(11, (3,)))),
        add(_row("alg.random", 1, 1, seed=4, x=rnd.randrange(L), r=rnd.randrange(L), u=rnd.randrange(L), rho=rnd.randrange(L), wv=some(5, ()),
                 uj=some(11, ()), uji=some(11, ()))),
        add(_row("alg.rho-1", 1, 0, seed=5, x=rnd.randrange(L), r=rnd.randrange(L), u=rnd.randrange(L), rho=L - 1, wv=some(5, (1,)), uj=some(11, (1,)),
                 uji=some(11, (1,)))),
        add(_row("alg.n8", 8, 0, seed=6, x=rnd.randrange(L), r=rnd.randrange(L), u=rnd.randrange(L), rho=rnd.randrange(L), wv=some(12, (0, 1)),
                 uj=some(11, ()), uji=some(11, ()))),
    ]
    rho0 = add(out[alg[2]]._replace(name="alg.rho0", rho=0))

    # -- launches.  Q and agg cycle; the digit rows have rho = 1, so agg changes nothing in what they must give
    cyc = QS + (Q_BEYOND,)
    count = [0]

    def launch(name, group, rows, Q=None, agg=None):
        k = count[0]
        count[0] += 1
        launches.append(Launch(name, group, tuple(rows), cyc[k % len(cyc)] if Q is None else Q, k % 2 if agg is None else agg))

    launch("n202.a", "n202", [big_a], Q=CANCEL_Q)
    launch("n202.b", "n202", [big_b], Q=Q_BEYOND)
    launch("n202.ac", "n202", [big_a, big_c], Q=7)
    launch("n202.b2", "n202", [big_b], Q=2)
    launch("n202.c1", "n202", [big_c], Q=1)
    for ver in (0, 1):
        ids, at, j = mid[ver], 0, 0
        while at < len(ids):
            b = (5, 3, 2, 1)[j % 4]
            launch("n8.v%d.%d" % (ver, j), "n8.%d" % (j % 4), ids[at:at + b])
            at, j = at + b, j + 1
        launch("n1.v%d.5" % ver, "n1", small[ver])
        launch("n1.v%d.3" % ver, "n1", small[ver][:3])
        launch("n1.v%d.1" % ver, "n1", small[ver][4:5])
        launch("n1.v%d.2" % ver, "n1", small[ver][1:3])
    launch("cancel", "special", [cancel], Q=1, agg=0)
    launch("cancel.3", "special", [small[1][0], cancel, small[1][1]], Q=1, agg=1)
    for b in (bad_wv, bad_a2, bad_tr, bad_a1):
        launch(out[b].name, "special", [b])
    launch("bad.mixed", "special", [bad_wv, bad_a2, bad_tr, bad_a1, mid[1][0]])
    # the mixed launch the strides are about: N = 8, 1, 202, 1, 8 with a one-phase N = 1 row on either side of the two-phase N = 202 row
    launch("mixed.7", "mixed", [mid[1][1], small[0][0], big_c, small[0][1], mid[0][0]], Q=7, agg=0)
    launch("mixed.64", "mixed", [mid[1][1], small[0][0], big_c, small[0][1], mid[0][0]], Q=64, agg=1)
    launch("mixed.2", "mixed", [small[0][2], big_a], Q=CANCEL_Q)
    launch("mixed.3", "mixed", [big_b, bad_wv, small[1][2]], Q=Q_BEYOND)
    launch("mixed.1", "mixed", [mid[0][1]], Q=2)
    for ri in alg:
        launch(out[ri].name + ".agg0", "algebra", [ri], agg=0)
    for ri in alg[2:] + [rho0]:
        launch(out[ri].name + ".agg1", "algebra", [ri], agg=1)
    launch("alg.mixed.agg0", "algebra", alg, agg=0)
    launch("alg.mixed.agg1", "algebra", alg[2:] + [rho0, cancel], agg=1)
    return out, launches


def rows():
    return _built()[0]


def launches():
    return _built()[1]


def groups():
    return sorted({la.group for la in launches()})


# ---- the ledger ------------------------------------------------------------------------------------------------------------------
def _signed(i):
    """point index -> (index of its absolute point, sign): sm.NEG2 is minus point 2"""
    return (2, -1) if i == sm.NEG2 else (i, 1)


def cancels(terms):
    """True when the terms sum to the identity for a reason the ledger can see without the oracle: at least two non-zero terms, and
    on every distinct point the scalars add up to 0 mod l (the identity, point 0, may carry anything)"""
    per = collections.defaultdict(int)
    for _, s, i in terms:
        p, sign = _signed(i)
        if p != 0:
            per[p] += sign * s
    return sum(1 for _, s, i in terms if s and _signed(i)[0] != 0) >= 2 and all(v % L == 0 for v in per.values())


def ledger():
    """asserts what the battery must contain; returns the counts it found"""
    rr, ll = rows(), launches()
    for row in rr:
        assert len(row.pidx) == n_points(row.n) and len(row.wv) == 4 + row.n and len(row.uj) == len(row.uji) == 11 and row.ver in (0, 1)
        assert all(0 <= v < L for v in (row.x, row.r, row.u, row.rho) + row.wv + row.uj + row.uji), row.name
        assert active_slots(row) == [a + 3 if (not row.ver and a >= 3) else a for a in range(n_points(row.n) - (0 if row.ver else 3))]
    used = sorted({ri for la in ll for ri in la.rows})
    assert used == list(range(len(rr))), "a row no launch runs"
    # digit strings through the wv slots with x = r = 1
    digit_at, have, carries = collections.defaultdict(set), set(), set()
    for ri, row in enumerate(rr):
        if (row.x, row.r) != (1, 1):
            continue
        for k, s, _ in expected(ri, 0)[2]:
            if slot_class(row.n, k) == "wv":
                assert s == row.wv[k - 6]
                have.add(s)
    for s in have:
        for j, d in enumerate(sm.offset_digits(s)):
            digit_at[j].add(d)
        carries.add(tuple(sm.offset_word_carries(s)))
    for j in range(63):
        assert digit_at[j] == set(range(-8, 8)), (j, sorted(digit_at[j]))
    assert digit_at[63] == {0, 1}  # a canonical scalar's top nibble is 0 or 1 and nothing carries into it (sm.ledger has the argument)
    for w in range(7):
        assert any(c[w] == 1 for c in carries) and any(c[w] == 0 for c in carries), w
    assert (1,) * 7 + (0,) in carries and (0,) * 8 in carries and all(c[7] == 0 for c in carries)
    assert sm.NAMED["777..78"] in have and sm.NAMED["777..77"] in have and sm.NAMED["all_8"] in have
    assert set(sm.offset_digits(sm.NAMED["777..77"])[:63]) == {7} and sm.offset_digits(sm.NAMED["all_8"])[:63] == [-8] + [-7] * 62
    for v in [0, 1, L - 1] + [2**k for k in range(253)] + [L - 2**k for k in range(253)]:
        assert v in have, hex(v)
    assert set(sm.scalar_battery()) <= have
    # zero scalars, undecodable points
    bad_class, zero_class, skipped_bad = set(), set(), 0
    for ri, row in enumerate(rr):
        status, digits, terms = expected(ri, 0)
        act = set(active_slots(row))
        bad = [k for k in act if not decodes(row.pidx[k])]
        assert status == (ERR_VERIFY if bad else OK)
        assert all(digits[k] == ZERO_DIGITS for k in bad) and not set(bad) & {k for k, _, _ in terms}
        assert all(slot_scalar(row, k, 0) not in (0, 1) for k in bad), row.name  # dropping it out is not what its scalar does anyway
        bad_class |= {slot_class(row.n, k) for k in bad}
        zero_class |= {slot_class(row.n, k) for k, s, i in terms if s == 0 and i != 0}
        assert all(digits[k] == ZERO_DIGITS for k, s, _ in terms if s == 0)
        if not row.ver:
            assert not act & {3, 4, 5} and all(digits[k] == UNWRITTEN for k in (3, 4, 5))
            if any(not decodes(row.pidx[k]) for k in (3, 4, 5)) and not bad:
                skipped_bad += 1  # undecodable encodings in the skipped slots and status OK: reading them would show
    assert bad_class == set(CLASSES), bad_class
    assert {"wv", "L", "R"} <= zero_class
    assert skipped_bad >= 3
    # every slot class with a scalar that is neither 0 nor 1, in both phases, without and with the weight
    for ver in (0, 1):
        for agg in (0, 1):
            seen = set()
            for la in ll:
                if la.agg == agg:
                    for ri in la.rows:
                        if rr[ri].ver == ver:
                            seen |= {slot_class(rr[ri].n, k) for k, s, _ in expected(ri, agg)[2] if s not in (0, 1)}
            assert seen == set(CLASSES) - (set() if ver else {"A2"}), (ver, agg, seen)
    assert any(la.agg and rr[ri].rho not in (0, 1) for la in ll for ri in la.rows)
    assert any(la.agg and rr[ri].rho == 0 for la in ll for ri in la.rows)
    # cancellation: a k_varbase lane whose share cancels, a whole row that cancels under k_varsum
    lane_hits, row_hits = set(), set()
    for la in ll:
        for ri in la.rows:
            row, terms = rr[ri], expected(ri, la.agg)[2]
            if cancels(terms):
                row_hits |= {f for f in forms_of(la) if f in (PREP_SUM, MX_PREP_SUM)}
            for q in range(min(la.Q, len(active_slots(row)))):
                share = set(lane_share(row, la.Q, q))
                mine = [t for t in terms if t[0] in share]
                if len(share) >= 2 and len(mine) == len(share) and cancels(mine):
                    lane_hits |= {(f, la.Q > 1) for f in forms_of(la) if f in (LANES, MX_LANES)}
    assert row_hits == {PREP_SUM, MX_PREP_SUM}, row_hits
    assert lane_hits >= {(LANES, True), (MX_LANES, True), (LANES, False), (MX_LANES, False)}, lane_hits
    a = next(ri for ri, row in enumerate(rr) if row.name == "n202.a")
    assert lane_share(rr[a], CANCEL_Q, CANCEL_LANE) == [10, 74, 138, 202] and all(slot_class(202, k) == "wv" for k in (10, 74, 138, 202))
    # shapes
    assert sum(1 for row in rr if row.n == 202) <= 3 and {row.n for row in rr} == set(NS)
    for form in FORM_NAMES:
        mine = [la for la in ll if form in forms_of(la)]
        assert {len(la.rows) for la in mine} == set(BS), (form, sorted({len(la.rows) for la in mine}))
        assert {rr[ri].n for la in mine for ri in la.rows} == set(NS) and {rr[ri].ver for la in mine for ri in la.rows} == {0, 1}
        assert {la.agg for la in mine} == {0, 1}
        if form in (LANES, MX_LANES):
            assert {la.Q for la in mine} == set(QS) | {Q_BEYOND}, form
            for n in NS:
                assert {la.Q for la in mine if any(rr[ri].n == n for ri in la.rows)} >= set(QS) | {Q_BEYOND}, (form, n)
    assert Q_BEYOND > max(len(active_slots(row)) for row in rr)
    assert all(len(la.rows) in BS for la in ll)
    strides = 0
    for la in ll:
        sig = [(rr[ri].n, rr[ri].ver) for ri in la.rows]
        for j in range(1, len(sig) - 1):
            if sig[j - 1] == (1, 0) and sig[j] == (202, 1) and sig[j + 1] == (1, 0) and {n for n, _ in sig} == set(NS) and {v for _, v in sig} == {0, 1}:
                strides += 1
    assert strides >= 2
    return {"rows": len(rr), "launches": len(ll), "kernel_runs": sum(len(forms_of(la)) for la in ll), "digit_strings": len(have),
            "slots": sum(len(active_slots(rr[ri])) for la in ll for ri in la.rows)}


# ---- the check, one launch through one form ------------------------------------------------------------------------------------------
def native_rows(launch):
    out = []
    for ri in launch.rows:
        row = rows()[ri]
        out.append((row.n, row.ver, [encoding(i) for i in row.pidx], (row.x, row.r, row.u, row.rho), row.wv, row.uj + row.uji))
    return out


def check_launch(ctx, launch, form):
    """runs the launch through bbp_debug_varbase and compares status, digit words and every partial sum; returns the sums compared"""
    lanes = form in (LANES, MX_LANES)
    nq = launch.Q if lanes else 1
    got = ctx.debug_varbase(form, native_rows(launch), launch.Q, launch.agg)
    what = (launch.name, FORM_NAMES[form], launch.Q, launch.agg)
    for (sums, digits, status), ri in zip(got, launch.rows):
        e_status, e_digits, _ = expected(ri, launch.agg)
        assert status == e_status, what + (rows()[ri].name, "status")
        wrong = [k for k in range(len(e_digits)) if digits[k] != e_digits[k]]
        assert not wrong, what + (rows()[ri].name, "digit words of slots", wrong[:5])
        e_sums = lane_sums(ri, launch.agg, nq)
        wrong = [q for q in range(nq) if sums[q] != e_sums[q]]
        assert not wrong, what + (rows()[ri].name, "partial sums of lanes", wrong[:5])
    return nq * len(launch.rows)
