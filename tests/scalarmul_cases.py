"""Scalar and point batteries for the radix-16 scalar multiplications of csrc/scalarmul.h, with a plain Python model of their two
recodings, for both tiers: tests/test_scalarmul_host.py (the header compiled for the host by tests/host_check.cpp) and
tests/test_gpu_scalarmul.py (compiled for gfx950 by tests/device_check.hip).  tests/test_scalarmul_cases_host.py asserts the ledger
over the battery, so that the battery cannot quietly lose an edge.

Every scalar is canonical (< L): the kernels index 8-entry tables by digit magnitude and the product never feeds them anything else.

Carry recoding (comb, tail tables): d = nibble_j + carry_in; carry_out = d > 8; digit = d - 16 carry_out.  d lies in 0..16, so the
digits a canonical scalar can produce are -7..8: d = 8 stays +8 and -8 is never produced.  (The tables hold 8 P, so a recoder that
carried at d >= 8 and produced -8 would be equally right; this one does not.)
Offset recoding (verifier Straus): sp = s + 0x88..8 over 256 bits with the carries between the words; digit = nibble_j(sp) - 8, -8..7."""
import functools
import random

from oracle.ref_py import ristretto as rs
from tests import arith_cases as ac

L = rs.L
TAIL_PIECES = 8  # csrc/scalarmul.h BBP_TAIL_PIECES (the tests ask the built libraries and compare)
TAIL_DIGITS = 64 // TAIL_PIECES
COMMIT_L = 8
OFFSET = int("88" * 32, 16)
STRAUS_MAX = 4


# ---- the model ---------------------------------------------------------------------------------------------------------------
def nibble(s, j):
    return (s >> (4 * j)) & 15


def carry_digits(s):
    """(digits[64], carry_in[65]) of the carry recoding; carry_in[64] is the carry out of digit 63"""
    digits, cin, c = [], [0], 0
    for j in range(64):
        d = nibble(s, j) + c
        c = 1 if d > 8 else 0
        digits.append(d - 16 * c)
        cin.append(c)
    return digits, cin


def offset_words(s):
    """the eight digit words of the offset recoding, computed word by word with the carries between the words"""
    words, cy = [], 0
    for i in range(8):
        cy += ((s >> (32 * i)) & 0xffffffff) + 0x88888888
        words.append(cy & 0xffffffff)
        cy >>= 32
    return words, cy


def offset_digits(s):
    words, _ = offset_words(s)
    return [((words[j >> 3] >> (4 * (j & 7))) & 15) - 8 for j in range(64)]


def offset_word_carries(s):
    """carry out of each of the eight word additions of s + 0x88..8"""
    out, cy = [], 0
    for i in range(8):
        cy += ((s >> (32 * i)) & 0xffffffff) + 0x88888888
        cy >>= 32
        out.append(cy)
    return out


def piece_value(s, k_lo, k_hi, pieces=TAIL_PIECES):
    """what ge_scalarmul_pieces multiplies the point by for pieces k_lo <= k < k_hi: the signed digits of those pieces at their weights"""
    digits, _ = carry_digits(s)
    per = 64 // pieces
    return sum(digits[j] << (4 * j) for j in range(per * k_lo, per * k_hi))


def carry_chains(s):
    """[(start, length)]: maximal runs of consecutive digits that carry out; the run's last carry enters digit start + length"""
    _, cin = carry_digits(s)
    out, j = [], 0
    while j < 64:
        if cin[j + 1]:
            a = j
            while j < 64 and cin[j + 1]:
                j += 1
            out.append((a, j - a))
        else:
            j += 1
    return out


# ---- the scalar battery ------------------------------------------------------------------------------------------------------
def boundary_positions(pieces=TAIL_PIECES):
    per = 64 // pieces
    pos = {0, 7, 8, 62}
    for k in range(1, pieces):
        pos |= {per * k - 1, per * k}
    return sorted(pos)


def _nibbles(fn):
    return sum(fn(j) << (4 * j) for j in range(64))


def chain(start, length):
    """a carry chain of `length` digits from digit `start`: a 9, then 8s that carry only because of the carry they receive"""
    return _nibbles(lambda j: 9 if j == start else 8 if start < j < start + length else 0)


NAMED = {
    "all_8": int("0" + "8" * 63, 16),            # sixty-three digits of +8, no carry anywhere
    "all_9": int("0" + "9" * 63, 16),            # every digit carries: -7, then -6s, a 1 at digit 63
    "2^252-1": 2**252 - 1,
    "777..78": int("0" + "7" * 62 + "8", 16),    # + 0x88..8 carries out of every 32-bit word, each time only through the carry it received
    "777..77": int("0" + "7" * 63, 16),          # one less: no word carries
    "chain40": chain(3, 40),
}


@functools.lru_cache(maxsize=None)
def scalar_classes():
    """{class name: [scalars]}; scalar_battery() is their concatenation without repeats"""
    cls = {}
    # every nibble at every boundary position, alone and with a carry arriving from the digit below
    digit = []
    for j in boundary_positions():
        top = 15 if j < 63 else 0
        digit += [n << (4 * j) for n in range(top + 1)]
        if j:
            digit += [(n << (4 * j)) | (9 << (4 * (j - 1))) for n in (0, 7, 8, 15)]
    cls["digit"] = digit
    cls["pos63"] = [1 << 252, (1 << 252) + 5, 9 << 248, 15 << 248, chain(0, 63), L - 1]
    cls["chain"] = [chain(0, n) for n in range(1, 64)] + [chain(63 - n, n) for n in range(1, 63)] + [chain(5, 7), chain(30, 4)]
    cls["named"] = list(NAMED.values())
    per = TAIL_DIGITS
    piece = []
    for k in range(TAIL_PIECES):
        piece.append(_nibbles(lambda j: 0 if j // per == k or j == 63 else 3))   # piece k all zero, the others not
        piece.append(_nibbles(lambda j: 5 if j // per == k and j != 63 else 0))  # piece k alone
        piece.append(_nibbles(lambda j: 12 if j // per == k and j != 63 else 0))  # piece k alone, negative digits, a carry out of it
    for q in range(COMMIT_L):
        piece.append(_nibbles(lambda j: 0 if j % COMMIT_L == q or j == 63 else 1))   # lane q of a split commitment adds nothing
        piece.append(_nibbles(lambda j: 11 if j % COMMIT_L == q and j != 63 else 0))  # only lane q's nibbles are set
    cls["piece"] = piece
    cls["value"] = ([0, 1, 2, 8, 9, 16, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 2**252] + [2**k for k in range(253)]
                    + [L - 2**k for k in range(253)])
    rnd = random.Random(0x5ca1a7)
    cls["random"] = [rnd.randrange(L) for _ in range(200)]
    return cls


@functools.lru_cache(maxsize=None)
def scalar_battery():
    seen, out = set(), []
    for vals in scalar_classes().values():
        for s in vals:
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def edge_scalars():
    """the short list every point of the point battery is multiplied by"""
    return [0, 1, 2, 8, 9, 16, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 2**252, NAMED["all_8"], NAMED["all_9"], NAMED["2^252-1"],
            NAMED["777..78"], NAMED["chain40"], chain(0, 63), chain(23, 40), scalar_classes()["random"][0], scalar_classes()["random"][1]]


def ledger(scalars=None, pieces=TAIL_PIECES):
    """asserts what the battery must contain; returns the counts it found"""
    scalars = scalar_battery() if scalars is None else scalars
    assert all(0 <= s < L for s in scalars), "a non-canonical scalar in the battery"
    per = 64 // pieces
    carry_at, offset_at, chains = {}, {}, set()
    word_carry_patterns = set()
    for s in scalars:
        cd, cin = carry_digits(s)
        od = offset_digits(s)
        assert cin[64] == 0, hex(s)  # a canonical scalar never carries out of digit 63
        assert sum(d << (4 * j) for j, d in enumerate(cd)) == s and sum(d << (4 * j) for j, d in enumerate(od)) == s, hex(s)
        assert offset_words(s)[1] == 0, hex(s)  # s + 0x88..8 < 2^256
        assert sum(piece_value(s, k, k + 1, pieces) for k in range(pieces)) == s
        for j in range(64):
            carry_at.setdefault(j, set()).add(cd[j])
            offset_at.setdefault(j, set()).add(od[j])
        chains |= set(carry_chains(s))
        word_carry_patterns.add(tuple(offset_word_carries(s)))
    # digit values: the carry recoding reaches -7..8 (see the module text: -8 is never produced), the offset recoding -8..7
    for j in boundary_positions(pieces):
        assert carry_at[j] == set(range(-7, 9)), (j, sorted(carry_at[j]))
        assert offset_at[j] == set(range(-8, 8)), (j, sorted(offset_at[j]))
    assert all(-7 <= d <= 8 for j in range(64) for d in carry_at[j]) and all(-8 <= d <= 7 for j in range(64) for d in offset_at[j])
    # position 63: L = 2^252 + c with c < 2^125, so digits 32..62 of L are zero; a canonical scalar with top nibble 1 has zero nibbles
    # there and carries nothing into digit 63; the carry comes only under top nibble 0.  Reachable {0, 1}, both present, in both forms.
    assert L >> 252 == 1 and (L >> 128) & ((1 << 124) - 1) == 0
    assert carry_at[63] == {0, 1} and offset_at[63] == {0, 1}
    assert any(nibble(s, 63) == 0 and carry_digits(s)[1][63] for s in scalars) and any(nibble(s, 63) == 1 for s in scalars)
    assert not any(nibble(s, 63) == 1 and carry_digits(s)[1][63] for s in scalars)
    # carry chains
    lengths = {n for _, n in chains}
    assert lengths >= set(range(1, 64)), sorted(set(range(1, 64)) - lengths)
    assert any(a == 0 for a, _ in chains) and any(a + n == 63 for a, n in chains) and (0, 63) in chains
    assert any(n >= 40 for _, n in chains)
    for b in sorted({per * k for k in range(1, pieces)} | {8 * w for w in range(1, 8)}):  # piece and word boundaries
        assert any(a < b < a + n for a, n in chains), b          # a chain runs through the boundary
        assert any(a + n == b for a, n in chains), b              # a chain ends by entering the first digit past it
        assert any(a == b for a, n in chains), b                  # a chain starts on it
    # named strings
    have = set(scalars)
    assert set(NAMED.values()) <= have
    assert carry_digits(NAMED["all_8"]) == ([8] * 63 + [0], [0] * 65)
    assert carry_digits(NAMED["all_9"])[0] == [-7] + [-6] * 62 + [1]
    assert offset_word_carries(NAMED["777..78"]) == [1] * 7 + [0] and offset_word_carries(NAMED["777..77"]) == [0] * 8
    assert offset_word_carries(2**252 - 1) == [1] * 7 + [0]
    assert len(word_carry_patterns) >= 20
    # piece patterns, in both recodings
    for digits_of in (lambda s: carry_digits(s)[0], offset_digits):
        zero_piece, lone_piece, zero_lane = set(), set(), set()
        for s in scalars:
            d = digits_of(s)
            nz = [any(d[per * k:per * k + per]) for k in range(pieces)]
            if nz.count(False) == 1:
                zero_piece.add(nz.index(False))
            if nz.count(True) == 1:
                lone_piece.add(nz.index(True))
            lanes = [any(d[q::COMMIT_L]) for q in range(COMMIT_L)]
            if lanes.count(False) == 1:
                zero_lane.add(lanes.index(False))
        assert zero_piece == set(range(pieces)) and lone_piece == set(range(pieces)) and zero_lane == set(range(COMMIT_L))
    # values
    for v in [0, 1, 2, 8, 9, 16, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 2**252] + [2**k for k in range(253)] + [L - 2**k for k in range(253)]:
        assert v in have, hex(v)
    assert len(scalar_classes()["random"]) == 200 and set(scalar_classes()["random"]) <= have
    return {"scalars": len(scalars), "chains": len(chains), "word_carry_patterns": len(word_carry_patterns)}


# ---- points, items, and the oracle's answers ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points():
    """arith_cases.point_cases(): the identity, the basepoint, 16 random multiples -- and the negation of point 2"""
    pts = list(ac.point_cases()[0])
    return pts + [rs.pt_neg(pts[2])]


NEG2 = 18   # index of -points()[2]
WORK = (2, 3, 4)  # the points the whole scalar battery is spread over


@functools.lru_cache(maxsize=None)
def encodings():
    return [rs.encode(p) for p in points()]


@functools.lru_cache(maxsize=None)
def pt_mul(s, i):
    return rs.pt_mul(s, points()[i])


@functools.lru_cache(maxsize=None)
def mul_items():
    """[(s, point index)]: every battery scalar on one of the WORK points, every edge scalar on every point"""
    items = [(s, WORK[n % len(WORK)]) for n, s in enumerate(scalar_battery())]
    items += [(s, i) for i in range(len(points())) for s in edge_scalars()]
    return items


def _partner(n, step):
    """index of a battery scalar that mul_items() puts on point WORK[(n + 1) % 3] (so the oracle multiplies each (scalar, point) once)"""
    third = len(scalar_battery()) // 3
    return 3 * ((step * n + 1) % third) + (n + 1) % 3


@functools.lru_cache(maxsize=None)
def comb_items():
    """[(i0, i1, v, b)] -> v P_i0 + b P_i1: scalars paired with their neighbours in the battery, the edge scalars on every base,
    equal bases with b = L - v (the identity) and b = v (equal partial sums)"""
    bat = scalar_battery()
    items = [(WORK[n % 3], WORK[(n + 1) % 3], v, bat[_partner(n, 7)]) for n, v in enumerate(bat)]
    items += [(i, (i + 5) % len(points()), s, edge_scalars()[(n + 1) % len(edge_scalars())]) for i in range(len(points()))
              for n, s in enumerate(edge_scalars())]
    for n, v in enumerate(edge_scalars() + scalar_classes()["random"][:20] + scalar_classes()["piece"]):
        i = WORK[n % 3]
        items.append((i, i, v, (L - v) % L))
        items.append((i, i, v, v))
    items += [(0, 0, 5, 7), (0, 1, L - 1, 1), (1, 0, 1, L - 1)]  # the identity as a base
    return items


def comb_expected(item):
    i0, i1, v, b = item
    return rs.encode(rs.pt_add(pt_mul(v, i0), pt_mul(b, i1)))


@functools.lru_cache(maxsize=None)
def share_ranges(pieces=TAIL_PIECES):
    """(k_lo, k_hi) of every share k_tail_lr can be compiled to hand a lane (BBP_TAIL_SPLIT = 1, 2, 4, .. pieces), and the empty range"""
    out, split = [], 1
    while split <= pieces:
        pps = pieces // split
        out += [(sh * pps, sh * pps + pps) for sh in range(split)]
        split *= 2
    return out + [(3, 3)]


@functools.lru_cache(maxsize=None)
def tail_items():
    """[(s, point index, k_lo, k_hi)]: every item of mul_items() whole, the battery's scalars share by share as well"""
    items = [(s, i, 0, TAIL_PIECES) for s, i in mul_items()]
    # (most 2^k, L - 2^k and random scalars and half the single-nibble ones go whole only, and share by share for every seventh of them)
    plain = set(scalar_classes()["value"][11:]) | set(scalar_classes()["random"][40:]) | set(scalar_classes()["digit"][1::2])
    items += [(s, WORK[n % len(WORK)], lo, hi) for n, s in enumerate(scalar_battery()) if s not in plain or n % 7 == 0
              for lo, hi in share_ranges() if (lo, hi) != (0, TAIL_PIECES)]
    return items


@functools.lru_cache(maxsize=None)
def _piece_point(i, k):
    """2^(32 k) P_i, by doublings"""
    p = points()[i]
    for _ in range(4 * TAIL_DIGITS * k):
        p = rs.pt_dbl(p)
    return p


@functools.lru_cache(maxsize=None)
def _piece_mul(s, i, k):
    """(signed value of piece k of s) P_i as the oracle computes it: the piece's digits as one small integer times 2^(32 k) P_i"""
    v = piece_value(s, k, k + 1) >> (4 * TAIL_DIGITS * k)
    return rs.pt_mul(v, _piece_point(i, k))  # pt_mul reduces a negative v mod L


def tail_expected(item):
    s, i, lo, hi = item
    if (lo, hi) == (0, TAIL_PIECES):
        return rs.encode(pt_mul(s, i))
    acc = rs.IDENT
    for k in range(lo, hi):
        acc = rs.pt_add(acc, _piece_mul(s, i, k))
    return rs.encode(acc)


@functools.lru_cache(maxsize=None)
def pair_items():
    """[(s1, i1, s2, i2)] -> s1 P_i1 + s2 P_i2"""
    bat = scalar_battery()
    items = [(s, WORK[n % 3], bat[_partner(n, 11)], WORK[(n + 1) % 3]) for n, s in enumerate(bat)]
    items += [(s, 2, s, NEG2) for s in edge_scalars() + scalar_classes()["random"][:20]]   # P1 = -P2, s1 = s2: the identity
    items += [(s, i, edge_scalars()[(n + 3) % len(edge_scalars())], (i + 1) % len(points())) for i in range(len(points()))
              for n, s in enumerate(edge_scalars()) if n % 4 == i % 4]
    return items


def pair_expected(item):
    s1, i1, s2, i2 = item
    return rs.encode(rs.pt_add(pt_mul(s1, i1), pt_mul(s2, i2)))


@functools.lru_cache(maxsize=None)
def straus_items():
    """[[(s, point index), ..]] of 1, 2 and 4 terms"""
    bat = scalar_battery()
    items = [[(s, WORK[n % 3])] for n, s in enumerate(bat)]
    items += [[(s, i)] for i in range(len(points())) for s in edge_scalars()]
    items += [[(s, 2), (s, NEG2)] for s in edge_scalars() + scalar_classes()["random"][:20]]  # P1 = -P2, s1 = s2
    term = lambda m: (bat[m], WORK[m % 3])  # as mul_items() pairs them
    items += [[term(n), term(_partner(n, 5))] for n in range(0, len(bat), 4)]
    items += [[term(n), term(_partner(n, 13)), term((n + 17) % len(bat)), term((n + 500) % len(bat))] for n in range(1, len(bat), 4)]
    items += [[(s, 2), (s, NEG2), (L - 1, 0), (NAMED["all_9"], 1)] for s in edge_scalars()]
    return items


def straus_expected(item):
    acc = rs.IDENT
    for s, i in item:
        acc = rs.pt_add(acc, pt_mul(s, i))
    return rs.encode(acc)


# ---- the checks, shared by both tiers ----------------------------------------------------------------------------------------
# `run` is a tests.scalarmul_run.Runner over one built library (host or device)
def check_comb(run):
    items = comb_items()
    one, split = run.comb(encodings(), items)
    bad = [n for n, it in enumerate(items) if not (one[n] == split[n] == comb_expected(it))]
    assert not bad, (run.name, len(bad), [(items[n][0], items[n][1], hex(items[n][2]), hex(items[n][3])) for n in bad[:3]])
    ident = rs.encode(rs.IDENT)
    assert sum(1 for o in one if o == ident) >= 40  # the cancelling commitments do reach the identity
    return len(items)


def check_comb_table(run):
    idx = [0, 1, 2, 9]
    got = run.comb_table([encodings()[i] for i in idx])
    for b, i in enumerate(idx):
        p = points()[i]
        for j in range(64):
            m = p
            for k in range(8):
                assert got[(b * 64 + j) * 8 + k] == rs.encode(m), (run.name, i, j, k)  # (k + 1) * 16^j * P
                m = rs.pt_add(m, p)
            for _ in range(4):
                p = rs.pt_dbl(p)
    return len(got)


def check_tail(run):
    assert run.tail_pieces() == TAIL_PIECES
    items = tail_items()
    got = run.tail(encodings(), items)
    bad = [n for n, it in enumerate(items) if got[n] != tail_expected(it)]
    assert not bad, (run.name, len(bad), [(hex(items[n][0]),) + items[n][1:] for n in bad[:3]])
    # the shares of a scalar sum to s P (in the oracle's arithmetic, from the bytes the code under test returned)
    where = {it: n for n, it in enumerate(items)}
    for n_s, s in enumerate(scalar_battery()[::7]):  # (every seventh scalar has all its shares among the items)
        i = WORK[(7 * n_s) % len(WORK)]
        for split in (2, TAIL_PIECES):
            pps = TAIL_PIECES // split
            acc = rs.IDENT
            for sh in range(split):
                acc = rs.pt_add(acc, rs.decode(got[where[(s, i, sh * pps, sh * pps + pps)]]))
            assert rs.encode(acc) == rs.encode(pt_mul(s, i)), (run.name, hex(s), split)
    return len(items)


def check_tail_pair(run):
    items = pair_items()
    got = run.tail_pair(encodings(), items)
    bad = [n for n, it in enumerate(items) if got[n] != pair_expected(it)]
    assert not bad, (run.name, len(bad), [(hex(items[n][0]), items[n][1], hex(items[n][2]), items[n][3]) for n in bad[:3]])
    return len(items)


def check_straus(run):
    items = straus_items()
    assert {len(it) for it in items} == {1, 2, 4}
    top, lanes, words = run.straus(encodings(), items)
    bad = [n for n, it in enumerate(items) if not (top[n] == lanes[n] == straus_expected(it))]
    assert not bad, (run.name, len(bad), [[(hex(s), i) for s, i in items[n]] for n in bad[:3]])
    for n, it in enumerate(items):
        for a, (s, _) in enumerate(it):
            assert words[n][a] == offset_words(s)[0], (run.name, hex(s))
        for a in range(len(it), STRAUS_MAX):
            assert words[n][a] == [0] * 8
    return len(items)
