"""CPU tier: the ledger of tests/scalarmul_cases.py -- what the scalar battery of the radix-16 scalar-multiplication tests must
contain -- and the model's own consistency."""
import random

from tests import scalarmul_cases as sm

L = sm.L


def test_ledger():
    counts = sm.ledger()
    print("scalar battery:", counts)
    assert counts["scalars"] <= 1500  # (the GPU tests stay a few seconds)


def test_ledger_notices_a_missing_edge():
    """the ledger fails when a class is dropped from the battery (the digit class alone is not missed: the random scalars reach every
    digit value at every position too)"""
    cls = sm.scalar_classes()
    for name in ("chain", "named", "piece", "value"):
        rest = [s for other, vals in cls.items() if other != name for s in vals]
        try:
            sm.ledger(rest)
        except AssertionError:
            continue
        raise AssertionError("the ledger does not miss class %r" % name)


def test_model_recodings():
    """both recodings give back the scalar; digit ranges; the offset form word by word equals the big addition"""
    rnd = random.Random(5)
    for s in [rnd.randrange(L) for _ in range(300)] + sm.scalar_battery()[:300]:
        cd, cin = sm.carry_digits(s)
        od = sm.offset_digits(s)
        assert sum(d << (4 * j) for j, d in enumerate(cd)) == s and all(-7 <= d <= 8 for d in cd) and cin[64] == 0
        assert sum(d << (4 * j) for j, d in enumerate(od)) == s and all(-8 <= d <= 7 for d in od)
        words, cy = sm.offset_words(s)
        assert cy == 0 and sum(w << (32 * i) for i, w in enumerate(words)) == s + sm.OFFSET
        for lo, hi in sm.share_ranges():
            assert sm.piece_value(s, lo, hi) == sum(sm.piece_value(s, k, k + 1) for k in range(lo, hi))
        assert sm.piece_value(s, 0, sm.TAIL_PIECES) == s


def test_items_are_canonical_and_in_range():
    npts = len(sm.points())
    assert sm.points()[sm.NEG2] == sm.rs.pt_neg(sm.points()[2]) and sm.points()[0] == sm.rs.IDENT
    for i0, i1, v, b in sm.comb_items():
        assert i0 < npts and i1 < npts and 0 <= v < L and 0 <= b < L
    for s, i, lo, hi in sm.tail_items():
        assert i < npts and 0 <= s < L and 0 <= lo <= hi <= sm.TAIL_PIECES
    for s1, i1, s2, i2 in sm.pair_items():
        assert i1 < npts and i2 < npts and 0 <= s1 < L and 0 <= s2 < L
    for it in sm.straus_items():
        assert 1 <= len(it) <= sm.STRAUS_MAX and all(i < npts and 0 <= s < L for s, i in it)
    assert any(i0 == i1 and (v + b) % L == 0 and v for i0, i1, v, b in sm.comb_items())
    assert any(i0 == i1 and v == b and v for i0, i1, v, b in sm.comb_items())
    assert any({i1, i2} == {2, sm.NEG2} and s1 == s2 for s1, i1, s2, i2 in sm.pair_items())
