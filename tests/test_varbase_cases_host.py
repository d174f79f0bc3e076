"""not-gpu tier: the ledger of tests/varbase_cases.py -- what the rows and launches of tests/test_gpu_varbase_kernels.py must contain
(every nibble at every digit position, the word-boundary carries, the named values, zero scalars and undecodable points in every slot
class, the cancelling lane and the cancelling row, every slot class in both phases and under both weights, the shapes).  No GPU and no
oracle product: the model of the kernels' algebra and of the offset recoding only."""
from tests import scalarmul_cases as sm
from tests import varbase_cases as vc


def test_ledger():
    counts = vc.ledger()
    print("varbase battery:", counts)
    assert counts["digit_strings"] > len(sm.scalar_battery()) and counts["launches"] >= 60


def test_offset_recoding_model():
    """the digit words the GPU test expects are s + 0x88..8 in Python, word for word"""
    for s in (0, 1, vc.L - 1, sm.NAMED["777..78"], sm.NAMED["all_9"], 2**252):
        words, carry = sm.offset_words(s)
        assert carry == 0 and sum(w << (32 * i) for i, w in enumerate(words)) == s + sm.OFFSET
    assert sm.offset_words(0)[0] == vc.ZERO_DIGITS


def test_slot_scalars_follow_the_table():
    """slot_scalar against the table of the module text, on a row where every input differs"""
    row = next(r for r in vc.rows() if r.name == "alg.random")
    L, m, x, r, u, rho = vc.L, 4 + row.n, row.x, row.r, row.u, row.rho
    want = [x, x * x, x**3, x * u, x * x * u, x**3 * u] + [w * r * x * x for w in row.wv] + [r * x**e for e in (1, 3, 4, 5, 6)]
    want += [v * v for v in row.uj] + [v * v for v in row.uji]
    assert len(want) == vc.n_points(row.n) == 6 + m + 5 + 22
    assert [vc.slot_scalar(row, k, 0) for k in range(len(want))] == [v % L for v in want]
    assert [vc.slot_scalar(row, k, 1) for k in range(len(want))] == [v * rho % L for v in want]
    assert [vc.slot_class(row.n, k) for k in (0, 2, 3, 5, 6, 5 + m, 6 + m, 10 + m, 11 + m, 21 + m, 22 + m, 32 + m)] == [
        "A1", "A1", "A2", "A2", "wv", "wv", "T", "T", "L", "L", "R", "R"]
