"""not-gpu tier of bbp_verify_rounds*: the packing helpers of the Python binding against pack_mixed_rows, the row size against the
header's formula, and both oracles on the expanded rows -- a round call promises the statuses of bbp_verify_batch_mixed on
expand_round_rows(...), so what the oracles say about those rows is what the device tier holds the engine to."""
import os
import re

import pytest

from oracle.ref_py import blindbid as bb
from oracle.ref_py import r1cs
from tests import oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2 ** 252 + 27742317777372353535851937790883648493
OK, VERIFY, FORMAT = 0, 1, 3


def _case(c):
    """golden full-size proof -> (record, score, z_img, seed, pub_list) bytes"""
    h = lambda k: bytes.fromhex(c[k])
    return h("record"), h("q"), h("z_img"), h("seed"), b"".join(bytes.fromhex(p) for p in c["pub_list"])


@pytest.fixture(scope="module")
def cases(golden):
    return [_case(c) for c in golden("proofs_full.json")["full"]]  # N = 1 and N = 8


def test_round_row_size_is_the_headers_formula(bbp):
    src = open(os.path.join(ROOT, "include", "bbp.h")).read()
    assert re.search(r"uint32_t bbp_round_row_size\(uint32_t N\);\s*/\* bbp_proof_record_size\(N\) \+ 64 \*/", src)
    for n in (1, 3, 8, 57, 202):
        assert bbp.round_row_size(n) == bbp.lib.bbp_round_row_size(n) == bbp.lib.bbp_proof_record_size(n) + 64 == 1121 + 32 * (4 + n) + 64
        assert bbp.verify_row_size(n) - bbp.round_row_size(n) == 32 * (1 + n)  # what a row no longer carries: seed || pub_list
    assert (bbp.round_row_size(202), bbp.verify_row_size(202)) == (7777, 14273)
    assert (bbp.round_row_size(8), bbp.verify_row_size(8)) == (1569, 1857)


def test_pack_and_expand_round_trip(bbp):
    def blob(tag, n):
        return bytes((tag * 31 + i) & 0xff for i in range(n))
    rounds = [(blob(1, 32), blob(2, 32 * 3)), (blob(3, 32), blob(4, 32 * 8)), (blob(5, 32), blob(6, 32 * 8)), (blob(7, 32), blob(8, 32))]
    round_Ns, table = bbp.pack_rounds(rounds)
    assert round_Ns == [3, 8, 8, 1] and len(table) == 32 * (4 + 20)
    assert bbp.round_table_offsets(round_Ns) == [0, 128, 416, 704, 768]
    round_of = [2, 0, 1, 1, 2, 0]  # round 3 has no row; rounds 1 and 2 share N = 8
    parts = [(blob(20 + i, bbp.record_size(round_Ns[r])), blob(40 + i, 32), blob(60 + i, 32)) for i, r in enumerate(round_of)]
    rows = b"".join(a + b + c for a, b, c in parts)
    Ns, blob_x = bbp.expand_round_rows(round_Ns, table, round_of, rows)
    want = bbp.pack_mixed_rows([(rec, sc, z, rounds[r][0], rounds[r][1]) for (rec, sc, z), r in zip(parts, round_of)])
    assert (Ns, blob_x) == want
    assert len(blob_x) == bbp.mixed_row_offsets(Ns)[-1] == len(rows) + sum(32 * (1 + round_Ns[r]) for r in round_of)
    # one round, round_of left out
    one_rows = b"".join(a + b + c for (a, b, c), r in zip(parts, round_of) if r == 0)
    assert bbp.expand_round_rows([3], table[:128], None, one_rows) == bbp.expand_round_rows([3], table[:128], [0, 0], one_rows)
    for bad in (lambda: bbp.expand_round_rows(round_Ns, table[:-1], round_of, rows), lambda: bbp.expand_round_rows(round_Ns, table, round_of, rows[:-1]),
                lambda: bbp.expand_round_rows(round_Ns, table, None, rows), lambda: bbp.expand_round_rows([3], table[:128], None, one_rows + b"\0"),
                lambda: bbp.pack_rounds([(blob(1, 31), blob(2, 32))]), lambda: bbp.pack_rounds([(blob(1, 32), blob(2, 33))])):
        with pytest.raises(ValueError):
            bad()


def _oracle_py(row, n):
    """Verify::verify on one expanded row in the Python oracle: OK / VERIFY / FORMAT"""
    rs_ = 1121 + 32 * (4 + n)
    rec, score, z_img, seed, pub = row[:rs_], row[rs_:rs_ + 32], row[rs_ + 32:rs_ + 64], row[rs_ + 64:rs_ + 96], row[rs_ + 96:]
    try:
        q, z, sd, items = bb.parse_public_inputs(score, z_img, seed, pub)
        return OK if bb.verify(bb.Proof.from_record(rec, n), q, z, sd, items) else VERIFY
    except r1cs.FormatError:
        return FORMAT
    except r1cs.VerificationError:
        return VERIFY


def test_oracles_on_expanded_rows(bbp, built, cases):
    """Two rounds (N = 1, N = 8), one golden proof each.  The expanded rows verify; a changed seed or list item in the table reaches
    exactly the rows of that round, a non-canonical seed is a FormatError for them, and bit 255 / + l on an item change nothing."""
    oc = oracle_c.load(built.build_oracle())
    (rec1, q1, z1, sd1, pub1), (rec8, q8, z8, sd8, pub8) = cases
    round_Ns, table = bbp.pack_rounds([(sd1, pub1), (sd8, pub8)])
    round_of = [1, 0, 1]
    rows = rec8 + q8 + z8 + rec1 + q1 + z1 + rec8 + q8 + z8
    toff = bbp.round_table_offsets(round_Ns)

    def verdicts(tab):
        Ns, blob = bbp.expand_round_rows(round_Ns, tab, round_of, rows)
        off = bbp.mixed_row_offsets(Ns)
        return [oc.verify_many(blob[off[i]:off[i + 1]], 1, Ns[i], threads=1)[0] for i in range(len(Ns))], Ns, blob, off

    def with_scalar(at, fn):
        return table[:at] + fn(int.from_bytes(table[at:at + 32], "little")).to_bytes(32, "little") + table[at + 32:]

    st, Ns, blob, off = verdicts(table)
    assert st == [OK, OK, OK]
    assert blob[off[0]:off[1]] == rec8 + q8 + z8 + sd8 + pub8 and blob[off[1]:off[2]] == rec1 + q1 + z1 + sd1 + pub1
    assert _oracle_py(blob[off[1]:off[2]], 1) == OK  # the Python oracle: ~3 s per full-size verification, two of them here
    last8 = toff[1] + 32 * 8
    assert verdicts(with_scalar(last8, lambda v: v ^ 1))[0] == [VERIFY, OK, VERIFY]
    assert verdicts(with_scalar(toff[0] + 32, lambda v: v ^ 1))[0] == [OK, VERIFY, OK]
    assert verdicts(with_scalar(toff[1], lambda v: (v + 1) % L))[0] == [VERIFY, OK, VERIFY]
    assert verdicts(with_scalar(toff[1], lambda v: v + L))[0] == [FORMAT, OK, FORMAT]
    bad = with_scalar(toff[0], lambda v: v + L)
    st, Ns, blob, off = verdicts(bad)
    assert st == [OK, FORMAT, OK]
    assert _oracle_py(blob[off[1]:off[2]], 1) == FORMAT
    for fn in (lambda v: v | 1 << 255, lambda v: v + L):
        assert verdicts(with_scalar(last8, fn))[0] == [OK, OK, OK]
        assert verdicts(with_scalar(toff[0] + 32, fn))[0] == [OK, OK, OK]
