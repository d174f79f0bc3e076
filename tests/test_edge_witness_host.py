"""not-gpu tier of the edge-witness cases (tests/edge_witness_cases.py): the C oracle proves and accepts every case, the edge each case
is named for is present in the oracle's record (a case that lost its edge fails here instead of passing silently on the GPU), the C
oracle reproduces the big-int oracle's records of tests/golden/proofs_edge.json byte for byte, and the host build of csrc/witness_check.h
reports every case satisfied."""
import pytest

from tests import edge_witness_cases as ew
from tests import oracle_c
from tests.test_prove_check_host import wc  # noqa: F401  (the host build of witness_check.h: (check(N, row), text(mask)))

OK, VERIFY, FORMAT = 0, 1, 3


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


@pytest.fixture(scope="module")
def enc_B(golden):
    return bytes.fromhex(golden("setup_kat.json")["B"])


@pytest.fixture(scope="module")
def proved(oc):
    """[(row, status, record)] for every row of the table: one oracle call per list length."""
    out = []
    for N in sorted({n for n, _ in ew.TABLE.values()}):
        rows = ew.all_rows(oc, N)
        recs, st = oc.prove_many(b"".join(ew.prove_row(r) for r in rows), b"".join(r["ent"] for r in rows), len(rows), N, threads=8)
        size = len(recs) // len(rows)
        out += [(r, s, recs[size * i:size * (i + 1)]) for i, (r, s) in enumerate(zip(rows, st))]
    return out


def test_the_table_holds_the_values_it_is_named_for(oc):
    rows = ew.all_rows(oc)
    assert [r["name"] for r in rows] == ["zero", "d0", "zero_blind", "one", "max", "d_wide/2^64", "d_wide/l-1", "noncanon_blind", "carry",
                                         "same_items", "zero_items", "n1_zero", "n202_zero_blind"]
    by = {r["name"]: r for r in rows}
    assert all(len(r["ent"]) == 32 * (4 + r["N"]) + 32 and len(r["pub"]) == r["N"] for r in rows)
    assert all(v < ew.L for r in rows for v in r["f"])                                        # the seven scalars stay canonical
    assert by["zero"]["f"][ew.D] == by["zero"]["f"][ew.K] == by["zero"]["f"][ew.SEED] == 0 and by["zero"]["ent"] == bytes(32 * 8)
    assert by["max"]["f"][ew.D] == 2**64 - 1 and by["max"]["f"][ew.K] == by["max"]["f"][ew.SEED] == ew.L - 1
    assert by["max"]["ent"] == ew.b32(ew.L - 1) * 7 + b"\xff" * 32
    assert by["one"]["ent"] == (b"\x01" + bytes(31)) * 8
    assert [ew.sc(by["noncanon_blind"]["ent"][32 * j:32 * j + 32]) for j in range(8)] == [ew.FF, ew.L, ew.L + 1, 1 << 255, ew.FF, ew.L, ew.L + 1, ew.FF]
    assert by["d_wide/2^64"]["f"][ew.D] == 1 << 64 and by["d_wide/l-1"]["f"][ew.D] == ew.L - 1
    assert by["carry"]["f"][ew.K] == ew.P7778 and [ew.sc(by["carry"]["ent"][32 * j:32 * j + 32]) for j in range(7)] == ew.CARRY[:7]
    assert set(by["same_items"]["pub"]) == {ew.b32(by["same_items"]["x"])} and by["same_items"]["toggle"] == 7
    assert [p == bytes(32) for p in by["zero_items"]["pub"]] == [True, False] * 4
    assert len(by["n202_zero_blind"]["identity_V"]) == 201 and by["n202_zero_blind"]["ent"][:32 * 206] == bytes(32 * 206)


def test_oracle_proves_and_accepts_every_case(oc, proved):
    for r, st, rec in proved:
        assert st == OK and len(rec) == 1121 + 32 * (4 + r["N"]), r["name"]
        f = r["f"]
        assert oc.verify(rec, ew.b32(f[ew.Q]), ew.b32(f[ew.Z]), ew.b32(f[ew.SEED]), ew.pub_list(r)) == OK, r["name"]


def test_every_case_holds_the_edge_it_is_named_for(proved, enc_B):
    for r, _st, rec in proved:
        assert ew.identity_slots(rec, r["N"]) == set(r["identity_V"]), r["name"]
        assert (r["f"][ew.Q] == 0) == r["score_zero"], r["name"]
    by = {r["name"]: (r, rec) for r, _st, rec in proved}
    assert {n for n, (r, _) in by.items() if r["identity_V"]} == {"zero", "zero_blind", "same_items", "n1_zero", "n202_zero_blind"}
    assert {n for n, (r, _) in by.items() if r["score_zero"]} == {"zero", "d0", "n1_zero"}
    for name, slot in (("zero", 4 + 1), ("zero_blind", 4 + 2), ("noncanon_blind", 4 + 1)):  # 1 * B + 0 * B_blinding (l reduces to zero)
        r, rec = by[name]
        assert rec[slice(*ew.v_slot(r["N"], slot))] == enc_B, name


def test_oracle_refuses_every_tampered_copy(oc, proved, enc_B):
    """What the GPU tier holds the device verifiers to: the oracle's status of every tampered row, none of them OK; the identity for
    A_I1 is a verification error, the identity for V is not refused by itself (the untampered rows above hold it)."""
    for r, _st, rec in proved:
        t = ew.tampered(r, rec, enc_B)
        st = oc.verify_many(b"".join(rec2 + tail for _l, rec2, tail in t), len(t), r["N"], threads=8)
        assert st == [VERIFY] * len(t), (r["name"], [(l, s) for (l, _r, _t), s in zip(t, st)])  # none is a FormatError: the bytes parse
        assert t[-1][0] == "A_I1 = identity", r["name"]


def test_c_oracle_reproduces_the_big_int_oracle_s_golden_records(oc, golden):
    cases = golden("proofs_edge.json")["edge"]
    rows = ew.golden_rows(oc)
    assert [(c["case"], c["N"], c["toggle"]) for c in cases] == ew.GOLDEN
    for c, r in zip(cases, rows):
        s7 = b"".join(bytes.fromhex(c[k]) for k in ["d", "k", "y", "y_inv", "q", "z_img", "seed"])
        pub = b"".join(bytes.fromhex(p) for p in c["pub_list"])
        ent = bytes.fromhex(c["entropy"])
        assert (s7, pub, c["toggle"], ent) == (ew.scalars7(r), ew.pub_list(r), r["toggle"], r["ent"]), c["name"]  # the file is the table's rows
        rc, rec, trace = oc.prove(s7, pub, c["toggle"], ent, want_trace=True)
        assert rc == OK and rec.hex() == c["record"], c["name"]
        for k in ("y", "z", "u", "x", "w"):
            assert trace[k] == c["trace"][k], (c["name"], k)
        assert ew.identity_slots(rec, c["N"]) == set(r["identity_V"]), c["name"]
        assert oc.verify(rec, bytes.fromhex(c["q"]), bytes.fromhex(c["z_img"]), bytes.fromhex(c["seed"]), pub) == OK


def test_witness_check_is_satisfied_by_every_case(oc, wc):  # noqa: F811
    check, text = wc
    rows = ew.all_rows(oc) + ew.golden_rows(oc)
    for r in rows:
        assert check(r["N"], ew.prove_row(r)) == 0, (r["name"], text(check(r["N"], ew.prove_row(r))))
    zero = ew.build(oc, "zero")[0]
    bad = dict(zero, f=list(zero["f"]))
    bad["f"][ew.Z] = (zero["f"][ew.Z] + 1) % ew.L
    assert check(3, ew.prove_row(bad)) == 8 and "z_img" in text(8)
    for other in (0, 2):                                             # the toggle on an item that is not x
        assert zero["pub"][other] != zero["pub"][zero["toggle"]]
        assert check(3, ew.prove_row(dict(zero, toggle=other))) == 4
    same = ew.build(oc, "same_items")[0]
    assert all(check(8, ew.prove_row(dict(same, toggle=t))) == 0 for t in range(8))  # every item is x: any toggle satisfies
    items = ew.build(oc, "zero_items")[0]
    assert check(8, ew.prove_row(dict(items, toggle=0))) == 4       # a zero item is not x
