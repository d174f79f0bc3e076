"""not-gpu tier: why the forged rows of tests/forgery_cases.py are the right ones to throw at the device verifiers.

The model is the big-int oracle (oracle/ref_py) on the small circuits of tests/golden/proofs_small.json with its mega-check
point captured.  For every cancelling set it shows that each member is rejected with a residual that is not the identity, that
the residuals add up to the identity -- so a verifier that sums a group's checks with equal weights, one weight, or none accepts
the whole set -- and that the sum under the weights the device draws (the second 64-byte draw of each proof's verifier rng,
csrc/verifier.inc k_vtranscript) is not the identity.  tests/test_gpu_verify_forgery.py requires status VERIFY for exactly these
rows on every aggregated path.

The field sweep then runs through the Python oracle and the C oracle, which must agree on the class (OK / VerificationError /
FormatError) of every row; a row whose mutation changed a value the verifier computes with must not be OK.  Both oracles refuse
a non-canonical score, z_img or seed as the reference's parse does (src/blindbid/verify.rs:100-102: serde Scalars; the bid list
goes through Scalar::from_bits at line 115).  The two are restatements of that one rule, not independent witnesses of it; the
device's k_vparse is the third reading, and tests/test_gpu_boundary.py pins it."""
import hashlib
import random

import pytest

from oracle.ref_py import blindbid as bb, merlin, r1cs, ristretto as rs
from tests import forgery_cases as fc, oracle_c

OK, VERIFY, FORMAT = fc.OK, fc.VERIFY, fc.FORMAT


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


def _row(c):
    return (bytes.fromhex(c["record"]), bytes.fromhex(c["q"]), bytes.fromhex(c["z_img"]), bytes.fromhex(c["seed"]),
            b"".join(bytes.fromhex(p) for p in c["pub_list"]))


def py_status(row, rounds, cap, ent=bytes(32)):
    """The Python oracle's class of a row: its parse of the record and of the public inputs (oracle/ref_py/blindbid.py
    parse_public_inputs), then its verifier."""
    try:
        proof = bb.Proof.from_record(row[0], fc.n_of(row))
        score, z_img, seed, pub = bb.parse_public_inputs(row[1], row[2], row[3], row[4])
        bb.verify(proof, score, z_img, seed, pub, ent, rounds, cap)
    except r1cs.FormatError:
        return FORMAT
    except r1cs.VerificationError:
        return VERIFY
    return OK


@pytest.fixture()
def spy(monkeypatch):
    """Captures, per verification, the mega-check point (the last rs.msm r1cs makes) and the verifier rng (to draw rho)."""
    seen = {}
    msm, build_rng = rs.msm, merlin.Transcript.build_rng

    def spy_msm(s, p):
        seen["mega"] = msm(s, p)
        return seen["mega"]

    def spy_rng(self, witnesses, entropy32):
        seen["rng"] = build_rng(self, witnesses, entropy32)
        return seen["rng"]
    monkeypatch.setattr(r1cs.rs, "msm", spy_msm)
    monkeypatch.setattr(merlin.Transcript, "build_rng", spy_rng)

    def residual(row, c, ent):
        seen.clear()
        st = py_status(row, c["rounds"], c["cap"], ent)
        rho = rs.sc_wide(seen["rng"].fill_bytes(64))  # the rng has given r; the next 64 bytes are this proof's weight
        return st, seen["mega"], rho
    return residual


def _sum(points):
    acc = rs.IDENT
    for p in points:
        acc = rs.pt_add(acc, p)
    return acc


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_cancelling_sets_pass_an_unweighted_sum_and_fail_the_weighted_one(golden, spy, idx):
    c = golden("proofs_small.json")["small"][idx]
    row = _row(c)
    st, mega, _ = spy(row, c, b"\x05" * 32)
    assert st == OK and rs.pt_eq(mega, rs.IDENT)
    which = ("pair_small", "pair_252", "triple", "set32") if idx == 0 else ("pair_small", "pair_252", "triple")
    sets = fc.cancelling_sets(row, random.Random(100 + idx), which)
    assert len(sets) == 2 * len(which)
    for name, members in sets.items():
        res = []
        for i, m in enumerate(members):
            ent = hashlib.sha256(b"forgery-model %d %s %d" % (idx, name.encode(), i)).digest()  # a different verifier rng per member
            st, mega, rho = spy(m, c, ent)
            assert st == VERIFY, (name, i)
            assert not rs.pt_eq(mega, rs.IDENT), (name, i)
            res.append((mega, rho))
        assert len({rho for _, rho in res}) == len(res) and all(rho not in (0, 1) for _, rho in res)
        equal = rs.pt_eq(_sum(m for m, _ in res), rs.IDENT)
        weighted = rs.pt_eq(_sum(rs.pt_mul(rho, m) for m, rho in res), rs.IDENT)
        one_rho = rs.pt_eq(_sum(rs.pt_mul(res[0][1], m) for m, _ in res), rs.IDENT)
        print("%s %-12s members %2d  equal-weight sum is identity: %s  one shared weight: %s  per-proof weights: %s"
              % (c["name"], name, len(members), equal, one_rho, weighted))
        assert equal, name        # no weights, or rho = 1: the set would be accepted
        assert one_rho, name      # one weight for the whole group (every row reading one entropy row): accepted as well
        assert not weighted, name  # the weights the device draws: rejected


def test_same_entropy_gives_members_of_a_set_the_same_weight(golden, spy):
    """The control of the GPU tier rests on this: a and b are not in the transcript, so two members of a set that are given the
    same verifier entropy draw the same r and the same rho, and their weighted residuals cancel."""
    c = golden("proofs_small.json")["small"][0]
    for name, members in fc.cancelling_sets(_row(c), random.Random(7), ("pair_small",)).items():
        got = [spy(m, c, b"\x09" * 32) for m in members]
        assert got[0][2] == got[1][2]
        assert rs.pt_eq(_sum(rs.pt_mul(rho, m) for _, m, rho in got), rs.IDENT), name


@pytest.mark.parametrize("layout", ["compact", "two_phase"])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_sweep_python_and_c_oracle_agree_on_every_row(golden, oc, idx, layout):
    small = golden("proofs_small.json")["small"]
    c = small[idx]
    row = _row(c)
    # a donor of the same N: the same bid proved again under other entropy (other blindings, other points and scalars)
    ent = hashlib.sha512(b"forgery donor %d" % idx).digest() * 8
    f = lambda k: fc.i32(bytes.fromhex(c[k]))
    pub = [fc.i32(bytes.fromhex(p)) for p in c["pub_list"]]
    donor_rec = bb.prove(f("d"), f("k"), f("y"), f("y_inv"), f("q"), f("z_img"), f("seed"), pub, c["toggle"],
                         ent[:32 * (4 + c["N"]) + 32], c["rounds"], c["cap"]).to_record()
    donor = (donor_rec,) + row[1:]
    if layout == "two_phase":
        row, donor = fc.two_phase(row), fc.two_phase(donor)
    assert py_status(row, c["rounds"], c["cap"]) == OK and py_status(donor, c["rounds"], c["cap"]) == OK
    cases = fc.sweep(row, donor, c["toggle"])
    n_fields = len(fc.field_table(row))
    assert n_fields == (13 if layout == "compact" else 16) + 12 + 4 + c["N"] + 3 + c["N"]  # lg_n = 6 on the small circuits
    assert {cs.label.split(":")[0] for cs in cases if not cs.label.startswith("swap")} == {fl.name for fl in fc.field_table(row)}
    count = {OK: 0, VERIFY: 0, FORMAT: 0}
    for cs in cases:
        p = py_status(cs.row, c["rounds"], c["cap"])
        q = oc.verify(*cs.row, rounds=c["rounds"], cap=c["cap"])
        assert p == q, (cs.label, p, q)
        assert p in count
        if cs.differs:
            assert p != OK, cs.label
        else:
            assert p == OK, cs.label
        count[p] += 1
    print(c["name"], layout, "rows", len(cases), "OK %d VERIFY %d FORMAT %d" % (count[OK], count[VERIFY], count[FORMAT]))
    assert count[VERIFY] > 100
    assert count[FORMAT] == 16  # l and 2^256 - 1 in each of the five proof scalars, v + l and v + 2^255 in score, z_img and seed
    assert count[OK] == sum(1 for cs in cases if not cs.differs)


def test_expected_fallback_model():
    st = [0, 1, 0, 0, 3, 0, 1, 0, 0]
    early = [False, False, False, False, True, False, True, False, False]
    assert fc.expected_fallback(st, early, 1) == 0
    assert fc.expected_fallback(st, early, 3) == 3            # group 0 only: group 1 holds a format error, group 2 an early reject
    assert fc.expected_fallback(st, early, 4) == 4
    assert fc.expected_fallback(st, early, 1024) == 7
    assert fc.expected_fallback([0] * 9, [False] * 9, 3) == 0
