"""not-gpu tier: the EXPANDED blinding draw (include/bbp.h bbp_set_blinding_draw).

Draws and fixture: the host restatement csrc/blinding_expand.h (tests/blinding_expand_check.cpp, a stand-alone program under
AddressSanitizer + UBSan) against the Python model tests/expanded_draw_model.py; tests/golden/proofs_expanded_draw.json against the model,
the unmodified Python verifier and the C oracle.

Plan: csrc/prove_plan.h through tests/expanded_plan_check.cpp.  With the setting at MERLIN every plan and trace line of the sweep equals
what the header gave before it knew the setting (PARENT_PLANS, printed by the same program built over the parent commit's header); with
EXPANDED the chain is EXPANDED, the draw buffer 32 B bytes, and everything that places the call is as under MERLIN."""
import subprocess

import pytest

from oracle.ref_py import blindbid as bb, ristretto as rs
from tests import expanded_draw_model as model, oracle_c

EXPANDED = 4  # ProvePlan::Chain


@pytest.fixture(scope="module")
def cases(golden):
    return golden("proofs_expanded_draw.json")["expanded_draw"]


@pytest.fixture(scope="module")
def oc(built):
    return oracle_c.load(built.build_oracle())


def _h(c, k):
    return bytes.fromhex(c[k])


def _i(c, k):
    return int.from_bytes(_h(c, k), "little")


def _pub(c):
    return b"".join(bytes.fromhex(p) for p in c["pub_list"])


def _s7(c):
    return b"".join(_h(c, k) for k in ["d", "k", "y", "y_inv", "q", "z_img", "seed"])


def _model_rng(c):
    """the prover's transcript up to its rng, from a fixture record's commitments and entropy: the model's ExpandedRng"""
    m, rec, ent = 4 + c["N"], _h(c, "record"), _h(c, "entropy")
    V = [rec[len(rec) - 32 * m + 32 * i:len(rec) - 32 * m + 32 * i + 32] for i in range(m)]
    t = model.ExpandedDrawTranscript()
    t.append_message(b"dom-sep", b"r1cs v1")
    for v in V:
        t.append_message(b"V", v)
    t.append_u64(b"m", m)
    return t.build_rng([(b"v_blinding", ent[32 * i:32 * i + 32]) for i in range(m)], ent[32 * m:]), b"".join(V)


@pytest.mark.parametrize("name", ["xd_n1", "xd_n202"])
def test_host_restatement_equals_model(built, cases, name):
    c = next(x for x in cases if x["name"] == name)
    m, n1, p = 4 + c["N"], c["n_mul"], 5
    assert n1 == model.n_mul_of(c["N"]) == {1: 1445, 202: 2048}[c["N"]]
    rng, V = _model_rng(c)
    js = [0, 1, 2, 3, 3 + n1 - 1, 3 + n1, 2 + 2 * n1]
    ent = _h(c, "entropy")
    out = subprocess.run([built.build_blinding_expand_check(), str(m), str(n1), str(p), V.hex(), ent[:32 * m].hex(), ent[32 * m:].hex()] + [str(j) for j in js],
                         capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "key " + rng.key.hex() and rng.key.hex() == c["draw_key"]
    for line, j in zip(out[1:], js):
        slot = (0, p * (1 + 2 * n1)) if j == 0 else (1, p * (1 + n1)) if j == 1 else (2, p * (1 + 2 * n1) + j - 2)
        assert line == "draw %d %s %d %d" % (j, rs.sc_bytes(rs.sc_wide(model.draw_bytes(rng.key, j))).hex(), slot[0], slot[1]), j
    for _ in range(3 + 2 * n1):
        rng.fill_bytes(64)
    assert out[1 + len(js)] == "next " + rng.fill_bytes(64).hex()  # the t blindings go on in the TranscriptRng, after the key squeeze
    # a draw beyond the last is refused, not computed
    assert subprocess.run([built.build_blinding_expand_check(), str(m), str(n1), "0", V.hex(), ent[:32 * m].hex(), ent[32 * m:].hex(), str(3 + 2 * n1)]).returncode == 2


def test_chacha_block_rfc8439():
    """RFC 8439 section 2.3.2: the model's block function"""
    key = bytes(range(32))
    nonce = (0x09000000, 0x4a000000, 0x00000000)
    assert model.chacha20_block(key, 1, nonce).hex() == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                                                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_fixture_n1_regenerated_from_model(cases, monkeypatch):
    """the one slow test (about 20 s): the big-int prover with the model's transcript gives the fixture's N = 1 record"""
    c = cases[0]
    assert c["name"] == "xd_n1"
    monkeypatch.setattr(bb, "new_transcript", model.ExpandedDrawTranscript)
    pr = bb.prove(_i(c, "d"), _i(c, "k"), _i(c, "y"), _i(c, "y_inv"), _i(c, "q"), _i(c, "z_img"), _i(c, "seed"),
                  [int.from_bytes(bytes.fromhex(p), "little") for p in c["pub_list"]], c["toggle"], _h(c, "entropy"))
    assert pr.to_record().hex() == c["record"]


def test_fixture_records_verify(cases, oc):
    assert [(c["name"], c["N"]) for c in cases] == [("xd_n1", 1), ("xd_n8_a", 8), ("xd_n8_b", 8), ("xd_n8_c", 8), ("xd_n202", 202)]
    assert len({c["entropy"] for c in cases if c["N"] == 8}) == 3
    for c in cases:
        rec = _h(c, "record")
        assert len(rec) == 1121 + 32 * (4 + c["N"])
        pub_int = [int.from_bytes(bytes.fromhex(p), "little") for p in c["pub_list"]]
        assert bb.verify(bb.Proof.from_record(rec, c["N"]), _i(c, "q"), _i(c, "z_img"), _i(c, "seed"), pub_int), c["name"]
        assert oc.verify(rec, _h(c, "q"), _h(c, "z_img"), _h(c, "seed"), _pub(c)) == 0, c["name"]


def test_fixture_commitments_equal_merlin_record(cases, oc):
    """same inputs and entropy through the C oracle (the merlin draw): the 4 + N commitments are equal, A_I1, A_O1 and S1 are not"""
    for c in cases:
        rc, mrec = oc.prove(_s7(c), _pub(c), c["toggle"], _h(c, "entropy"))
        assert rc == 0
        rec, m = _h(c, "record"), 4 + c["N"]
        assert len(mrec) == len(rec) and rec[-32 * m:] == mrec[-32 * m:], c["name"]
        for k in range(3):  # version byte, then A_I1, A_O1, S1
            assert rec[1 + 32 * k:33 + 32 * k] != mrec[1 + 32 * k:33 + 32 * k], (c["name"], k)


# ---- plan ------------------------------------------------------------------------------------------------------------------------------
def sweep():
    """the arguments of expanded_plan_check's `plan` after DRAW: B INFLIGHT BUSY DEEP_MODE LAST_SLICED CALLS N1 HWQ [NAME TEXT]..."""
    rows = []
    for B in (1, 32, 33, 64, 130, 192, 768, 769, 1023, 1024, 2300, 2301, 4096, 4097):
        for inflight in (0, 1, 3):
            rows.append("%d %d %d %d %d 7 1466 4" % (B, inflight, inflight > 0, inflight >= 3, inflight > 0))
    for knobs in ("BBP_RNG_COOP 0", "BBP_RNG_DPP 1 BBP_SLICES 4 BBP_TR_WAVE_BELOW 64", "BBP_RNG_COOP 1 BBP_RNG_DPP 0 BBP_SERIAL_LDS 0 BBP_RNG_BLOCK 512"):
        for B in (1, 33, 64, 769, 1024, 4097):
            for inflight in (0, 3):
                rows.append("%d %d 0 %d 0 2 2048 4 %s" % (B, inflight, inflight >= 3, knobs))
    rows += ["64 3 0 1 0 5 1445 8", "1024 3 0 1 0 6 1445 8", "1024 1 1 0 1 3 1445 8 BBP_OPEN_ON_CHAIN 1"]
    return rows


PARENT_PLANS = """
7 0 0 1 1 2 1 3 2 64 64 1 2 0 0 -1 73 1 187840 | prove call 7: B 1 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 2 64 64 1 2 0 0 -1 73 1 187840 | prove call 7: B 1 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 2 64 64 1 2 0 1 3 9 3 187840 | prove call 7: B 1 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 2 64 64 1 2 0 0 -1 73 1 6010880 | prove call 7: B 32 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 2 64 64 1 2 0 0 -1 73 1 6010880 | prove call 7: B 32 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 2 64 64 1 2 0 1 3 9 3 6010880 | prove call 7: B 32 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 64 1 2 0 0 -1 73 1 6198720 | prove call 7: B 33 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 64 1 2 0 0 -1 73 1 6198720 | prove call 7: B 33 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 1 64 64 1 2 0 1 3 9 3 6198720 | prove call 7: B 33 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 64 1 2 0 0 -1 73 1 12021760 | prove call 7: B 64 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 64 1 2 0 0 -1 73 1 12021760 | prove call 7: B 64 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 1 64 64 1 2 0 1 3 9 3 12021760 | prove call 7: B 64 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 128 1 2 0 0 -1 73 1 24419200 | prove call 7: B 130 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 128 1 2 0 0 -1 73 1 24419200 | prove call 7: B 130 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 1 64 128 1 2 0 1 3 9 3 24419200 | prove call 7: B 130 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 128 1 2 0 0 -1 73 1 36065280 | prove call 7: B 192 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 128 1 2 0 0 -1 73 1 36065280 | prove call 7: B 192 inflight 1 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 1 0 1 1 2 1 3 1 64 128 1 2 0 1 3 9 3 36065280 | prove call 7: B 192 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 256 1 2 0 0 -1 73 1 144261120 | prove call 7: B 768 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 1 0 0 1 1 3 1 64 256 0 0 3 0 -1 15 0 144261120 0 256 512 768 | prove call 7: B 768 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 1
7 1 0 1 1 2 1 3 1 64 256 1 2 0 1 3 9 3 144261120 | prove call 7: B 768 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 0 1 1 2 1 3 1 64 256 1 2 0 0 -1 73 1 144448960 | prove call 7: B 769 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 144448960 0 256 512 769 | prove call 7: B 769 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 144448960 | prove call 7: B 769 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 1 1 2 1 3 1 64 256 1 2 0 0 -1 73 1 192160320 | prove call 7: B 1023 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 192160320 0 341 682 1023 | prove call 7: B 1023 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 192160320 | prove call 7: B 1023 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 0 0 1 1 3 1 64 256 0 0 3 0 -1 15 0 192348160 0 341 682 1024 | prove call 7: B 1024 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 1 coop 1
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 192348160 0 341 682 1024 | prove call 7: B 1024 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 192348160 | prove call 7: B 1024 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 0 0 1 1 3 1 64 256 0 0 3 0 -1 15 0 432032000 0 766 1533 2300 | prove call 7: B 2300 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 1 coop 1
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 432032000 0 766 1533 2300 | prove call 7: B 2300 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 432032000 | prove call 7: B 2300 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 432219840 0 767 1534 2301 | prove call 7: B 2301 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 1 coop 0
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 432219840 0 767 1534 2301 | prove call 7: B 2301 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 432219840 | prove call 7: B 2301 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 769392640 0 1365 2730 4096 | prove call 7: B 4096 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 1 coop 0
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 769392640 0 1365 2730 4096 | prove call 7: B 4096 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 1 0 1 1 2 0 0 0 64 256 1 2 0 1 3 9 3 769392640 | prove call 7: B 4096 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
7 0 0 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 769580480 0 1365 2731 4097 | prove call 7: B 4097 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 1 coop 0
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 769580480 0 1365 2731 4097 | prove call 7: B 4097 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
7 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 769580480 0 1365 2731 4097 | prove call 7: B 4097 inflight 3 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
2 0 0 1 0 2 0 0 0 64 64 1 3 0 0 -1 19 0 262336 | prove call 2: B 1 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 1 0 1 0 2 0 0 0 64 64 1 3 0 1 1 3 0 262336 | prove call 2: B 1 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 1 0 2 0 0 0 64 64 1 3 0 0 -1 19 0 8657088 | prove call 2: B 33 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 1 0 1 0 2 0 0 0 64 64 1 3 0 1 1 3 0 8657088 | prove call 2: B 33 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 1 0 2 0 0 0 64 64 1 3 0 0 -1 19 0 16789504 | prove call 2: B 64 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 1 0 1 0 2 0 0 0 64 64 1 3 0 1 1 3 0 16789504 | prove call 2: B 64 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 1 0 2 0 0 0 64 256 1 3 0 0 -1 19 0 201736384 | prove call 2: B 769 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 1 0 1 0 2 0 0 0 64 256 1 3 0 1 1 3 0 201736384 | prove call 2: B 769 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 0 0 0 0 0 0 64 256 0 0 3 0 -1 15 0 268632064 0 341 682 1024 | prove call 2: B 1024 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 0
2 1 0 1 0 2 0 0 0 64 256 1 3 0 1 1 3 0 268632064 | prove call 2: B 1024 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 0 0 0 0 0 0 64 256 0 0 3 0 -1 15 0 1074790592 0 1365 2731 4097 | prove call 2: B 4097 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 0
2 0 0 0 0 0 0 0 0 64 256 0 0 3 0 -1 15 0 1074790592 0 1365 2731 4097 | prove call 2: B 4097 inflight 3 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 0
2 0 0 1 0 2 1 2 2 64 64 1 3 0 0 -1 19 0 262336 | prove call 2: B 1 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 2 2 64 64 1 3 0 1 1 3 0 262336 | prove call 2: B 1 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 2 2 64 64 1 3 0 0 -1 19 0 8657088 | prove call 2: B 33 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 2 2 64 64 1 3 0 1 1 3 0 8657088 | prove call 2: B 33 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 2 2 64 64 1 3 0 0 -1 19 0 16789504 | prove call 2: B 64 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 2 2 64 64 1 3 0 1 1 3 0 16789504 | prove call 2: B 64 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 2 1 64 256 1 3 0 0 -1 19 0 201736384 | prove call 2: B 769 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 0 0 0 64 256 1 3 0 1 1 3 0 201736384 | prove call 2: B 769 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 0 0 0 1 2 1 64 256 0 0 4 0 -1 31 0 268632064 0 256 512 768 1024 | prove call 2: B 1024 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 1
2 1 0 1 0 2 0 0 0 64 256 1 3 0 1 1 3 0 268632064 | prove call 2: B 1024 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 0
2 0 0 0 0 0 0 0 0 64 256 0 0 4 0 -1 31 0 1074790592 0 1024 2048 3072 4097 | prove call 2: B 4097 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 0
2 0 0 0 0 0 0 0 0 64 256 0 0 4 0 -1 31 0 1074790592 0 1024 2048 3072 4097 | prove call 2: B 4097 inflight 3 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 0
2 0 0 1 0 2 1 1 2 64 512 1 3 0 0 -1 19 0 262336 | prove call 2: B 1 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 1 2 64 512 1 3 0 1 1 3 0 262336 | prove call 2: B 1 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 1 1 64 512 1 3 0 0 -1 19 0 8657088 | prove call 2: B 33 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 1 1 64 512 1 3 0 1 1 3 0 8657088 | prove call 2: B 33 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 1 1 64 512 1 3 0 0 -1 19 0 16789504 | prove call 2: B 64 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 1 1 64 512 1 3 0 1 1 3 0 16789504 | prove call 2: B 64 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 1 0 2 1 1 1 64 512 1 3 0 0 -1 19 0 201736384 | prove call 2: B 769 inflight 0 deep 0 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 1 0 1 0 2 1 1 1 64 512 1 3 0 1 1 3 0 201736384 | prove call 2: B 769 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 0 0 0 1 1 1 64 512 0 0 3 0 -1 15 0 268632064 0 341 682 1024 | prove call 2: B 1024 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 1
2 1 0 1 0 2 1 1 1 64 512 1 3 0 1 1 3 0 268632064 | prove call 2: B 1024 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 2 coop 1
2 0 0 0 0 0 1 1 1 64 512 0 0 3 0 -1 15 0 1074790592 0 1365 2731 4097 | prove call 2: B 4097 inflight 0 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 1
2 0 0 0 0 0 1 1 1 64 512 0 0 3 0 -1 15 0 1074790592 0 1365 2731 4097 | prove call 2: B 4097 inflight 3 deep 0 behind_sliced 0 dual 0 rotate 0 par 0 coop 1
5 1 0 1 1 0 1 3 1 64 64 1 3 0 0 -1 81 1 11849728 | prove call 5: B 64 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 0 coop 1
6 1 0 1 0 1 0 0 0 64 256 1 1 0 0 -1 7 0 189595648 | prove call 6: B 1024 inflight 3 deep 1 behind_sliced 0 dual 1 rotate 1 par 1 coop 0
3 0 1 0 0 1 0 0 0 64 256 0 0 3 0 -1 15 0 189595648 0 341 682 1024 | prove call 3: B 1024 inflight 1 deep 0 behind_sliced 1 dual 0 rotate 0 par 1 coop 0
"""


def _plans(built, draw):
    text = "".join("plan %d %s\n" % (draw, r) for r in sweep())
    out = subprocess.run([built.build_expanded_plan_check()], input=text, capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")
    assert lines[-1] == "" and len(lines) == len(sweep()) + 1
    return lines[:-1]


def test_plan_merlin_is_the_parents(built):
    assert _plans(built, 0) == PARENT_PLANS.strip("\n").split("\n")


def test_plan_expanded(built):
    names = ("call deep behind_sliced dual open_stream par coop chain prefix_form serial_blk cblk rotate heavy_stream slices open_on_chain chain_stream "
             "roles raw_index raw_bytes").split()
    for row, ml, xl in zip(sweep(), _plans(built, 0), _plans(built, 1)):
        B = int(row.split()[0])
        tr_wave_below = 64 if "BBP_TR_WAVE_BELOW 64" in row else 32
        (mv, mt), (xv, xt) = (l.split(" | ") for l in (ml, xl))
        mv, xv = mv.split(), xv.split()
        md, xd = dict(zip(names, mv)), dict(zip(names, xv))
        assert int(xd["chain"]) == EXPANDED and int(md["chain"]) != EXPANDED, row
        assert int(xd["raw_bytes"]) == 32 * B and int(md["raw_bytes"]) == 64 * B * (3 + 2 * int(row.split()[6])), row
        assert int(xd["prefix_form"]) == (2 if B <= tr_wave_below else 1), row
        for k in names:  # streams, rotation, slices, par, raw_index: decided exactly as under MERLIN
            if k not in ("coop", "chain", "prefix_form", "raw_bytes"):
                assert xd[k] == md[k], (row, k)
        assert xv[len(names):] == mv[len(names):], row  # the slice bounds
        assert xd["coop"] == "0" and xt == mt.rsplit(" coop ", 1)[0] + " coop 0 draw expanded", row
        assert not mt.endswith("draw expanded")
