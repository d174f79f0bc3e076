"""not-gpu tier: selecting a round's bids (include/bbp.h bbp_prove_round_select, bbp_select_round_dev, bbp_debug_round_select).  The
rules as csrc/round_select.h states them (round_select_host), its compare helpers, screening, score record and staging layouts run in
tests/round_select_check.cpp, a stand-alone program under AddressSanitizer + UBSan; the expected selections come from the ten-line
model below (tests/round_select_cases.py), the expected score records from the big-int oracle (tests/prove_round_cases.py)."""
import os
import subprocess
import tempfile

import pytest

from tests import prove_round_cases as rc
from tests import round_select_cases as sc

OK, GENS_LEN, FORMAT, BAD_ARG = 0, 2, 3, 4


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_round_select_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "round_select_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def _select_cmd(scores, statuses, floor, K):
    return ["select %d %d %s" % (len(scores), K, sc.b32(floor).hex())] + ["%d %s" % (st, sc.b32(s).hex()) for s, st in zip(scores, statuses)]


def _parse_sel(line):
    f = line.split()
    assert f[0] == "sel"
    return [int(x) for x in f[3:]], int(f[1]), int(f[2])


def test_self_checks_of_helpers_and_layouts(check):
    assert check([]) == []


def test_round_select_host_against_the_model(check):
    cases = sc.host_cases()
    assert len(cases) > 60
    cmds = []
    for scores, statuses, floor, K in cases:
        cmds += _select_cmd(scores, statuses, floor, K)
    out = check(cmds)
    assert len(out) == len(cases)
    for line, (scores, statuses, floor, K) in zip(out, cases):
        assert _parse_sel(line) == sc.model(scores, statuses, floor, K), (scores, statuses, floor, K)


def test_model_on_hand_made_cases():
    """The model itself, on selections written out by hand (it decides every other case)."""
    st = [OK] * 5
    assert sc.model([5, 9, 9, 1, 7], st, 0, 2) == ([1, 2], 2, 5)            # a tie inside the selection
    assert sc.model([5, 9, 9, 1, 7], st, 0, 1) == ([1], 1, 5)               # a tie across the K-th place: the lower index
    assert sc.model([5, 9, 9, 1, 7], st, 6, 0) == ([1, 2, 4], 3, 3)         # K = 0: all of Q
    assert sc.model([5, 9, 9, 1, 7], [OK, BAD_ARG, OK, OK, FORMAT], 5, 9) == ([0, 2], 2, 2)
    assert sc.model([5, 9, 9, 1, 7], st, 10, 3) == ([], 0, 0)
    assert sc.model([5, 9, 9, 1, 7], st, 0, 3) == ([1, 2, 4], 3, 5)         # sel in index order, not rank order


@pytest.mark.parametrize("N,B", [(1, 3), (3, 5), (8, 5)])
def test_score_record_matches_the_oracle(check, N, B):
    r = rc.honest(N, B, tag=1)
    _check_scores(check, r)


def test_score_record_statuses(check):
    _check_scores(check, rc.status_round())
    _check_scores(check, rc.status_round(seed=rc.L))


def _check_scores(check, r):
    mimc = b"".join(rc.b32(c) for c in rc._C)
    out = check(["score %d %d %s %s %s" % (r.N, r.B, r.table.hex(), r.bid_bytes.hex(), mimc.hex())])
    assert len(out) == r.B
    for i, line in enumerate(out):
        st, toggle, w = r.expect[i]
        want_q = rc.b32(w["q"]) if st == OK else bytes(32)
        assert line.split() == ["rec", str(st), str(toggle if st == OK else 0), want_q.hex()], i


def test_header_formulas_binding_surface_and_screening_without_a_device(bbp, check):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_SELECT_MAX_BIDS (1u << 20)" in hdr and bbp.SELECT_MAX_BIDS == 1 << 20
    assert "Selecting a round's bids" in hdr
    for name in ("bbp_select_round_dev", "bbp_prove_round_select", "bbp_debug_round_select"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("prove_round_select", "select_round_dev", "debug_round_select"):
        assert callable(getattr(bbp.Context, name)), name
    assert "prove_round_select" in vars(bbp.Pool)
    assert bbp.select_floor(1) == b"\x01" + bytes(31) and bbp.select_floor((1 << 256) - 1) == b"\xff" * 32
    with pytest.raises(ValueError):
        bbp.select_floor(b"\x00" * 31)
    # the checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form
    lib = bbp.lib
    assert lib.bbp_prove_round_select(None, 8, 1, 1, 1, 1, 0, 0, None, None, None, 1, None, None, None, 1) == BAD_ARG
    assert lib.bbp_select_round_dev(None, 8, 1, 1, 1, 1, 0, 0, None, 1, 1, None, None, None, None, None) == BAD_ARG
    assert lib.bbp_debug_round_select(None, 1, 1, 1, 1, 0, 0, None, 1, 1) == BAD_ARG
    # ... and the checks on the numbers, in their order (csrc/round_select.h round_select_screen, what the entry point runs)
    out = check(["screen 0 %d" % (bbp.SELECT_MAX_BIDS + 1), "screen 203 %d" % (bbp.SELECT_MAX_BIDS + 1), "screen 202 %d" % (bbp.SELECT_MAX_BIDS + 1),
                 "screen 202 %d" % bbp.SELECT_MAX_BIDS, "screen 1 0", "screen 0 0", "screen 203 0"])
    assert out == ["screen %d 1" % BAD_ARG, "screen %d 1" % GENS_LEN, "screen %d 1" % BAD_ARG, "screen 0 0", "screen 0 1", "screen %d 1" % BAD_ARG,
                   "screen %d 1" % GENS_LEN]
