"""not-gpu tier: the best valid proofs of many rounds (include/bbp.h bbp_verify_rounds_best, bbp_verify_rounds_best_dev,
bbp_debug_rounds_best).  The rules as csrc/rounds_best.h states them (rounds_best_host), the extended-key comparison, the radix select
as the kernel runs it, the state layout and the screening order run in tests/rounds_best_check.cpp, a stand-alone program under
AddressSanitizer + UBSan; the expected answers come from the model of tests/rounds_best_cases.py, which is itself held to cases written
out by hand."""
import os
import subprocess
import tempfile

import pytest

from tests import round_best_cases as bc
from tests import rounds_best_cases as mc

OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, SKIPPED = 0, 1, 2, 3, 4, -1
L = bc.L


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_rounds_best_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "rounds_best_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def test_model_on_hand_made_cases():
    """The model itself, on answers written out by hand (it decides every other case)."""
    #        row:  0  1  2  3  4  5  6  7  8
    round_of = [0, 1, 0, 1, 0, 1, 0, 1, 0]
    keys = [9, 9, 8, 7, 7, 5, 6, 3, 5]
    # two rounds that stop at different steps (K = 1, tranche 1): round 0's top claim holds, one step; round 1's first two tranches
    # (row 1, then rows 3 and 5) fail and row 7 holds in the third
    v = [OK, VERIFY, OK, VERIFY, OK, FORMAT, OK, OK, OK]
    assert mc.model(2, round_of, keys, v, None, 1, 1) == ([[0], [7]], [1, 1], [5, 4], [1, 4], 3,
                                                          [OK, VERIFY, SKIPPED, VERIFY, SKIPPED, FORMAT, SKIPPED, OK, SKIPPED])
    # ... the same with tranche 4: one step, each round's first four candidates
    assert mc.model(2, round_of, keys, v, None, 1, 4) == ([[0], [7]], [1, 1], [5, 4], [4, 4], 1,
                                                          [OK, VERIFY, OK, VERIFY, OK, FORMAT, OK, OK, SKIPPED])
    # a round with no row (round 2 of 3) reports zeros; K = 2 with tranche 1: T_0 = 2
    assert mc.model(3, round_of, keys, [OK] * 9, None, 2, 1) == ([[0, 2], [1, 3], []], [2, 2, 0], [5, 4, 0], [2, 2, 0], 1,
                                                                 [OK, OK, OK, OK, SKIPPED, SKIPPED, SKIPPED, SKIPPED, SKIPPED])
    # a round whose every key is >= l: FORMAT, no candidate, no step of its own
    k2 = [9, L, 8, L + 1, 7, bc.ALL_ONES, 6, L, 5]
    assert mc.model(2, round_of, k2, [OK] * 9, None, 1, 1) == ([[0], []], [1, 0], [5, 0], [1, 0], 1,
                                                               [OK, FORMAT, SKIPPED, FORMAT, SKIPPED, FORMAT, SKIPPED, FORMAT, SKIPPED])
    # a round whose floor is >= l: every row SKIPPED (a key >= l stays FORMAT); the other round's floor 7 admits rows 0, 2, 4
    assert mc.model(2, round_of, keys, [VERIFY] * 9, [7, L], 1, 1) == ([[], []], [0, 0], [3, 0], [3, 0], 2,
                                                                        [VERIFY, SKIPPED, VERIFY, SKIPPED, VERIFY, SKIPPED, SKIPPED, SKIPPED, SKIPPED])
    # K = 0: one step that holds every candidate of every round; all valid rows in rank order
    assert mc.model(2, round_of, keys, v, [6, 0], 0, 1) == ([[0, 2, 4, 6], [7]], [4, 1], [4, 4], [4, 4], 1,
                                                            [OK, VERIFY, OK, VERIFY, OK, FORMAT, OK, OK, SKIPPED])
    # nothing to do at all: no step
    assert mc.model(2, round_of, keys, v, [L, L], 1, 1)[4] == 0
    assert [mc.tranches_run(10, e, 1, 1) for e in (0, 1, 3, 7, 10)] == [0, 1, 2, 3, 4] and mc.tranches_run(10, 10, 0, 1) == 1


def test_self_checks_of_helpers_select_and_layout(check):
    assert check([]) == []


def _bests_cmd(R, round_of, keys, verdicts, floors, K, tranche, cap):
    return (["bests %d %d %d %d %d %d" % (R, len(keys), K, tranche, cap, 1 if floors else 0)] + [bc.b32(f).hex() for f in (floors or [])] +
            ["%d %d %s" % (r, v, bc.b32(k).hex()) for r, k, v in zip(round_of, keys, verdicts)])


def _parse_bests(line, R):
    head, status = line.split("|#|")
    parts = head.split("|")
    assert parts[0].split()[0] == "bests" and len(parts) == R + 1
    per = [[int(x) for x in p.split()] for p in parts[1:]]
    return ([p[3:] for p in per], [p[0] for p in per], [p[1] for p in per], [p[2] for p in per], int(parts[0].split()[1]), [int(x) for x in status.split()])


def test_rounds_best_host_against_the_model(check):
    cases = mc.host_cases()
    assert len(cases) >= 60
    caps = [len(c[2]) if n % 3 else 1 for n, c in enumerate(cases)]  # every third case: room for one entry per round only
    cmds = []
    for (R, ro, keys, verdicts, floors, K, tranche), cap in zip(cases, caps):
        cmds += _bests_cmd(R, ro, keys, verdicts, floors, K, tranche, cap)
    out = check(cmds)
    assert len(out) == len(cases)
    several_steps = uneven = empty = 0
    for line, (R, ro, keys, verdicts, floors, K, tranche), cap in zip(out, cases, caps):
        best, n_best, n_cand, n_exam, steps, status = mc.model(R, ro, keys, verdicts, floors, K, tranche)
        assert _parse_bests(line, R) == ([b[:cap] for b in best], n_best, n_cand, n_exam, steps, status), (R, ro, keys, verdicts, floors, K, tranche)
        ran = [mc.tranches_run(c, e, K, tranche) for c, e in zip(n_cand, n_exam)]
        several_steps += steps > 1
        uneven += len({t for t in ran if t}) > 1
        empty += 0 in n_cand
    assert several_steps > 10 and uneven > 10 and empty > 10


def test_header_binding_surface_and_screening_without_a_device(bbp, check):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_BEST_MAX_ROUNDS (1u << 16)" in hdr and bbp.BEST_MAX_ROUNDS == 1 << 16
    assert hdr.index("Best proofs of a round, one per bidder") < hdr.index("Best valid proofs of many rounds") < hdr.index("bbp_verify_rounds_best(")
    assert "A round that no row names reports zeros" in hdr and "never on timing" in hdr
    for name in ("bbp_verify_rounds_best", "bbp_verify_rounds_best_dev", "bbp_debug_rounds_best"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("verify_rounds_best", "verify_rounds_best_dev", "debug_rounds_best"):
        assert callable(getattr(bbp.Context, name)), name
    assert "verify_rounds_best" in vars(bbp.Pool) and "verify_rounds_best_dev" not in vars(bbp.Pool)
    # the checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form
    lib = bbp.lib
    assert lib.bbp_verify_rounds_best(None, 1, 1, 1, 1, 1, 1, None, 1, 1, 0, None, 1, 1, 1, None, 1) == BAD_ARG
    assert lib.bbp_verify_rounds_best_dev(None, 1, 1, 1, 1, 1, 1, 1, None, 1, 1, 0, None, 1, 1, 1, None, 1, None) == BAD_ARG
    assert lib.bbp_debug_rounds_best(None, 1, 1, 1, 1, 1, None, 1, 1, 0, None, 1, 1, 1, None, 1) == BAD_ARG
    # ... and the checks on the numbers, in their order (what the entry points run: csrc/rounds_best.h rounds_best_screen)
    top, rmax = bbp.SELECT_MAX_BIDS, bbp.BEST_MAX_ROUNDS
    out = check(["screen 0 %d 0 5" % (top + 1),            # R == 0 before everything
                 "screen %d 1 8 0" % (rmax + 1),           # R above the limit (round_Ns is not looked at)
                 "screen 2 %d 203,0 5,5" % (top + 1),      # a 0 in round_Ns before an entry above BBP_MAX_ITEMS, wherever they are
                 "screen 2 %d 203,8 5,5" % (top + 1),      # GENS_LEN before B
                 "screen 2 %d 8,8 5,5" % (top + 1),        # B before round_of
                 "screen 2 0 8,8 -",                       # B == 0: done, round_of not looked at
                 "screen 2 0 203,8 -",                     # ... but the table is
                 "screen 2 2 8,8 -",                       # round_of NULL with R > 1
                 "screen 1 2 8 -",                         # ... is fine with one round
                 "screen 2 3 8,202 0,1,2",                 # round_of[i] >= R
                 "screen 2 3 8,202 0,1,1"])
    assert out == ["screen %d 1" % BAD_ARG, "screen %d 1" % BAD_ARG, "screen %d 1" % BAD_ARG, "screen %d 1" % GENS_LEN, "screen %d 1" % BAD_ARG, "screen 0 1",
                   "screen %d 1" % GENS_LEN, "screen %d 1" % BAD_ARG, "screen 0 0", "screen %d 1" % BAD_ARG, "screen 0 0"]
