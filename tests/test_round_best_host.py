"""not-gpu tier: the best valid proofs of a round (include/bbp.h bbp_verify_round_best, bbp_verify_round_best_dev, bbp_debug_round_best).
The rules as csrc/round_best.h states them (round_best_host), the key screening, the tranche sizes, the ranking and the staging layouts
run in tests/round_best_check.cpp, a stand-alone program under AddressSanitizer + UBSan; the expected answers come from the
fifteen-line model of tests/round_best_cases.py, which is itself held to cases written out by hand."""
import os
import subprocess
import tempfile

import pytest

from tests import round_best_cases as bc

OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, SKIPPED = 0, 1, 2, 3, 4, -1
L = bc.L


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_round_best_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "round_best_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def test_model_on_hand_made_cases():
    """The model itself, on answers written out by hand (it decides every other case)."""
    keys = [5, 9, 9, 1, 7]
    ok = [OK] * 5
    # a tie inside a tranche: both 9s are examined together, the lower index ranks first
    assert bc.model(keys, ok, 0, 2, 2) == ([1, 2], 2, 5, 2, [SKIPPED, OK, OK, SKIPPED, SKIPPED])
    # a tie across a tranche boundary: tranche 0 is row 1 alone, the lower index
    assert bc.model(keys, ok, 0, 1, 1) == ([1], 1, 5, 1, [SKIPPED, OK, SKIPPED, SKIPPED, SKIPPED])
    # ... and when row 1 fails, tranche 1 (two rows) holds row 2 and row 4: 1 + 2 examined
    assert bc.model(keys, [OK, VERIFY, OK, OK, OK], 0, 1, 1) == ([2], 1, 5, 3, [SKIPPED, VERIFY, OK, SKIPPED, OK])
    # K == 0: one tranche of every candidate, all valid rows in rank order
    assert bc.model(keys, [OK, VERIFY, OK, FORMAT, OK], 5, 0, 1) == ([2, 4, 0], 3, 4, 4, [OK, VERIFY, OK, SKIPPED, OK])
    # K larger than the number of valid rows: everything is examined (T_0 = K = 4 rows, then the last one)
    assert bc.model(keys, [OK, VERIFY, VERIFY, OK, VERIFY], 0, 4, 1) == ([0, 3], 2, 5, 5, [OK, VERIFY, VERIFY, OK, VERIFY])
    # tranche < K: T_0 = K
    assert bc.model(keys, ok, 0, 3, 1) == ([1, 2, 4], 3, 5, 3, [SKIPPED, OK, OK, SKIPPED, OK])
    # every verdict bad
    assert bc.model(keys, [VERIFY, FORMAT] * 2 + [VERIFY], 0, 1, 2) == ([], 0, 5, 5, [VERIFY, FORMAT, VERIFY, FORMAT, VERIFY])
    # floor above every key; floor >= l
    assert bc.model(keys, ok, 10, 1, 1) == ([], 0, 0, 0, [SKIPPED] * 5)
    assert bc.model(keys, ok, L, 0, 1) == ([], 0, 0, 0, [SKIPPED] * 5)
    # a key >= l below a floor >= l is FORMAT, not SKIPPED; l - 1 is the highest candidate there is
    assert bc.model([L, L - 1, bc.ALL_ONES, 3], ok[:4], L + 1, 1, 1) == ([], 0, 0, 0, [FORMAT, SKIPPED, FORMAT, SKIPPED])
    assert bc.model([L, L - 1, bc.ALL_ONES, 3], ok[:4], 0, 1, 1) == ([1], 1, 2, 1, [FORMAT, OK, FORMAT, SKIPPED])
    # tranche >= B: one tranche
    assert bc.model(keys, [OK, VERIFY, VERIFY, OK, OK], 0, 1, 64) == ([4], 1, 5, 5, [OK, VERIFY, VERIFY, OK, OK])
    # tranche 0 is the default
    assert bc.model(list(range(100)), [VERIFY] * 100, 0, 1, 0)[3] == 100 and bc.model(list(range(100)), [OK] * 100, 0, 1, 0)[3] == bc.TRANCHE_DEFAULT
    assert [bc.max_tranches(n, 4) for n in (0, 1, 4, 5, 12, 13, 28, 29)] == [0, 1, 1, 2, 2, 3, 3, 4]


def test_self_checks_of_helpers_and_layouts(check):
    assert check([]) == []


def _best_cmd(keys, verdicts, floor, K, tranche, cap):
    return ["best %d %d %d %d %s" % (len(keys), K, tranche, cap, bc.b32(floor).hex())] + ["%d %s" % (v, bc.b32(k).hex()) for k, v in zip(keys, verdicts)]


def _parse_best(line):
    head, best, status = line.split("|")
    f = head.split()
    assert f[0] == "best"
    return [int(x) for x in best.split()], int(f[1]), int(f[2]), int(f[3]), [int(x) for x in status.split()]


def test_round_best_host_against_the_model(check):
    cases = bc.host_cases()
    assert len(cases) > 60
    caps = [len(c[0]) if n % 3 else 2 for n, c in enumerate(cases)]  # every third case: room for two entries only
    cmds = []
    for (keys, verdicts, floor, K, tranche), cap in zip(cases, caps):
        cmds += _best_cmd(keys, verdicts, floor, K, tranche, cap)
    out = check(cmds)
    assert len(out) == len(cases)
    seen_stop_early = seen_all = 0
    for line, (keys, verdicts, floor, K, tranche), cap in zip(out, cases, caps):
        best, n_best, n_cand, n_exam, status = bc.model(keys, verdicts, floor, K, tranche)
        assert _parse_best(line) == (best[:cap], n_best, n_cand, n_exam, status), (keys, verdicts, floor, K, tranche)
        seen_stop_early += n_exam < n_cand
        seen_all += n_cand > 0 and n_exam == n_cand
    assert seen_stop_early > 10 and seen_all > 10


def test_key_screening_and_ranking(check):
    out = check(["key %s %s" % (bc.b32(k).hex(), bc.b32(f).hex())
                 for k, f in ((L - 1, 0), (L, 0), (bc.ALL_ONES, 0), (L, bc.ALL_ONES), (L - 1, L), (5, 5), (4, 5), (0, 0), (1 << 255, 0), (1 << 224, (1 << 224) + 1))])
    assert out == ["key %d" % s for s in (OK, FORMAT, FORMAT, FORMAT, SKIPPED, OK, SKIPPED, OK, FORMAT, SKIPPED)]
    # pairs in any order -> rank order: key descending (the most significant word decides), then index ascending
    pairs = [(7, (1 << 224) + 5), (2, (2 << 224) + 1), (9, 3), (4, (2 << 224) + 1), (0, (1 << 224) + 9)]
    cmd = ["rank %d %d" % (len(pairs), 5)] + ["%d %s" % (i, bc.b32(k).hex()) for i, k in pairs]
    assert check(cmd) == ["rank 2 4 0 7 9"]
    cmd[0] = "rank 5 2"
    assert check(cmd) == ["rank 2 4"]


def test_header_binding_surface_and_screening_without_a_device(bbp, check):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_ROW_SKIPPED (-1)" in hdr and bbp.ROW_SKIPPED == -1
    assert "#define BBP_BEST_TRANCHE_DEFAULT %du" % bbp.BEST_TRANCHE_DEFAULT in hdr and bbp.BEST_TRANCHE_DEFAULT == bc.TRANCHE_DEFAULT
    assert hdr.index("Selecting a round's bids") < hdr.index("Best valid proofs of a round")
    assert "At most n_candidates rows are verified" in hdr and "ceil(log2(n_candidates / T_0 + 1)) tranches" in hdr
    for name in ("bbp_verify_round_best", "bbp_verify_round_best_dev", "bbp_debug_round_best"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("verify_round_best", "verify_round_best_dev", "debug_round_best"):
        assert callable(getattr(bbp.Context, name)), name
    assert "verify_round_best" in vars(bbp.Pool)
    # the checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form
    lib = bbp.lib
    assert lib.bbp_verify_round_best(None, 8, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_verify_round_best_dev(None, 8, 1, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, None) == BAD_ARG
    assert lib.bbp_debug_round_best(None, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1) == BAD_ARG
    # ... and the checks on the numbers, in their order (what the entry points run: csrc/round_select.h round_select_screen)
    top = bbp.SELECT_MAX_BIDS
    out = check(["screen 0 %d" % (top + 1), "screen 203 %d" % (top + 1), "screen 202 %d" % (top + 1), "screen 202 %d" % top, "screen 1 0", "screen 0 0",
                 "screen 203 0"])
    assert out == ["screen %d 1" % BAD_ARG, "screen %d 1" % GENS_LEN, "screen %d 1" % BAD_ARG, "screen 0 0", "screen 0 1", "screen %d 1" % BAD_ARG,
                   "screen %d 1" % GENS_LEN]
