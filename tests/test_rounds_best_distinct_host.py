"""not-gpu tier: the best proofs of many rounds, one per bidder (include/bbp.h bbp_verify_rounds_best_distinct, its _dev form,
bbp_debug_rounds_best_distinct).  The rules as csrc/rounds_best_distinct.h states them (rounds_best_distinct_host), the identity table with
identities that belong to a round, the per-step plan and the extra layout run in tests/rounds_best_distinct_check.cpp, a stand-alone program
under AddressSanitizer + UBSan; the expected answers come from the model of tests/rounds_best_distinct_cases.py, which is itself held to
cases written out by hand."""
import os
import random
import subprocess
import tempfile

import pytest

from tests import round_best_cases as bc
from tests import round_best_distinct_cases as dc
from tests import rounds_best_distinct_cases as mdc

OK, VERIFY, GENS_LEN, FORMAT, BAD_ARG, SKIPPED, DUPLICATE = 0, 1, 2, 3, 4, -1, -2
L = bc.L


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_rounds_best_distinct_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "rounds_best_distinct_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def test_model_on_hand_made_cases():
    """The model itself, on answers written out by hand (it decides every other case)."""
    for (verdicts, K, tranche), (best, n_cand, n_exam, n_dups, steps, status) in mdc.HAND_CASES:
        got = mdc.model(2, mdc.HAND_ROUND_OF, mdc.HAND_KEYS, mdc.HAND_IDS, verdicts, None, K, tranche)
        assert got[:7] == (best, [len(b) for b in best], n_cand, n_exam, n_dups, steps, status), (K, tranche)
    # case 3: the rounds stop at different steps, and the stopped round's settled id sits on a row that stays SKIPPED
    assert mdc.model(2, mdc.HAND_ROUND_OF, mdc.HAND_KEYS, mdc.HAND_IDS, mdc.HAND_ROW1_BAD, None, 1, 1)[7] == [1, 2]
    # a round of 7 candidates, T_0 = 3, whose first tranche settles the id of all the rest: one step, 3 examined, 4 dropped, K not reached;
    # round 1 is named by no row
    a, b = b"a" * 32, b"b" * 32
    got = mdc.model(2, [0] * 7, [9, 8, 7, 6, 5, 4, 3], [a, b, b, b, b, b, b], [VERIFY, OK, OK] + [OK] * 4, None, 3, 1)
    assert got[:7] == ([[1], []], [1, 0], [7, 0], [3, 0], [4, 0], 1, [VERIFY, OK, OK] + [DUPLICATE] * 4)
    got = mdc.model(2, [0] * 7, [9, 8, 7, 6, 5, 4, 3], [a, b, a, b, b, b, b], [OK, OK, OK] + [OK] * 4, None, 3, 1)
    assert got[:7] == ([[0, 1], []], [2, 0], [7, 0], [3, 0], [4, 0], 1, [OK, OK, OK] + [DUPLICATE] * 4)
    # the same bytes in two rounds are two identities; with one round they are one
    assert mdc.model(2, [0, 1], [5, 5], [a, a], [OK, OK], None, 0, 1)[:2] == ([[0], [1]], [1, 1])
    assert mdc.model(1, [0, 0], [5, 5], [a, a], [OK, OK], None, 0, 1)[:2] == ([[0]], [1])


def test_self_checks_of_helpers_table_and_layout(check):
    assert check([]) == []


def _cmd(R, round_of, keys, ids, verdicts, floors, K, tranche, cap):
    return (["bestsd %d %d %d %d %d %d" % (R, len(keys), K, tranche, cap, 1 if floors else 0)] + [bc.b32(f).hex() for f in (floors or [])] +
            ["%d %d %s %s" % (r, v, bc.b32(k).hex(), i.hex()) for r, k, i, v in zip(round_of, keys, ids, verdicts)])


def _parse(line, R):
    head, status = line.split("|#|")
    parts = head.split("|")
    assert parts[0].split()[0] == "bestsd" and len(parts) == R + 1
    per = [[int(x) for x in p.split()] for p in parts[1:]]
    return ([p[4:] for p in per], [p[0] for p in per], [p[1] for p in per], [p[2] for p in per], [p[3] for p in per], int(parts[0].split()[1]),
            [int(x) for x in status.split()])


def test_rounds_best_distinct_host_against_the_model(check):
    cases = mdc.host_cases()
    assert len(cases) >= 60
    caps = [len(c[2]) if n % 3 else 1 for n, c in enumerate(cases)]  # every third case: room for one entry per round only
    cmds = []
    for case, cap in zip(cases, caps):
        cmds += _cmd(*case, cap)
    out = check(cmds)
    assert len(out) == len(cases)
    drops = uneven = shared = 0
    for line, case, cap in zip(out, cases, caps):
        R, ro, keys, ids, verdicts, floors, K, tranche = case
        best, n_best, n_cand, n_exam, n_dups, steps, status, ran = mdc.model(*case)
        assert _parse(line, R) == ([b[:cap] for b in best], n_best, n_cand, n_exam, n_dups, steps, status), case
        assert all(e + d <= c for e, d, c in zip(n_exam, n_dups, n_cand)) and status.count(DUPLICATE) == sum(n_dups)
        drops += sum(n_dups) > 0
        uneven += len({t for t in ran if t}) > 1
        shared += len(set(zip(ids, ro))) > len(set(ids))  # some id turns up in two rounds
    assert drops > 10 and uneven > 10 and shared > 10, (drops, uneven, shared)


def _table_cmd(log2, rows):
    return ["table %d %d" % (log2, len(rows))] + ["%d %d %s %s" % (e, r, dc.b32(k).hex(), i.hex()) for e, r, k, i in rows]


def _table_want(rows):
    """(claimed, the holders ascending, find of every row): the holder of an identity (round, id) is the first inserted row in candidate order"""
    holder = {}
    for n, (e, r, k, i) in enumerate(rows):
        if e and ((r, i) not in holder or (-k, n) < (-rows[holder[r, i]][2], holder[r, i])):
            holder[r, i] = n
    return len(holder), sorted(holder.values()), [holder.get((r, i), -1) for _, r, _, i in rows]


def _parse_table(line):
    head, held, finds = line.split("|")
    f = head.split()
    assert f[0] == "table"
    return int(f[1]), int(f[2]), [int(x) for x in held.split()], [int(x) for x in finds.split()]


def test_round_aware_table_one_row_after_the_other(check):
    rnd = random.Random(23)
    base = rnd.randbytes(32)
    cmds, wants = [], []
    # the tightest size: 2^s - 1 identities in 2^s slots -- ONE id in 2^s - 1 rounds, each with a second row of a higher key that displaces
    # the first; a round the table does not hold is looked up through the longest run there is and ends at the one empty slot (wrap-around:
    # the runs cross the table's end for some of the sizes)
    for log2 in (1, 2, 4, 6, 8):
        n = (1 << log2) - 1
        rows = [(1, r, 100 + r, base) for r in range(n)] + [(1, r, 500 + r, base) for r in range(n)] + [(0, n, 7, base)]
        cmds += _table_cmd(log2, rows)
        wants.append(_table_want(rows))
        assert wants[-1] == (n, list(range(n, 2 * n)), list(range(n, 2 * n)) * 2 + [-1])
    # one id in every round beside per-round ids, rows of one identity arriving in any order: the same row holds
    rows = [(1, n % 5, rnd.randrange(L), (base, bytes([n % 3]) * 32)[n % 2]) for n in range(40)] + [(0, 5, 5, base), (0, 0, 5, rnd.randbytes(32))]
    for order in range(4):
        shuffled = rows[:40]
        random.Random(order).shuffle(shuffled)
        cmds += _table_cmd(7, shuffled + rows[40:])
        wants.append(_table_want(shuffled + rows[40:]))
        assert wants[-1][0] == 5 + 5 * 3 and wants[-1][2][-2:] == [-1, -1]
    # equal keys: the lower index holds; the same bytes in another round hold a slot of their own
    rows = [(1, 0, 7, base)] * 3 + [(1, 1, 7, base)] * 2
    cmds += _table_cmd(3, rows)
    wants.append(_table_want(rows))
    assert wants[-1] == (2, [0, 3], [0, 0, 0, 3, 3])
    out = check(cmds)
    assert len(out) == len(wants)
    for line, (claimed, held, finds) in zip(out, wants):
        assert _parse_table(line) == (0, claimed, held, finds)
    # a full table: one id in 2^s rounds fills 2^s slots; one more round raises the probe flag (bit 0) and neither loops nor gets in
    flag, claimed, held, finds = _parse_table(check(_table_cmd(3, [(1, r, r, base) for r in range(9)]))[0])
    assert (flag, claimed, held, finds[:8]) == (1, 8, list(range(8)), list(range(8))) and finds[8] == -1


def test_header_binding_pool_surface_and_screening_without_a_device(bbp):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert hdr.index("Best valid proofs of many rounds") < hdr.index("Best proofs of many rounds, one per bidder") < hdr.index("bbp_verify_rounds_best_distinct(")
    assert hdr.index("bbp_debug_rounds_best(bbp_ctx") < hdr.index("Best proofs of many rounds, one per bidder")
    for phrase in ("the same 32 z_img bytes in two rounds are two identities", "runs no drop pass", "n_duplicates (R entries) is a required pointer",
                   "never on timing", "bbp_verify_rounds_best_distinct   the same, one per bidder", "bbp_debug_rounds_best_distinct, bbp_set_profiling"):
        assert phrase in hdr, phrase
    for name in ("bbp_verify_rounds_best_distinct", "bbp_verify_rounds_best_distinct_dev", "bbp_debug_rounds_best_distinct"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("verify_rounds_best_distinct", "verify_rounds_best_distinct_dev", "debug_rounds_best_distinct"):
        assert callable(getattr(bbp.Context, name)), name
    assert "verify_rounds_best_distinct" in vars(bbp.Pool) and "verify_rounds_best_distinct_dev" not in vars(bbp.Pool)
    assert "debug_rounds_best_distinct" not in vars(bbp.Pool)
    assert bbp.RoundsBestDistinct._fields == ("best", "n_best", "n_candidates", "n_examined", "n_duplicates", "n_steps", "status", "raw")
    # the checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form
    lib = bbp.lib
    assert lib.bbp_verify_rounds_best_distinct(None, 1, 1, 1, 1, 1, 1, None, 1, 1, 0, None, 1, 1, 1, 1, None, 1) == BAD_ARG
    assert lib.bbp_verify_rounds_best_distinct_dev(None, 1, 1, 1, 1, 1, 1, 1, None, 1, 1, 0, None, 1, 1, 1, 1, None, 1, None) == BAD_ARG
    assert lib.bbp_debug_rounds_best_distinct(None, 1, 1, 1, 1, 1, 1, None, 1, 1, 0, 0, None, 1, 1, 1, 1, None, 1) == BAD_ARG
    # ... the entry points screen the numbers with rounds_best.h's rounds_best_screen, whose order tests/test_rounds_best_host.py holds
    src = open(bbp.lib_path.rsplit("/", 1)[0] + "/csrc/capi_bests.hip").read()
    for name in ("bbp_verify_rounds_best_distinct", "bbp_verify_rounds_best_distinct_dev"):
        assert 'bests_screen(ctx, "%s", R, round_Ns, B, round_of, &done)' % name in src, name
