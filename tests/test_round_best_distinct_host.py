"""not-gpu tier: the best proofs of a round, one per bidder (include/bbp.h bbp_verify_round_best_distinct, its _dev form,
bbp_debug_round_best_distinct).  The rules as csrc/round_best.h states them (round_best_distinct_host), the identity table's helpers as the
kernels run them and the extra layout run in tests/round_best_distinct_check.cpp, a stand-alone program under AddressSanitizer + UBSan;
the expected answers come from the model of tests/round_best_distinct_cases.py, which is itself held to cases written out by hand."""
import os
import random
import subprocess
import tempfile

import pytest

from tests import round_best_distinct_cases as dc

OK, VERIFY, FORMAT, BAD_ARG, SKIPPED, DUPLICATE = 0, 1, 3, 4, -1, -2
L = dc.L


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_round_best_distinct_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "round_best_distinct_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def test_model_on_hand_made_cases():
    """The model itself, on answers written out by hand (it decides every other case)."""
    a, b, c = "a", "b", "c"
    ok5 = [OK] * 5
    # two OK rows of one id in one tranche: the first in candidate order holds -- here the HIGHER index, whose key is higher; both
    # statuses are OK, n_best counts one
    assert dc.model([5, 9], [a, a], [OK, OK], 0, 2, 2) == ([1], 1, 2, 2, 0, [OK, OK])
    assert dc.model([9, 9], [a, a], [OK, OK], 0, 2, 2) == ([0], 1, 2, 2, 0, [OK, OK])  # equal keys: the lower index
    # the same id across a tranche boundary: the later row becomes DUPLICATE, and the call goes on to the next identity
    # (T_0 = K = 2: rows 0 and 1; one identity settled; row 2 carries it and is dropped; tranche 1 is row 3 alone)
    assert dc.model([9, 8, 7, 6], [a, b, a, c], [OK, VERIFY, OK, OK], 0, 2, 1) == ([0, 3], 2, 4, 3, 1, [OK, VERIFY, DUPLICATE, OK])
    # without the rule the same input gives the copy as second winner (the existing call: tests/round_best_cases.py)
    assert dc.bc.model([9, 8, 7, 6], [OK, VERIFY, OK, OK], 0, 2, 1)[0] == [0, 2]
    # a failing higher-scored row with the victim's id: it settles nothing, the victim still wins and is verified
    assert dc.model([9, 8, 7], [a, a, b], [VERIFY, OK, OK], 0, 1, 1) == ([1], 1, 3, 3, 0, [VERIFY, OK, OK])
    assert dc.model([9, 8, 7], [a, a, b], [FORMAT, OK, OK], 0, 2, 1) == ([1, 2], 2, 3, 3, 0, [FORMAT, OK, OK])
    # K == 0: one tranche, every candidate examined, zero duplicates, holders distinct
    keys, ids = [5, 9, 9, 1, 7], [a, b, a, c, b]
    assert dc.model(keys, ids, [OK, OK, OK, VERIFY, OK], 0, 0, 1) == ([1, 2], 2, 5, 5, 0, [OK, OK, OK, VERIFY, OK])
    assert dc.model(keys, ids, ok5, 5, 0, 1) == ([1, 2], 2, 4, 4, 0, [OK, OK, OK, SKIPPED, OK])
    # stop reached: the remaining rows of a settled id stay SKIPPED, not DUPLICATE
    assert dc.model(keys, [a] * 5, ok5, 0, 1, 1) == ([1], 1, 5, 1, 0, [SKIPPED, OK, SKIPPED, SKIPPED, SKIPPED])
    # ... and when K asks for more identities than there are, every other row of the settled one is dropped unverified
    assert dc.model(keys, [a] * 5, ok5, 0, 2, 1) == ([1], 1, 5, 2, 3, [DUPLICATE, OK, OK, DUPLICATE, DUPLICATE])
    # a tranche of one (tranche 1, K 1) that fails: tranche 1 holds two rows of one id, both verified, the first holds
    assert dc.model(keys, [c, b, a, c, a], [OK, VERIFY, OK, OK, OK], 0, 1, 1) == ([2], 1, 5, 3, 0, [SKIPPED, VERIFY, OK, SKIPPED, OK])
    # a tranche is the next T_t LIVE rows: T_0 = 2 settles a; rows 2 and 3 are dropped; T_1 = 4 takes rows 4..7 and stops; row 8 is never reached
    got = dc.model([9, 8, 7, 6, 5, 4, 3, 2, 1], [a, "z", a, a, b, "y", "y", c, c], [OK, VERIFY] + [OK] * 7, 0, 2, 1)
    assert got == ([0, 4], 2, 9, 6, 2, [OK, VERIFY, DUPLICATE, DUPLICATE, OK, OK, OK, OK, SKIPPED])
    keys6, ids6 = [9, 8, 7, 6, 5, 4], [a, a, a, b, c, c]
    got = dc.model(keys6, ids6, [OK] * 6, 0, 3, 1)  # T_0 = 3: rows 0, 1, 2 in one tranche (all verified); T_1 = 6 takes the rest
    assert got == ([0, 3, 4], 3, 6, 6, 0, [OK] * 6)
    got = dc.model(keys6, ids6, [OK] * 6, 0, 6, 1)  # K = 6 > identities: T_0 = 6, one tranche
    assert got == ([0, 3, 4], 3, 6, 6, 0, [OK] * 6)
    got = dc.model([9, 8, 7, 6, 5, 4, 3], [a, a, a, a, b, b, c], [OK] * 7, 0, 3, 1)  # T_0 = 3, drop row 3, T_1 takes 4, 5, 6
    assert got == ([0, 4, 6], 3, 7, 6, 1, [OK, OK, OK, DUPLICATE, OK, OK, OK])
    # keys >= l and the floor, as in the existing call
    assert dc.model([L, L - 1, bc_all_ones(), 3], [a, a, a, a], [OK] * 4, 0, 0, 1) == ([1], 1, 2, 2, 0, [FORMAT, OK, FORMAT, OK])
    assert dc.model(keys, ids, ok5, 10, 1, 1) == ([], 0, 0, 0, 0, [SKIPPED] * 5)
    # examined + dups <= n_candidates, in every case above and in the generated ones
    for keys, ids, verdicts, floor, K, tranche in dc.host_cases():
        best, n_best, nc, ne, nd, status = dc.model(keys, ids, verdicts, floor, K, tranche)
        assert ne + nd <= nc and len({ids[i] for i in best}) == len(best) == n_best
        assert status.count(DUPLICATE) == nd and (K or nd == 0)


def bc_all_ones():
    return dc.bc.ALL_ONES


def test_self_checks_of_helpers_and_layout(check):
    assert check([]) == []


def _cmd(keys, ids, verdicts, floor, K, tranche, cap):
    return ["distinct %d %d %d %d %s" % (len(keys), K, tranche, cap, dc.b32(floor).hex())] + [
        "%d %s %s" % (v, dc.b32(k).hex(), i.hex()) for k, i, v in zip(keys, ids, verdicts)]


def _parse(line):
    head, best, status = line.split("|")
    f = head.split()
    assert f[0] == "distinct"
    return [int(x) for x in best.split()], int(f[1]), int(f[2]), int(f[3]), int(f[4]), [int(x) for x in status.split()]


def test_round_best_distinct_host_against_the_model(check):
    cases = dc.host_cases()
    assert len(cases) > 60 and {len(c[0]) for c in cases} >= {1, 40}
    caps = [len(c[0]) if n % 3 else 2 for n, c in enumerate(cases)]  # every third case: room for two entries only
    cmds = []
    for (keys, ids, verdicts, floor, K, tranche), cap in zip(cases, caps):
        cmds += _cmd(keys, ids, verdicts, floor, K, tranche, cap)
    out = check(cmds)
    assert len(out) == len(cases)
    seen_dups = seen_stop_early = seen_shared_tranche = 0
    for line, (keys, ids, verdicts, floor, K, tranche), cap in zip(out, cases, caps):
        best, n_best, nc, ne, nd, status = dc.model(keys, ids, verdicts, floor, K, tranche)
        assert _parse(line) == (best[:cap], n_best, nc, ne, nd, status), (keys, ids, verdicts, floor, K, tranche)
        seen_dups += nd > 0
        seen_stop_early += ne + nd < nc
        seen_shared_tranche += status.count(OK) > n_best
    assert seen_dups > 10 and seen_stop_early > 10 and seen_shared_tranche > 10


def _table_cmd(log2, rows):
    return ["table %d %d" % (log2, len(rows))] + ["%d %s %s" % (e, dc.b32(k).hex(), i.hex()) for e, k, i in rows]


def _table_want(rows):
    """(claimed, the holders ascending, find of every row): the holder of an identity is the first inserted row in candidate order"""
    holder = {}
    for n, (e, k, i) in enumerate(rows):
        if e and (i not in holder or (-k, n) < (-rows[holder[i]][1], holder[i])):
            holder[i] = n
    return len(holder), sorted(holder.values()), [holder.get(i, -1) for _, _, i in rows]


def _parse_table(line):
    head, held, finds = line.split("|")
    f = head.split()
    assert f[0] == "table"
    return int(f[1]), int(f[2]), [int(x) for x in held.split()], [int(x) for x in finds.split()]


def test_table_helpers_run_one_row_after_the_other(check):
    rnd = random.Random(9)
    base = rnd.randbytes(32)
    near = [bytes([base[0] ^ 1]) + base[1:], base[:31] + bytes([base[31] ^ 0x80]), base]  # differ only in byte 0, only in byte 31
    cmds, wants = [], []
    # ids equal in 31 bytes are three identities; the rows of one identity arrive in any order and the same row holds
    rows = [(1, rnd.randrange(L), near[n % 3]) for n in range(12)] + [(0, 5, near[0]), (0, 5, rnd.randbytes(32))]
    for order in range(4):
        shuffled = rows[:12]
        random.Random(order).shuffle(shuffled)
        cmds += _table_cmd(5, shuffled + rows[12:])
        wants.append(_table_want(shuffled + rows[12:]))
        assert wants[-1][0] == 3
    # exactly one empty slot: 2^s - 1 identities in 2^s slots, each with a second row of a higher key that displaces the first; an id the
    # table does not hold is looked up through the longest run there is and ends at the one empty slot
    for log2 in (1, 2, 4, 6):
        n_ids = (1 << log2) - 1
        ids = [rnd.randbytes(32) for _ in range(n_ids)]
        rows = [(1, 100 + n, i) for n, i in enumerate(ids)] + [(1, 500 + n, i) for n, i in enumerate(ids)] + [(0, 7, rnd.randbytes(32))]
        cmds += _table_cmd(log2, rows)
        wants.append(_table_want(rows))
        assert wants[-1][1] == list(range(n_ids, 2 * n_ids)) and wants[-1][2][-1] == -1
    # equal keys: the lower index holds, whichever enters first
    rows = [(1, 7, base)] * 5
    cmds += _table_cmd(3, rows)
    wants.append(_table_want(rows))
    assert wants[-1] == (1, [0], [0] * 5)
    out = check(cmds)
    assert len(out) == len(wants)
    for line, (claimed, held, finds) in zip(out, wants):
        assert _parse_table(line) == (0, claimed, held, finds)
    # a full table: 2^s identities in 2^s slots all get in; one more raises the probe flag (bit 0) and neither loops nor gets in
    ids = [rnd.randbytes(32) for _ in range(9)]
    flag, claimed, held, finds = _parse_table(check(_table_cmd(3, [(1, n, i) for n, i in enumerate(ids)]))[0])
    assert (flag, claimed, held, finds[:8]) == (1, 8, list(range(8)), list(range(8))) and finds[8] == -1


def test_header_and_binding_surface_without_a_device(bbp):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_ROW_DUPLICATE (-2)" in hdr and bbp.ROW_DUPLICATE == -2 == DUPLICATE
    assert "#define BBP_ROW_SKIPPED (-1)" in hdr and bbp.ROW_SKIPPED == -1
    assert hdr.index("Best valid proofs of a round") < hdr.index("Best proofs of a round, one per bidder")
    for name in ("bbp_verify_round_best_distinct", "bbp_verify_round_best_distinct_dev", "bbp_debug_round_best_distinct"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name), name
    for name in ("verify_round_best_distinct", "verify_round_best_distinct_dev", "debug_round_best_distinct"):
        assert callable(getattr(bbp.Context, name)), name
    assert "verify_round_best_distinct" in vars(bbp.Pool)
    # the checks that need no context: a NULL required pointer is BBP_ERR_BAD_ARG in every form -- n_duplicates among them
    lib = bbp.lib
    assert lib.bbp_verify_round_best_distinct(None, 8, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_verify_round_best_distinct_dev(None, 8, 1, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1, None) == BAD_ARG
    assert lib.bbp_debug_round_best_distinct(None, 1, 1, 1, 1, 1, 1, 0, 0, 0, None, 1, 1, 1, 1, 1) == BAD_ARG
    # with a (made-up, never dereferenced) context the NULL check still comes first
    assert lib.bbp_verify_round_best_distinct(1, 8, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, None, 1) == BAD_ARG
    assert lib.bbp_verify_round_best_distinct_dev(1, 8, 1, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, None, 1, None) == BAD_ARG
    assert lib.bbp_debug_round_best_distinct(1, 1, 1, 1, 1, 1, 1, 0, 0, 0, None, 1, 1, 1, None, 1) == BAD_ARG
    assert lib.bbp_debug_round_best_distinct(1, 1, 1, None, 1, 1, 1, 0, 0, 0, None, 1, 1, 1, 1, 1) == BAD_ARG  # ids
