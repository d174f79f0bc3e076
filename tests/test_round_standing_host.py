"""not-gpu tier: a standing of a round (include/bbp.h bbp_standing_open, bbp_standing_offer, bbp_standing_read, bbp_standing_close,
bbp_debug_standing_offer).  The rules as csrc/round_standing.h states them (standing_offer_host) run in tests/round_standing_check.cpp, a
stand-alone program under AddressSanitizer + UBSan; the expected answers come from the model of tests/round_standing_cases.py, which is
itself held to cases written out by hand, to the one-shot model and to truth()."""
import os
import random
import subprocess
import tempfile

import pytest

from tests import round_standing_cases as sc

dc = sc.dc
OK, VERIFY, FORMAT, BAD_ARG, INTERNAL, SKIPPED, DUPLICATE = 0, 1, 3, 4, 6, -1, -2
L = sc.L


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_round_standing_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "round_standing_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def test_model_on_hand_made_cases():
    a, b, c, d = b"a" * 32, b"b" * 32, b"c" * 32, b"d" * 32
    st = sc.Standing(0, 3)
    assert st.offer([9, 7, 5], [a, b, c], [OK, OK, OK], 1) == ([0, 1, 2], 3, 3, 3, 0, [OK, OK, OK])
    assert st.entries == [(9, a, 0), (7, b, 1), (5, c, 2)]
    # improvement: the identity at rank 2 comes back with a higher key; size unchanged, ranks re-ordered.  A lower copy of a held
    # identity above the bar is a DUPLICATE; an equal key at a later serial loses: SKIPPED, the standing is full
    assert st.offer([8, 6, 5], [c, a, d], [OK, OK, OK], 1) == ([0], 1, 2, 1, 1, [OK, DUPLICATE, SKIPPED])
    assert st.entries == [(9, a, 0), (8, c, 3), (7, b, 1)]
    # eviction: d pushes b out; b's row is forgotten and its resend is SKIPPED (the bar rose to 8)
    assert st.offer([10], [d], [OK], 1) == ([0], 1, 1, 1, 0, [OK])
    assert st.entries == [(10, d, 6), (9, a, 0), (8, c, 3)]
    assert st.offer([7, 8], [b, b], [OK, OK], 1) == ([], 0, 0, 0, 0, [SKIPPED, SKIPPED]) and st.offered == 9
    # not full: an equal key at a later serial of a held identity is a DUPLICATE
    st = sc.Standing(0, 3)
    st.offer([9], [a], [OK], 1)
    assert st.offer([9, 9], [a, b], [OK, OK], 1) == ([1], 1, 2, 1, 1, [DUPLICATE, OK])
    # a forged higher score on a held identity fails and changes nothing; sent again it costs another check
    assert st.offer([50], [a], [VERIFY], 1) == ([], 0, 1, 1, 0, [VERIFY])
    assert st.offer([50], [a], [VERIFY], 1) == ([], 0, 1, 1, 0, [VERIFY]) and st.entries == [(9, a, 0), (9, b, 2)]
    # keys >= l, the floor, and an offer of nothing
    st = sc.Standing(5, 1)
    assert st.offer([L, 4, 5], [a, b, c], [OK, OK, OK], 0) == ([2], 1, 1, 1, 0, [FORMAT, SKIPPED, OK])
    assert st.offer([], [], [], 0) == ([], 0, 0, 0, 0, []) and st.offered == 3
    # the model against the one-shot model (first offers) and against truth (random cuts): the counts the rule's author reports
    assert sc.self_check() == (200, 800)


def test_self_checks_of_helpers_and_layouts(check):
    assert check([]) == []


def _standing(floor, K):
    return ["standing %d %s" % (K, sc.b32(floor).hex())]


def _offer(keys, ids, verdicts, tranche, cap, log2=0):
    return ["offer %d %d %d %d" % (len(keys), tranche, cap, log2)] + ["%d %s %s" % (v, sc.b32(k).hex(), i.hex()) for k, i, v in zip(keys, ids, verdicts)]


def _parse(line):
    head, entered, status, entries = line.split("|")
    f = head.split()
    assert f[0] == "offer"
    ent = []
    for e in entries.split():
        s, k, i = e.split(":")
        ent.append((int.from_bytes(bytes.fromhex(k), "little"), bytes.fromhex(i), int(s)))
    return int(f[1]), ([int(x) for x in entered.split()], int(f[2]), int(f[3]), int(f[4]), int(f[5]), [int(x) for x in status.split()]), ent, int(f[6])


def _run_plan(check, plan):
    """plan: [(case, bursts, caps)] -> every burst against the model and truth"""
    cmds = []
    for (keys, ids, verdicts, floor, K, tranche), bursts, caps in plan:
        cmds += _standing(floor, K)
        for sl, cap in zip(bursts, caps):
            cmds += _offer(keys[sl], ids[sl], verdicts[sl], tranche, cap)
    out = iter(check(cmds))
    n = 0
    for case, bursts, caps in plan:
        keys, ids, verdicts, floor, K, tranche = case
        for (want, entries, offered), sl, cap in zip(sc.run_bursts(case, bursts), bursts, caps):
            rc, got, got_entries, got_offered = _parse(next(out))
            assert rc == OK and got == (want[0][:cap],) + want[1:], (case, bursts)
            assert got_entries == entries == sc.truth(keys[:sl.stop], ids[:sl.stop], verdicts[:sl.stop], floor, K) and got_offered == offered == sl.stop
            n += 1
    assert next(out, None) is None
    return n


def test_first_offer_equals_the_one_shot_call(check):
    cases = sc.host_cases()
    assert len(cases) >= 200
    plan = [(c, [slice(0, len(c[0]))], [len(c[0]) if n % 3 else 2]) for n, c in enumerate(cases)]
    for (keys, ids, verdicts, floor, K, tranche), _, _ in plan:  # the model's first offer IS dc.model, field for field
        assert sc.Standing(floor, K).offer(keys, ids, verdicts, tranche) == dc.model(keys, ids, verdicts, floor, K, tranche)
    assert _run_plan(check, plan) == len(cases)


def test_random_cuts_give_truth_after_every_burst(check):
    rnd = random.Random(11)
    plan = []
    for case in sc.host_cases():
        B = len(case[0])
        for _ in range(2):
            bursts = sc.cuts(B, rnd.randrange(1, 5), rnd)
            plan.append((case, bursts, [B] * len(bursts)))
    assert any(sl.start == sl.stop for _, bursts, _ in plan for sl in bursts)  # an empty burst among them
    assert _run_plan(check, plan) > 800


def test_resend_examines_no_valid_row_again(check):
    cmds, cases = [], sc.host_cases()[::3]
    for keys, ids, verdicts, floor, K, tranche in cases:
        cmds += _standing(floor, K) + _offer(keys, ids, verdicts, tranche, len(keys)) * 2
    out = check(cmds)
    seen = 0
    for n, (keys, ids, verdicts, floor, K, tranche) in enumerate(cases):
        _, _, entries, _ = _parse(out[2 * n])
        rc, (entered, ne, nc, nx, nd, status), again, offered = _parse(out[2 * n + 1])
        assert rc == OK and again == entries and entered == [] and offered == 2 * len(keys)
        examined = [j for j, (s, k) in enumerate(zip(status, keys)) if s not in (SKIPPED, DUPLICATE) and k < L]  # (k >= l: FORMAT by screening)
        assert nx == len(examined) and all(verdicts[j] != OK and status[j] == verdicts[j] for j in examined)
        st = sc.Standing(floor, K)
        st.offer(keys, ids, verdicts, tranche)
        assert (entered, ne, nc, nx, nd, status) == st.offer(keys, ids, verdicts, tranche)
        seen += nx
    assert seen > 0  # forged rows are examined each time they are sent


@pytest.mark.parametrize("K", [1, 2, 64, 65, 1024])
def test_merge_at_K(check, K):
    rnd = random.Random(K)
    B = 3 * K + 5
    keys = [rnd.randrange(1, 1 << 40) for _ in range(B)]
    keys[3] = keys[1]  # equal keys: the earlier serial first
    ids = dc.id_pool(B, B, 70 + K)
    for j in range(0, B - 1, 5):  # every fifth identity has a second row
        ids[j + 1] = ids[j]
    verdicts = [rnd.choice((OK, OK, OK, VERIFY)) for _ in range(B)]
    case = (keys, ids, verdicts, 0, K, 4)
    bursts = [slice(0, K // 2 + 1), slice(K // 2 + 1, K + 2), slice(K + 2, B)]
    assert _run_plan(check, [(case, bursts, [B] * 3)]) == 3
    assert len(sc.truth(keys, ids, verdicts, 0, K)) == K  # the standing filled: the cut ran


def test_identity_table_at_its_tightest(check):
    rnd = random.Random(3)
    ids = [rnd.randbytes(32) for _ in range(7)]
    keys = [100 + n for n in range(7)] + [200 + n for n in range(7)]
    verdicts = [OK] * 14
    st = sc.Standing(0, 4)
    want1, want2 = st.offer(keys[:7], ids, verdicts[:7], 2), st.offer(keys[7:], ids, verdicts[7:], 2)
    # 7 identities in 8 slots: one empty slot ends every probe; every identity improves in the second offer
    cmds = _standing(0, 4) + _offer(keys[:7], ids, verdicts[:7], 2, 7, 3) + _offer(keys[7:], ids, verdicts[7:], 2, 7, 3)
    out = check(cmds)
    assert _parse(out[0])[:2] == (OK, want1) and _parse(out[1])[:2] == (OK, want2) and _parse(out[1])[2] == st.entries
    # 9 identities do not fit into 8 slots: BBP_ERR_INTERNAL, and the standing is as the first offer left it
    ids9 = ids + [rnd.randbytes(32), rnd.randbytes(32)]
    out = check(_standing(0, 9) + _offer(keys[:7], ids, verdicts[:7], 0, 7, 3) + _offer([300 + n for n in range(9)], ids9, [OK] * 9, 0, 9, 3))
    first, second = _parse(out[0]), _parse(out[1])
    assert first[0] == OK and second[0] == INTERNAL and second[2] == first[2] and second[3] == first[3] == 7


def test_handle_bookkeeping(check):
    steps = ["o"] * 64 + ["o", "c5", "c5", "o", "c63", "c0", "o", "o", "o", "c64", "c99"]
    out = check(["handles", " ".join(steps)])
    got = [int(x) for x in out[0].split()[1:]]
    assert got == list(range(64)) + [64, 1, 0, 5, 1, 1, 0, 63, 64, 0, 0]


def test_header_and_binding_surface_without_a_device(bbp):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert "#define BBP_STANDING_MAX_K 1024u" in hdr and bbp.STANDING_MAX_K == 1024 == sc.MAX_K
    assert "#define BBP_STANDING_MAX_OPEN 64u" in hdr and bbp.STANDING_MAX_OPEN == 64 == sc.MAX_OPEN
    assert hdr.index("Best proofs of many rounds, one per bidder") < hdr.index("Standing of a round")
    names = ("bbp_standing_open", "bbp_standing_offer", "bbp_standing_read", "bbp_standing_close", "bbp_debug_standing_offer", "bbp_debug_standing_trip")
    for name in names:
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name) and name in hdr, name
    for name in ("standing_open", "standing_offer", "standing_read", "standing_close", "debug_standing_offer"):
        assert callable(getattr(bbp.Context, name)), name
    for name in ("standing_open", "standing_offer", "standing_read", "standing_close"):
        assert name in vars(bbp.Pool), name
    assert "debug_standing_offer" not in vars(bbp.Pool)
    assert bbp.StandingOffer._fields == ("entered", "n_entered", "n_candidates", "n_examined", "n_duplicates", "status", "raw")
    assert bbp.StandingEntries._fields == ("serials", "scores", "z_imgs", "n_entries", "n_offered")
    # the checks that need no context: a NULL handle or a NULL required pointer is BBP_ERR_BAD_ARG
    lib = bbp.lib
    assert lib.bbp_standing_open(None, 8, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_standing_open(1, 8, None, 1, 1, 1) == BAD_ARG and lib.bbp_standing_open(1, 8, 1, None, 1, 1) == BAD_ARG
    assert lib.bbp_standing_open(1, 8, 1, 1, 1, None) == BAD_ARG
    assert lib.bbp_standing_offer(None, 0, 1, 1, 0, 0, None, 1, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_standing_read(None, 0, 0, None, None, None, 1, None) == BAD_ARG and lib.bbp_standing_read(1, 0, 0, None, None, None, None, None) == BAD_ARG
    assert lib.bbp_standing_close(None, 0) == BAD_ARG
    assert lib.bbp_debug_standing_offer(None, 0, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1) == BAD_ARG
