"""not-gpu tier: one offer to many standings (include/bbp.h bbp_standings_offer, bbp_debug_standings_offer).  The rule as
csrc/standings.h states it (standings_offer_host) runs in tests/standings_check.cpp, a stand-alone program under AddressSanitizer + UBSan;
the expected answers come from the model of tests/standings_cases.py: S instances of tests/round_standing_cases.py's Standing."""
import os
import subprocess
import tempfile

import pytest

from tests import standings_cases as mc

sc = mc.sc
OK, VERIFY, FORMAT, BAD_ARG, INTERNAL, SKIPPED, DUPLICATE = 0, 1, 3, 4, 6, -1, -2


@pytest.fixture(scope="module")
def check(built):
    exe = built.build_standings_check()

    def run(commands):
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("\n".join(commands) + "\n")
        try:
            r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
        finally:
            os.unlink(f.name)
        assert r.returncode == 0 and "standings_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout.splitlines()[:-1]
    return run


def _standings(Ks, floors):
    return ["standings %d" % len(Ks)] + ["%d %s" % (K, mc.b32(f).hex()) for K, f in zip(Ks, floors)]


def _offer(S, standing_of, keys, ids, verdicts, tranche, cap, log2=None):
    head = ["offer %d %d %d" % (len(keys), tranche, cap), " ".join(str(x) for x in (log2 or [0] * S))]
    return head + ["%d %d %s %s" % (s, v, mc.b32(k).hex(), i.hex()) for s, k, i, v in zip(standing_of, keys, ids, verdicts)]


def _parse(lines, S):
    """the S + 2 lines of one offer -> rc, n_steps, per standing [entered, ne, nc, nx, nd], offered, entries, statuses"""
    head = lines[0].split()
    assert head[0] == "offer"
    per, offered, entries = [], [], []
    for s in range(S):
        counts, ent, held = lines[1 + s].split("|")
        f = [int(x) for x in counts.split()]
        assert f[0] == s
        per.append([[int(x) for x in ent.split()]] + f[1:5])
        offered.append(f[5])
        entries.append([(int.from_bytes(bytes.fromhex(k), "little"), bytes.fromhex(i), int(n)) for n, k, i in (e.split(":") for e in held.split())])
    status = lines[1 + S].split()
    assert status[0] == "status"
    return int(head[1]), int(head[2]), per, offered, entries, [int(x) for x in status[1:]]


def _run_sequences(check, seqs):
    """every offer of every sequence against the model: counts, entered (cut to cap), statuses, n_steps, entries, offered"""
    cmds = []
    for Ks, floors, offers in seqs:
        cmds += _standings(Ks, floors)
        for so, keys, ids, verdicts, tranche, cap in offers:
            cmds += _offer(len(Ks), so, keys, ids, verdicts, tranche, cap)
    out, at, n = check(cmds), 0, 0
    for Ks, floors, offers in seqs:
        S = len(Ks)
        stands = [sc.Standing(f, K) for K, f in zip(Ks, floors)]
        for so, keys, ids, verdicts, tranche, cap in offers:
            want, steps, status = mc.offer(stands, so, keys, ids, verdicts, tranche)
            rc, got_steps, per, offered, entries, got_status = _parse(out[at:at + S + 2], S)
            at += S + 2
            assert rc == OK and got_steps == steps and got_status == status, (Ks, offers)
            assert per == [[w[0][:cap]] + w[1:] for w in want], (Ks, so, keys)
            assert entries == [st.entries for st in stands] and offered == [st.offered for st in stands]
            n += 1
    assert at == len(out)
    return n


def test_self_checks_of_plan_and_layout(check):
    assert check([]) == []


def test_model_on_hand_made_cases():
    a, b, c, d = b"a" * 32, b"b" * 32, b"c" * 32, b"d" * 32
    st = [sc.Standing(0, 2), sc.Standing(0, 2), sc.Standing(0, 1)]
    # rows of standings 0 and 1 interleaved; standing 2 receives no row; one z_img (a) in both: two identities
    per, steps, status = mc.offer(st, [0, 1, 0, 1], [9, 9, 7, 5], [a, a, b, c], [OK] * 4, 1)
    assert per == [[[0, 2], 2, 2, 2, 0], [[1, 3], 2, 2, 2, 0], [[], 0, 0, 0, 0]] and steps == 1 and status == [OK] * 4
    assert st[0].entries == [(9, a, 0), (7, b, 1)] and st[1].entries == [(9, a, 0), (5, c, 1)] and st[2].offered == 0
    # an improvement in standing 0 (b comes back higher) while standing 1 evicts (d pushes c out); serials are per standing
    per, steps, status = mc.offer(st, [1, 0, 0, 1], [6, 8, 7, 5], [d, b, a, c], [OK] * 4, 1)
    assert per == [[[1], 1, 1, 1, 0], [[0], 1, 1, 1, 0], [[], 0, 0, 0, 0]] and status == [OK, OK, SKIPPED, SKIPPED]
    assert st[0].entries == [(9, a, 0), (8, b, 2)] and st[1].entries == [(9, a, 0), (6, d, 2)] and [s.offered for s in st] == [4, 4, 0]
    # cap smaller than n_entered is the caller's cut: the model reports everything
    st = [sc.Standing(0, 3), sc.Standing(0, 3)]
    per, steps, _ = mc.offer(st, [0, 1, 0, 1, 0], [5, 5, 6, 6, 7], [a, a, b, b, c], [OK] * 5, 1)
    assert per[0][:2] == [[4, 2, 0], 3] and per[1][:2] == [[3, 1], 2] and steps == 1
    # n_steps is the most tranches any standing ran: K = 1, tranche 1, three forged rows in front of the valid one in standing 1
    st = [sc.Standing(0, 1), sc.Standing(0, 1)]
    per, steps, status = mc.offer(st, [0, 1, 1, 1, 1], [5, 9, 8, 7, 6], [a, a, b, c, d], [OK, VERIFY, VERIFY, VERIFY, OK], 1)
    assert steps == 3 and per[0][3] == 1 and per[1][3] == 4 and status == [OK, VERIFY, VERIFY, VERIFY, OK]


def test_hand_made_cases_against_the_rule(check):
    a, b, c, d = b"a" * 32, b"b" * 32, b"c" * 32, b"d" * 32
    S = 4
    same_z = ([0, 1, 2, 3], [9, 8, 7, 6], [a] * 4, [OK] * 4, 0, 4)  # one z_img in all standings enters every one
    seqs = [
        ([2, 2, 1], [0, 0, 0], [([0, 1, 0, 1], [9, 9, 7, 5], [a, a, b, c], [OK] * 4, 1, 4), ([1, 0, 0, 1], [6, 8, 7, 5], [d, b, a, c], [OK] * 4, 1, 4)]),
        ([1] * S, [0] * S, [same_z, same_z]),
        ([3, 3], [0, 0], [([0, 1, 0, 1, 0], [5, 5, 6, 6, 7], [a, a, b, b, c], [OK] * 5, 1, 2), ([0, 1], [9, 9], [d, d], [OK, VERIFY], 1, 0)]),
        ([1, 1], [0, 0], [([0, 1, 1, 1, 1], [5, 9, 8, 7, 6], [a, a, b, c, d], [OK, VERIFY, VERIFY, VERIFY, OK], 1, 5)]),
        ([2, 16, 1], [0, 1 << 6, 0], [([], [], [], [], 0, 0), ([2], [mc.L], [a], [OK], 0, 1)]),
    ]
    assert _run_sequences(check, seqs) == 9


def test_random_sequences_with_resends(check):
    seqs = mc.random_sequences(seed=21, n_seq=150)
    assert {len(Ks) for Ks, _, _ in seqs} == set(range(1, 9)) and {K for Ks, _, _ in seqs for K in Ks} == {1, 3, 16}
    assert _run_sequences(check, seqs) >= 300


def test_internal_in_one_standing_changes_no_state(check):
    a = [bytes([n]) * 32 for n in range(1, 12)]
    first = ([0, 1, 2] * 2, [9, 8, 7, 6, 5, 4], a[:6], [OK] * 6, 0, 6)
    # standing 1's table is forced to two slots: its three identities (K + rows) do not fit -> BBP_ERR_INTERNAL, every state as before
    second = ([0, 1, 2, 1, 1], [19, 18, 17, 16, 15], a[6:11], [OK] * 5, 0, 5)
    cmds = _standings([4, 4, 4], [0, 0, 0]) + _offer(3, *first) + _offer(3, *second, log2=[0, 1, 0]) + _offer(3, *second)
    out = check(cmds)  # (the program itself holds the states against their copies when rc != 0)
    r1, r2, r3 = (_parse(out[5 * n:5 * n + 5], 3) for n in range(3))
    assert r1[0] == OK and r2[0] == INTERNAL and r3[0] == OK
    assert r2[3] == r1[3] == [2, 2, 2] and r2[4] == r1[4]
    stands = [sc.Standing(0, 4) for _ in range(3)]
    mc.offer(stands, *first[:5])
    want, steps, status = mc.offer(stands, *second[:5])
    assert r3[2] == want and r3[1] == steps and r3[5] == status and r3[4] == [st.entries for st in stands] and r3[3] == [3, 5, 3]


def test_header_and_binding_surface_without_a_device(bbp):
    hdr = open(bbp.lib_path.rsplit("/", 2)[0] + "/include/bbp.h").read()
    assert hdr.index("Standing of a round") < hdr.index("Standings of many rounds")
    single = hdr[hdr.index("Standing of a round"):hdr.index("Standings of many rounds")]
    assert "standings over many rounds in one call" not in single
    many = hdr[hdr.index("Standings of many rounds"):]
    assert "Out of scope: a _dev form; a server opcode; more than BBP_STANDING_MAX_OPEN standings" in many
    for name in ("bbp_standings_offer", "bbp_debug_standings_offer"):
        assert name in bbp.SIGNATURES and hasattr(bbp.lib, name) and name in hdr, name
    assert callable(bbp.Context.standings_offer) and callable(bbp.Context.debug_standings_offer)
    assert "standings_offer" in vars(bbp.Pool) and "debug_standings_offer" not in vars(bbp.Pool)
    assert bbp.StandingsOffer._fields == ("entered", "n_entered", "n_candidates", "n_examined", "n_duplicates", "n_steps", "status", "raw")
    # the checks that need no context: a NULL handle or a NULL required pointer is BBP_ERR_BAD_ARG
    lib = bbp.lib
    assert lib.bbp_standings_offer(None, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_standings_offer(1, 2, 1, 1, None, 1, 0, 0, None, 1, 1, 1, 1, 1, 1) == BAD_ARG  # standing_of NULL with S == 2
    assert lib.bbp_standings_offer(1, 1, 1, 1, 1, 1, 0, 1, None, 1, 1, 1, 1, 1, 1) == BAD_ARG  # entered_out NULL with cap == 1
    assert lib.bbp_standings_offer(1, 1, None, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_debug_standings_offer(None, 1, 1, 1, 1, 1, 1, 1, 0, 0, None, 1, 1, 1, 1, 1, 1) == BAD_ARG
    assert lib.bbp_debug_standings_offer(1, 1, 1, 1, 1, 1, 1, None, 0, 0, None, 1, 1, 1, 1, 1, 1) == BAD_ARG
