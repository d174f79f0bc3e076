"""The rules of bbp_verify_rounds_best (include/bbp.h "Best valid proofs of many rounds") as a model: tests/round_best_cases.py's model per
round, the indices mapped back, n_steps the most tranches any round ran.  Both tiers use it: the CPU tier (tests/test_rounds_best_host.py:
csrc/rounds_best.h on the host) and the GPU tier (tests/test_gpu_rounds_best.py).  Keys and floors are ints in [0, 2^256)."""
import random

from tests import round_best_cases as bc

L = bc.L
OK, VERIFY, FORMAT, SKIPPED = bc.OK, bc.VERIFY, bc.FORMAT, bc.SKIPPED


def tranches_run(n_candidates, n_examined, K, tranche):
    """the tranches a round ran: the least t whose first t tranches hold n_examined rows"""
    T0 = max(tranche or bc.TRANCHE_DEFAULT, K) if K else n_candidates
    t = 0
    while bc.examined_after(n_candidates, T0, t) < n_examined:
        t += 1
    return t


def model(R, round_of, keys, verdicts, floors, K, tranche):
    """(best: R lists in rank order, n_best[R], n_candidates[R], n_examined[R], n_steps, status[B]); floors: None or R ints"""
    B = len(keys)
    status = [None] * B
    best, n_best, n_cand, n_exam, steps = [], [], [], [], 0
    by_round = [[] for _ in range(R)]
    for i in range(B):
        by_round[round_of[i]].append(i)
    for r, rows in enumerate(by_round):
        b, nb, nc, ne, st = bc.model([keys[i] for i in rows], [verdicts[i] for i in rows], floors[r] if floors else 0, K, tranche)
        best.append([rows[j] for j in b])
        n_best.append(nb), n_cand.append(nc), n_exam.append(ne)
        for j, i in enumerate(rows):
            status[i] = st[j]
        steps = max(steps, tranches_run(nc, ne, K, tranche))
    return best, n_best, n_cand, n_exam, steps, status


# ---- row-to-round maps ---------------------------------------------------------------------------------------------------------------------
def map_blocks(B, R):
    return [i * R // B for i in range(B)]


def map_mod(B, R):
    return [i % R for i in range(B)]


def map_skewed(B, R):
    """round 0 holds all but R - 1 rows; every other round one row"""
    return [0] * (B - (R - 1)) + list(range(1, R)) if B >= R else map_mod(B, R)


def map_holes(B, R):
    """every third round is named by no row (its rows go to the round behind it)"""
    named = [r for r in range(R) if r % 3 != 1] or [0]
    return [named[i % len(named)] for i in range(B)]


MAPS = {"blocks": map_blocks, "mod": map_mod, "skewed": map_skewed, "holes": map_holes}


def floors_alternating(R, round_of, keys):
    """by round: 0, the round's median key, l"""
    out, by_round = [], [[] for _ in range(R)]
    for i, k in enumerate(keys):
        by_round[round_of[i]].append(k)
    for r in range(R):
        mine = sorted(by_round[r])
        out.append((0, mine[len(mine) // 2] if mine else 0, L)[r % 3])
    return out


def _candidates(R, round_of, keys, floors):
    per = [[] for _ in range(R)]
    for i, k in enumerate(keys):
        if (floors[round_of[i]] if floors else 0) <= k < L:
            per[round_of[i]].append(i)
    return [sorted(c, key=lambda i: (-keys[i], i)) for c in per]


def verdicts_top_third_bad(R, round_of, keys, floors):
    v = [OK] * len(keys)
    for cand in _candidates(R, round_of, keys, floors):
        for n, i in enumerate(cand[:len(cand) // 3]):
            v[i] = (VERIFY, FORMAT)[n % 2]
    return v


def verdicts_first_tranches_bad(R, round_of, keys, floors, K, tranche):
    """round r's first (r mod 4) tranches are bad, the rest OK: rounds stop at different steps"""
    v = [OK] * len(keys)
    for r, cand in enumerate(_candidates(R, round_of, keys, floors)):
        T0 = max(tranche or bc.TRANCHE_DEFAULT, K) if K else len(cand)
        for i in cand[:bc.examined_after(len(cand), T0, r % 4)]:
            v[i] = VERIFY
    return v


def host_cases():
    """(R, round_of, keys, verdicts, floors, K, tranche) for the CPU tier: more than 60"""
    rnd = random.Random(47)
    cases = []
    for B, R, kind in ((1, 1, bc.keys_uniform), (7, 3, bc.keys_edges), (40, 5, bc.keys_low_byte), (60, 9, bc.keys_uniform), (33, 40, bc.keys_uniform)):
        keys = kind(B, 200 + B)
        for mname, make in MAPS.items():
            ro = make(B, R)
            fl = floors_alternating(R, ro, keys)
            for floors, K, tranche in ((None, 1, 1), (fl, 0, 4), (fl, 3, 1), (None, 2, 4)):
                for verdicts in ([OK] * B, verdicts_top_third_bad(R, ro, keys, floors), verdicts_first_tranches_bad(R, ro, keys, floors, K, tranche),
                                 [rnd.choice((OK, VERIFY, FORMAT)) for _ in range(B)]):
                    cases.append((R, ro, keys, verdicts, floors, K, tranche))
    return cases
