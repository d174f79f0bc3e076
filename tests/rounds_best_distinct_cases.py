"""The rules of bbp_verify_rounds_best_distinct (include/bbp.h "Best proofs of many rounds, one per bidder") as a model:
tests/round_best_distinct_cases.py's model per round, the indices mapped back, n_steps the most tranches any round ran, counted by a
simulation of its own.  Both tiers use it: the CPU tier (tests/test_rounds_best_distinct_host.py:
csrc/rounds_best_distinct.h on the host) and the GPU tier (tests/test_gpu_rounds_best_distinct.py).  Keys and floors are ints in
[0, 2^256); an id is the 32 raw z_img bytes of a row, and belongs to the row's round."""
import random

from tests import round_best_cases as bc
from tests import round_best_distinct_cases as dc
from tests import rounds_best_cases as mc

L = bc.L
OK, VERIFY, FORMAT, SKIPPED, DUPLICATE = dc.OK, dc.VERIFY, dc.FORMAT, dc.SKIPPED, dc.DUPLICATE


def tranches_run(keys, ids, verdicts, floor, K, tranche):
    """the tranches one round runs under the single-round one-per-bidder rule: a tranche of the live candidates, stop on K settled
    identities, else drop the live candidates of settled identities and double"""
    live = sorted((i for i, k in enumerate(keys) if floor <= k < L), key=lambda i: (-keys[i], i))
    T = max(tranche or bc.TRANCHE_DEFAULT, K) if K else len(live)
    settled, t = set(), 0
    while live:
        batch, live = live[:T], live[T:]
        settled |= {ids[i] for i in batch if verdicts[i] == OK}
        t, T = t + 1, 2 * T
        if K and len(settled) >= K:
            break
        live = [i for i in live if ids[i] not in settled]
    return t


def model(R, round_of, keys, ids, verdicts, floors, K, tranche):
    """(best: R lists in rank order, n_best[R], n_candidates[R], n_examined[R], n_duplicates[R], n_steps, status[B], ran[R]: the tranches
    every round ran); floors: None or R ints"""
    B = len(keys)
    status = [None] * B
    best, n_best, n_cand, n_exam, n_dups, ran = [], [], [], [], [], []
    by_round = [[] for _ in range(R)]
    for i in range(B):
        by_round[round_of[i]].append(i)
    for r, rows in enumerate(by_round):
        mine = ([keys[i] for i in rows], [ids[i] for i in rows], [verdicts[i] for i in rows], floors[r] if floors else 0, K, tranche)
        b, nb, nc, ne, nd, st = dc.model(*mine)
        best.append([rows[j] for j in b])
        n_best.append(nb), n_cand.append(nc), n_exam.append(ne), n_dups.append(nd)
        for j, i in enumerate(rows):
            status[i] = st[j]
        ran.append(tranches_run(*mine))
    return best, n_best, n_cand, n_exam, n_dups, max(ran, default=0), status, ran


# ---- three cases written out by hand from the rule as include/bbp.h states it ------------------------------------------------------------
A, B_, C = b"A" * 32, b"B" * 32, b"C" * 32
HAND_ROUND_OF = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
HAND_KEYS = [9, 9, 8, 8, 7, 7, 6, 6, 5, 5]
HAND_IDS = [A, A, A, B_, B_, A, C, B_, C, C]
HAND_ROW1_BAD = [OK, VERIFY, OK, OK, OK, OK, OK, OK, OK, OK]
#   (verdicts, K, tranche) -> best, n_candidates, n_examined, n_duplicates, n_steps, status
HAND_CASES = [
    # id A wins in both rounds: an identity belongs to its round
    (([OK] * 10, 2, 1), ([[0, 4], [1, 3]], [5, 5], [5, 2], [0, 0], 2, [0, 0, 0, 0, 0, -1, 0, -1, 0, -1])),
    # round 1's top claim fails: A is settled by row 5 only in the second tranche, row 7 (id B, settled by row 3) is dropped before it
    ((HAND_ROW1_BAD, 2, 1), ([[0, 4], [3, 5]], [5, 5], [5, 4], [0, 1], 2, [0, 1, 0, 0, 0, 0, 0, -2, 0, 0])),
    # K = 1: round 0 stops at step 0, and row 2 (its settled id A) stays SKIPPED, not DUPLICATE, while round 1 runs on
    ((HAND_ROW1_BAD, 1, 1), ([[0], [3]], [5, 5], [1, 3], [0, 0], 2, [0, 1, -1, 0, -1, 0, -1, -1, -1, -1])),
]


# ---- identities --------------------------------------------------------------------------------------------------------------------------
ID_SCHEMES = ("shared", "per_round")


def make_ids(B, R, round_of, scheme, n_ids, seed):
    """B ids.  "shared": drawn from ONE pool of n_ids identities whatever the round (the same bytes turn up in several rounds);
    "per_round": every round draws from a pool of n_ids identities of its own"""
    if scheme == "shared":
        return dc.id_pool(B, n_ids, seed)
    rnd = random.Random(seed)
    pools = [[rnd.randbytes(32) for _ in range(max(1, min(n_ids, B)))] for _ in range(R)]
    seen = [0] * R
    out = []
    for i in range(B):
        pool, r = pools[round_of[i]], round_of[i]
        out.append(pool[seen[r]] if n_ids >= B and seen[r] < len(pool) else pool[rnd.randrange(len(pool))])
        seen[r] += 1
    return out


def id_arms(B):
    """(scheme, n_ids) in the order both tiers draw them in turn: pools of 1, 3, B / 4 and B identities, shared and per round"""
    return [(scheme, n) for n in dc.id_pools(B) for scheme in ID_SCHEMES]


def host_cases():
    """(R, round_of, keys, ids, verdicts, floors, K, tranche) for the CPU tier: the maps, key sets and verdict mixes of
    rounds_best_cases.host_cases(), the ids drawn in turn from one pool shared by all rounds and from per-round pools"""
    cases = []
    for n, (R, ro, keys, verdicts, floors, K, tranche) in enumerate(mc.host_cases()):
        B = len(keys)
        scheme, n_ids = id_arms(B)[(n + n // 16) % 8]
        cases.append((R, ro, keys, make_ids(B, R, ro, scheme, n_ids, 3000 + n), verdicts, floors, K, tranche))
    return cases
