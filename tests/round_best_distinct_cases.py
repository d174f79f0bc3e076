"""The rules of bbp_verify_round_best_distinct (include/bbp.h "Best proofs of a round, one per bidder") as a twenty-line model, and the
made-up identities both tiers run through it: the CPU tier (tests/test_round_best_distinct_host.py: csrc/round_best.h on the host) and the
GPU tier (tests/test_gpu_round_best_distinct.py: the shipped kernels through bbp_debug_round_best_distinct, the verifier through the
public forms).  Keys and the floor are ints in [0, 2^256); an id is the 32 raw z_img bytes of a row (any hashable value will do for the
model); a verdict is what verification says of a row: OK, VERIFY or FORMAT."""
import random

from tests import round_best_cases as bc

L = bc.L
OK, VERIFY, FORMAT, SKIPPED, DUPLICATE = bc.OK, bc.VERIFY, bc.FORMAT, bc.SKIPPED, -2
b32 = bc.b32


def model(keys, ids, verdicts, floor, K, tranche):
    """(best in rank order, n_best, n_candidates, n_examined, n_duplicates, status)"""
    status = [FORMAT if k >= L else SKIPPED for k in keys]
    live = sorted((i for i, k in enumerate(keys) if floor <= k < L), key=lambda i: (-keys[i], i))
    nc, T = len(live), (max(tranche or bc.TRANCHE_DEFAULT, K) if K else len(live))
    settled, holders, examined, dups = set(), [], 0, 0
    while live:
        batch, live = live[:T], live[T:]
        for i in batch:
            status[i] = verdicts[i]
            examined += 1
            if verdicts[i] == OK and ids[i] not in settled:
                settled.add(ids[i])
                holders.append(i)
        T *= 2
        if K and len(holders) >= K:
            break
        keep = []
        for i in live:
            if ids[i] in settled:
                status[i] = DUPLICATE
                dups += 1
            else:
                keep.append(i)
        live = keep
    best = holders[:K] if K else holders
    return best, len(best), nc, examined, dups, status


def id_pool(B, n_ids, seed):
    """B ids drawn from n_ids distinct identities (n_ids >= B: every row its own)"""
    rnd = random.Random(seed)
    pool = [rnd.randbytes(32) for _ in range(max(1, n_ids))]
    assert len(set(pool)) == len(pool)
    if n_ids >= B:
        return pool[:B]
    return [pool[rnd.randrange(len(pool))] for _ in range(B)]


def id_pools(B):
    """the pool sizes both tiers use: 1 identity, 3, B / 4 and B"""
    return (1, 3, max(1, B // 4), B)


def host_cases():
    """(keys, ids, verdicts, floor, K, tranche) for the CPU tier: the key sets and verdict mixes of round_best_cases.host_cases, the ids
    drawn in turn from pools of 1, 3, B / 4 and B identities"""
    cases = []
    for n, (keys, verdicts, floor, K, tranche) in enumerate(bc.host_cases()):
        B = len(keys)
        cases.append((keys, id_pool(B, id_pools(B)[(n + n // 8) % 4], 1000 + n), verdicts, floor, K, tranche))
    # ... and cases that ask for more identities than a tranche can settle, so rows are dropped between tranches
    rnd = random.Random(47)
    for B, kind in ((9, bc.keys_low_byte), (23, bc.keys_uniform), (40, bc.keys_edges)):
        keys = kind(B, 200 + B)
        for n_ids in (3, max(1, B // 4)):
            for verdicts in ([OK] * B, bc.verdicts_top_third_bad(keys), [rnd.choice((OK, OK, VERIFY, FORMAT)) for _ in range(B)]):
                for K, tranche in ((4, 1), (5, 2), (2, 1)):
                    cases.append((keys, id_pool(B, n_ids, 2000 + len(cases)), verdicts, 0, K, tranche))
    return cases
