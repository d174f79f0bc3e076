"""The rules of bbp_verify_round_best (include/bbp.h "Best valid proofs of a round") as a fifteen-line model, and the made-up key sets both
tiers run through it: the CPU tier (tests/test_round_best_host.py: csrc/round_best.h on the host) and the GPU tier
(tests/test_gpu_round_best.py: the shipped kernels through bbp_debug_round_best, the verifier through the two public forms).  Keys and the
floor are ints in [0, 2^256); a verdict is what verification says of a row: OK, VERIFY or FORMAT."""
import random

from oracle.ref_py import ristretto as rs

L = rs.L
OK, VERIFY, FORMAT, SKIPPED = 0, 1, 3, -1
ALL_ONES = (1 << 256) - 1
TRANCHE_DEFAULT = 16  # BBP_BEST_TRANCHE_DEFAULT


def b32(x):
    return x.to_bytes(32, "little")


def model(keys, verdicts, floor, K, tranche):
    """(best in rank order, n_best, n_candidates, n_examined, status)"""
    status = [FORMAT if k >= L else SKIPPED for k in keys]
    cand = sorted((i for i, k in enumerate(keys) if floor <= k < L), key=lambda i: (-keys[i], i))
    T = max(tranche or TRANCHE_DEFAULT, K) if K else len(cand)
    at, ok = 0, []
    while at < len(cand):
        for i in cand[at:at + T]:
            status[i] = verdicts[i]
            ok += [i] if verdicts[i] == OK else []
        at, T = min(at + T, len(cand)), 2 * T
        if K and len(ok) >= K:
            break
    best = ok[:K] if K else ok
    return best, len(best), len(cand), at, status


def max_tranches(n_candidates, T0):
    """ceil(log2(n_candidates / T0 + 1)): the least t with T0 (2^t - 1) >= n_candidates"""
    t = 0
    while T0 * ((1 << t) - 1) < n_candidates:
        t += 1
    return t


def examined_after(n_candidates, T0, tranches):
    return min(n_candidates, T0 * ((1 << tranches) - 1))


def keys_uniform(B, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(L) for _ in range(B)]


def keys_low_byte(B, seed):
    """equal on their top 31 bytes: every radix pass of the selection works"""
    rnd = random.Random(seed)
    hi = (rnd.randrange(L >> 1) >> 8) << 8
    return [hi + rnd.randrange(256) for _ in range(B)]


def keys_edges(B, seed):
    """keys at l - 1, l and 2^256 - 1 among uniform ones"""
    keys = keys_uniform(B, seed)
    for j, v in enumerate((L - 1, L, ALL_ONES, L - 1, L + 1)):
        if j < B:
            keys[(7 * j + 1) % B] = v
    return keys


def verdicts_top_third_bad(keys, floor=0):
    """bad (alternating VERIFY, FORMAT) on exactly the top third of the candidates"""
    cand = sorted((i for i, k in enumerate(keys) if floor <= k < L), key=lambda i: (-keys[i], i))
    v = [OK] * len(keys)
    for n, i in enumerate(cand[:len(cand) // 3]):
        v[i] = (VERIFY, FORMAT)[n % 2]
    return v


def host_cases():
    """(keys, verdicts, floor, K, tranche) for the CPU tier: more than 60"""
    rnd = random.Random(43)
    cases = []
    for B, kind in ((1, keys_uniform), (2, keys_edges), (9, keys_low_byte), (23, keys_uniform), (23, keys_edges), (40, keys_low_byte)):
        keys = kind(B, 100 + B)
        pick = sorted(keys)[B // 2]
        for verdicts in ([OK] * B, [VERIFY] * B, verdicts_top_third_bad(keys), [rnd.choice((OK, VERIFY, FORMAT)) for _ in range(B)]):
            for floor, K, tranche in ((0, 1, 1), (0, 0, 4), (pick, 3, 1), (pick + 1, 2, 4), (0, B, 0), (L, 1, 1), (0, 3, 2 * B), (ALL_ONES, 0, 0)):
                cases.append((keys, verdicts, floor, K, tranche))
    cases.append(([12345] * 11, [VERIFY, OK] * 5 + [OK], 0, 2, 1))  # all keys equal: the index alone orders them
    cases.append(([12345] * 11, [VERIFY] * 11, 12345, 1, 3))
    return cases
