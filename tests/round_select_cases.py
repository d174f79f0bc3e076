"""The selection rules of bbp_prove_round_select as a ten-line model, and the made-up score sets both tiers run through it: the CPU tier
(tests/test_round_select_host.py: csrc/round_select.h on the host) and the GPU tier (tests/test_gpu_round_select.py: the shipped
kernel through bbp_debug_round_select).  Scores are ints in [0, l); a floor is any int in [0, 2^256)."""
import random

from oracle.ref_py import ristretto as rs

L = rs.L
OK, FORMAT, BAD_ARG = 0, 3, 4
ALL_ONES = (1 << 256) - 1


def b32(x):
    return x.to_bytes(32, "little")


def model(scores, statuses, floor, K):
    """(sel in ascending index order, n_sel, n_qualified): include/bbp.h "Selecting a round's bids"."""
    q = [i for i, (s, st) in enumerate(zip(scores, statuses)) if st == OK and s >= floor]
    sel = q if K == 0 or len(q) <= K else sorted(sorted(q, key=lambda i: (-scores[i], i))[:K])
    return sel, len(sel), len(q)


def _grid(scores, statuses, floors=None, extra_K=()):
    """floors: 0, one bid's score, that score + 1, l, 2^256 - 1; K: 0, 1, |Q|, above |Q| (and extra_K)"""
    ok = [s for s, st in zip(scores, statuses) if st == OK]
    pick = sorted(ok)[len(ok) // 2] if ok else 7
    out = []
    for floor in floors if floors is not None else (0, pick, pick + 1, L, ALL_ONES):
        nq = model(scores, statuses, floor, 0)[2]
        for K in sorted({0, 1, max(nq, 1), nq + 3} | set(extra_K)):
            out.append((scores, statuses, floor, K))
    return out


def host_cases():
    rnd = random.Random(41)
    cases = []
    mixed = [rnd.randrange(L) for _ in range(23)]
    st = [OK] * 23
    for i in (2, 9, 10):
        st[i], mixed[i] = BAD_ARG, 0
    st[17], mixed[17] = FORMAT, 0
    cases += _grid(mixed, st, extra_K=(5, 18))
    cases += _grid([0] * 6, [BAD_ARG, FORMAT] * 3)                       # all bids refused
    cases += _grid([rnd.randrange(L)], [OK])                             # B = 1
    cases += _grid([0], [FORMAT])
    base = rnd.randrange(1 << 200)
    top = [base + (rnd.randrange(1, 1 << 28) << 224) for _ in range(12)]  # differ in the most significant word only ...
    low = [(base << 32) % (1 << 250) + rnd.randrange(1 << 32) for _ in range(12)]  # ... in the least significant only
    cases += _grid(top, [OK] * 12, extra_K=(3, 7)) + _grid(low, [OK] * 12, extra_K=(3, 7))
    # the two together: an order that reads the words the wrong way round ranks these differently
    both = [(1 << 224) + 5, (2 << 224) + 1, (1 << 224) + 9, 3, (2 << 224) + 0]
    cases += _grid(both, [OK] * 5, extra_K=(2, 3, 4))
    cases += _grid([12345] * 9, [OK] * 9, extra_K=(4,))                  # all scores equal
    dup = [50, 70, 60, 70, 60, 60, 10, 70, 60]                            # duplicates that straddle the K-th place
    cases += _grid(dup, [OK] * 9, floors=(0, 60, 61), extra_K=(2, 4, 5, 6))
    return cases


def cluster(B, seed, spread_bits):
    """B distinct scores that share everything above their lowest spread_bits bits (a 253-bit prefix)"""
    rnd = random.Random(seed)
    hi = (rnd.randrange(L >> 1) >> spread_bits) << spread_bits
    return [hi + v for v in rnd.sample(range(1 << spread_bits), B)]
