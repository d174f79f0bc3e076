"""The rule of one offer to many standings (include/bbp.h "Standings of many rounds") as a short model, for both tiers: the CPU tier
(tests/test_standings_host.py: csrc/standings.h on the host) and the GPU tier (tests/test_gpu_standings.py: the shipped kernels through
bbp_debug_standings_offer, the verifier through bbp_standings_offer).  The model is S instances of tests/round_standing_cases.py's
Standing, each offered its own rows in ascending call index, local indices mapped back to call indices."""
import random

from tests import round_standing_cases as sc

dc = sc.dc
L = sc.L
OK, VERIFY, FORMAT, SKIPPED, DUPLICATE = sc.OK, sc.VERIFY, sc.FORMAT, sc.SKIPPED, sc.DUPLICATE
b32 = sc.b32


def offer(stands, standing_of, keys, ids, verdicts, tranche):
    """one offer to the Standings `stands`: (per standing [entered as call indices, n_entered, n_candidates, n_examined, n_duplicates],
    n_steps, the B statuses).  A standing that receives no row is offered nothing and reports zeros."""
    B = len(keys)
    status, per, steps = [None] * B, [], 0
    for s, st in enumerate(stands):
        rows = [i for i in range(B) if standing_of[i] == s]
        st.tranches = 0
        ent, ne, nc, nx, nd, stat = st.offer([keys[i] for i in rows], [ids[i] for i in rows], [verdicts[i] for i in rows], tranche)
        per.append([[rows[j] for j in ent], ne, nc, nx, nd])
        for j, i in enumerate(rows):
            status[i] = stat[j]
        steps = max(steps, st.tranches)
    return per, steps, status


def random_offer(rnd, S, B, pool, key_bits=12, ok=0.8):
    """B rows for S standings: keys with many ties, ids drawn from `pool` (shared by all standings: one z_img in several standings),
    mostly valid; a few keys at or above l"""
    standing_of = [rnd.randrange(S) for _ in range(B)]
    keys = [L + rnd.randrange(3) if rnd.random() < 0.03 else rnd.randrange(1, 1 << key_bits) for _ in range(B)]
    ids = [rnd.choice(pool) for _ in range(B)]
    verdicts = [OK if rnd.random() < ok else rnd.choice((VERIFY, FORMAT)) for _ in range(B)]
    return standing_of, keys, ids, verdicts


def random_sequences(seed, n_seq, max_S=8, Ks=(1, 3, 16), max_B=40):
    """[(Ks per standing, floors, [(standing_of, keys, ids, verdicts, tranche, cap)])]: sequences of offers with resends"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n_seq):
        S = rnd.randrange(1, max_S + 1)
        ks = [rnd.choice(Ks) for _ in range(S)]
        floors = [rnd.choice((0, 0, 1 << 6)) for _ in range(S)]
        pool = [rnd.randbytes(32) for _ in range(rnd.randrange(2, 24))]
        offers, sent = [], []
        for _ in range(rnd.randrange(2, 6)):
            B = rnd.randrange(0, max_B)
            so, keys, ids, verdicts = random_offer(rnd, S, B, pool)
            for j in range(B):  # resends: a row offered before, to the same standing or to another
                if sent and rnd.random() < 0.25:
                    s0, k0, i0, v0 = rnd.choice(sent)
                    so[j], keys[j], ids[j], verdicts[j] = (s0 if rnd.random() < 0.7 else rnd.randrange(S)), k0, i0, v0
            sent += list(zip(so, keys, ids, verdicts))
            offers.append((so, keys, ids, verdicts, rnd.choice((0, 1, 2, 5, 64)), rnd.choice((B, B, 1, 0))))
        out.append((ks, floors, offers))
    return out
