"""The rules of a standing (include/bbp.h "Standing of a round") as a short model, and the statement they add up to (truth), for both
tiers: the CPU tier (tests/test_round_standing_host.py: csrc/round_standing.h on the host) and the GPU tier
(tests/test_gpu_round_standing.py: the shipped kernels through bbp_debug_standing_offer, the verifier through bbp_standing_offer).
Keys and the floor are ints in [0, 2^256); an id is the 32 raw z_img bytes of a row; a verdict is what verification says of a row."""
import random

from tests import round_best_distinct_cases as dc

bc = dc.bc
L = dc.L
OK, VERIFY, FORMAT, SKIPPED, DUPLICATE = dc.OK, dc.VERIFY, dc.FORMAT, dc.SKIPPED, dc.DUPLICATE
b32 = dc.b32
MAX_K, MAX_OPEN = 1024, 64


def _rank(entry):
    return (-entry[0], entry[2])


class Standing:
    """entries: (key, id, serial) in rank order -- key descending, then serial ascending; offered: the rows offered so far"""

    def __init__(self, floor, K):
        assert 1 <= K <= MAX_K
        self.floor, self.K, self.entries, self.offered = floor, K, [], 0

    def offer(self, keys, ids, verdicts, tranche):
        """(entered in rank order, n_entered, n_candidates, n_examined, n_duplicates, status); an offer of no rows changes nothing"""
        K, base, B = self.K, self.offered, len(keys)
        entries = list(self.entries)

        def passes(j):  # the third screening test: not full, or (key, serial) comes before entry K-1
            return len(entries) < K or (-keys[j], base + j) < _rank(entries[K - 1])

        status = [FORMAT if k >= L else SKIPPED for k in keys]
        live = sorted((j for j, k in enumerate(keys) if self.floor <= k < L and passes(j)), key=lambda j: (-keys[j], j))
        nc, T = len(live), max(tranche or bc.TRANCHE_DEFAULT, K)
        examined = dups = 0

        def leave(rows):
            nonlocal dups
            by_id = {e[1]: e for e in entries}
            keep = []
            for j in rows:
                if not passes(j):
                    continue  # stays SKIPPED
                held = by_id.get(ids[j])
                if held and _rank(held) < (-keys[j], base + j):
                    status[j] = DUPLICATE
                    dups += 1
                else:
                    keep.append(j)
            return keep

        live = leave(live)
        self.tranches = 0  # of the last offer (tools/round_best.py counts the round tables that travel)
        while live:
            batch, live = live[:T], live[T:]
            T *= 2
            self.tranches += 1
            by_id = {e[1]: e for e in entries}
            for j in batch:
                status[j] = verdicts[j]
                examined += 1
                mine = (keys[j], ids[j], base + j)
                if verdicts[j] == OK and (ids[j] not in by_id or _rank(mine) < _rank(by_id[ids[j]])):
                    by_id[ids[j]] = mine  # enters, or replaces the entry of its identity that it comes before
            entries = sorted(by_id.values(), key=_rank)[:K]
            live = leave(live)
        self.entries, self.offered = entries, base + B
        entered = [e[2] - base for e in entries if e[2] >= base]
        return entered, len(entered), nc, examined, dups, status


def truth(keys, ids, verdicts, floor, K):
    """What the entries must be after ANY sequence of offers that delivered these rows in this order (serial = index): per identity the
    first OK row at or above the floor in rank order, then the first K of those in rank order -- (key, id, serial) each."""
    first = {}
    for s, (k, i, v) in enumerate(zip(keys, ids, verdicts)):
        if v == OK and floor <= k < L and (i not in first or (-k, s) < _rank(first[i])):
            first[i] = (k, i, s)
    return sorted(first.values(), key=_rank)[:K]


def cuts(B, n_bursts, rnd):
    """B rows as n_bursts consecutive slices cut at random points (equal points give an empty burst)"""
    at = sorted(rnd.randrange(B + 1) for _ in range(n_bursts - 1))
    return [slice(a, b) for a, b in zip([0] + at, at + [B])]


def host_cases():
    """the K >= 1 cases of round_best_distinct_cases.host_cases(): (keys, ids, verdicts, floor, K, tranche)"""
    return [c for c in dc.host_cases() if c[4] >= 1]


def run_bursts(case, bursts):
    """the model over `bursts` (slices): the per-burst results, and the entries after each burst"""
    keys, ids, verdicts, floor, K, tranche = case
    st, out = Standing(floor, K), []
    for sl in bursts:
        out.append((st.offer(keys[sl], ids[sl], verdicts[sl], tranche), list(st.entries), st.offered))
    return out


def self_check():
    """the model against truth and against the one-shot model, over host_cases: run by the CPU tier before anything is held to it"""
    rnd = random.Random(5)
    n_first = n_cut = 0
    for case in host_cases():
        keys, ids, verdicts, floor, K, tranche = case
        (got, entries, offered), = run_bursts(case, [slice(0, len(keys))])
        assert got == dc.model(keys, ids, verdicts, floor, K, tranche), case
        assert entries == truth(keys, ids, verdicts, floor, K) and offered == len(keys)
        n_first += 1
        for _ in range(4):
            bursts = cuts(len(keys), rnd.randrange(1, 5), rnd)
            for (res, entries, offered), sl in zip(run_bursts(case, bursts), bursts):
                assert entries == truth(keys[:sl.stop], ids[:sl.stop], verdicts[:sl.stop], floor, K), (case, bursts)
                assert res[3] + res[4] <= res[2] and offered == sl.stop
            n_cut += 1
    return n_first, n_cut
