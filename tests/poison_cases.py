"""Shared builders of tests/test_gpu_poisoned_scratch.py: the poison words, the warm / poison / call pattern, rows proved by the C oracle
and the rows of the verify, round-best and standing cases with the oracle's verdict on each.

Scratch discipline: a call reads only what it wrote itself, the resident tables, or state csrc/secret_map.h exempts.
bbp_debug_poison_scratch fills everything else with a small word, so a kernel that reads a row, counter or bucket it did not write
returns a wrong byte.  Every reference here is the C oracle or the Python model of the family; nothing is held against the engine's
own earlier output alone."""
import os
import re
import types

from tests import prove_round_cases as rc
from tests import round_best_cases as bc
from tests import test_gpu_verify_mixed as vm

# Small words only: a scalar of such limbs is canonical and non-zero, a status of 1 or 3 is a real error code, and an index or count read
# from the fill stays inside the 4096-byte allocation slack.  Two words, because one alone can happen to be neutral (a weight of 1).
WORDS = (1, 3)
OK, VERIFY, FORMAT, BAD_ARG, SKIPPED, DUPLICATE = 0, 1, 3, 4, -1, -2
L = vm.L
G = 8          # aggregation group of the verify cases: B = 33 and B = 130 both end in a ragged group
WARM_CALLS = 5  # a call family rotates over at most four buffers (three prove buffers and staging slots, four verifier lanes)


def pattern(word):
    """the 16 bytes bbp_debug_secret_scan looks for after a poison: the word four times"""
    return word.to_bytes(4, "little") * 4


def allocations(c):
    """how many scratch allocations the context has made since it was created (bbp_describe)"""
    m = re.search(r"in (\d+) allocation\(s\) since bbp_init", c.describe())
    assert m, c.describe()
    return int(m.group(1))


class Poisoned:
    """`with Poisoned(c, word):` fills the context's scratch, runs the body, and then holds the context to the two things every case
    asks: the call under test allocated nothing (it ran over filled memory only: the warm call was large enough), and no health flag."""

    def __init__(self, c, word, grows=False):
        self.c, self.word, self.grows = c, word, grows

    def __enter__(self):
        self.filled = self.c.debug_poison_scratch(self.word)
        self.allocs = allocations(self.c)
        return self

    def __exit__(self, kind, value, tb):
        if kind is None:
            assert self.grows or allocations(self.c) == self.allocs, "the call under test allocated: its warm call was too small"
            assert self.c.health() == 0
        return False


def knob_context(bbp, knobs):
    """a context made with `knobs` in the environment (read by bbp_init), the environment restored"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        return bbp.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def filled(n, byte=0x6E):
    import torch
    return torch.full((max(n, 1),), byte, dtype=torch.uint8, device="cuda")


# ---- prove -------------------------------------------------------------------------------------------------------------------------------
def proved_rows(oc, bbp, B, N, seed):
    """B distinct prove rows at list length N with fixed entropy and the C oracle's records: row i does not depend on its batch"""
    ins, ents, tails = vm._synth(oc, B, N, seed=seed)
    out, st = oc.prove_many(b"".join(ins), b"".join(ents), B, N, threads=16)
    assert st == [OK] * B
    rs_ = bbp.record_size(N)
    return types.SimpleNamespace(N=N, B=B, ins=ins, ents=ents, tails=tails, rs=rs_, records=[out[i * rs_:(i + 1) * rs_] for i in range(B)])


def prove_args(p, B):
    return B, p.N, b"".join(p.ins[:B]), b"".join(p.ents[:B])


def tiled(p, B):
    """B rows by repetition of p's (warm calls: the result is not looked at beyond its statuses)"""
    return B, p.N, b"".join(p.ins[i % p.B] for i in range(B)), b"".join(p.ents[i % p.B] for i in range(B))


# ---- verify ------------------------------------------------------------------------------------------------------------------------------
def verify_rounds_of(oc, proved, Ns):
    """tests/test_gpu_verify_plan.py's rounds (one oracle-proved row and its t_x + 1 copy per N) with a third variant each: the score
    raised by l, a non-canonical scalar -- FORMAT by the oracle"""
    out = []
    for n in Ns:
        p = proved[n]
        bad = vm._tamper(p.full[0], n, "noncanon")
        assert oc.verify_many(bad, 1, n, threads=1) == [FORMAT]
        full = list(p.full) + [bad]
        rsz = len(p.variants[0]) - 64
        out.append(types.SimpleNamespace(N=n, full=full, variants=[r[:rsz + 64] for r in full], verdict=list(p.verdict) + [FORMAT], table=p.table))
    return out


NONCANON_AT = 5  # a row of the first group


def verify_picks(B, n_rounds):
    """row i belongs to round i % n_rounds; the last row is the tampered one, row NONCANON_AT the non-canonical one"""
    return [(i % n_rounds, 1 if i == B - 1 else 2 if i == NONCANON_AT else 0) for i in range(B)]


def verify_want(B):
    want = [OK] * B
    want[B - 1], want[NONCANON_AT] = VERIFY, FORMAT
    return want


def expected_fallback(B, want):
    return vm._expected_fallback([0] * B, want, G, {B - 1})


# ---- rounds of short rows with the oracle's verdicts -------------------------------------------------------------------------------------
T_X = 257


def set_score(row, N, value):
    rs_ = 1121 + 32 * (4 + N)
    return row[:rs_] + bc.b32(value) + row[rs_ + 32:]


def score_of(row, N):
    rs_ = 1121 + 32 * (4 + N)
    return int.from_bytes(row[rs_:rs_ + 32], "little")


def tamper(row, N, kind):
    b = bytearray(row)
    if kind == "flip":      # a flipped record byte (t_x): VERIFY
        b[T_X] ^= 0x01
        return bytes(b)
    if kind == "top":       # a claimed score raised to l - 1: a forged top claim, VERIFY, the first row examined
        return set_score(row, N, L - 1)
    if kind == "score_l":   # a score >= l: FORMAT, never examined
        return set_score(row, N, score_of(row, N) + L)
    raise KeyError(kind)


class OracleRound:
    """B short rows (record || score || z_img) of one round by repetition of n_bids bids proved by the C oracle, some tampered, and the
    oracle's verdict on every row"""

    def __init__(self, oc, bbp, N, n_bids, B, tag, tampered):
        r = rc.honest(N, n_bids, tag)
        ent = rc.entropy(tag, n_bids, N)
        recs, st = oc.prove_many(r.in_rows(), ent, n_bids, N, threads=16)
        assert st == [OK] * n_bids
        size = bbp.round_row_size(N)
        rows = r.rows(recs)
        base = [rows[size * i:size * (i + 1)] for i in range(n_bids)]
        self.N, self.B, self.size, self.table, self.round, self.entropy = N, B, size, r.table, r, ent
        self.honest_rows = rows
        self.row_list = [base[i % n_bids] for i in range(B)]
        for i, kind in tampered.items():
            self.row_list[i] = tamper(self.row_list[i], N, kind)
        self.rows = b"".join(self.row_list)
        self.keys = [score_of(x, N) for x in self.row_list]
        self.ids = [x[-32:] for x in self.row_list]
        self.verdicts = oc.verify_many(b"".join(x + r.table for x in self.row_list), B, N, threads=16)
