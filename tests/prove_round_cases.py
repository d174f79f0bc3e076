"""Rounds of raw bids for the bbp_prove_round tests, with what every output must be according to the big-int oracle (oracle/ref_py):
shared by the CPU tier (tests/test_prove_round_host.py, the header compiled for the host) and the GPU tier (tests/test_gpu_prove_round.py)."""
import hashlib
import random

from oracle.ref_py import blindbid as bb
from oracle.ref_py import ristretto as rs

L = rs.L
OK, FORMAT, BAD_ARG = 0, 3, 4
_C = bb.mimc_constants()


def b32(x):
    return x.to_bytes(32, "little")


class Round:
    """seed and items are 32-byte strings (raw, as they travel); bids a list of (d, k) ints; expect[i] = (status, toggle, witness)."""

    def __init__(self, N, seed, items, bids, expect):
        self.N, self.seed, self.items, self.bids, self.expect = N, seed, items, bids, expect
        self.B = len(bids)
        self.table = seed + b"".join(items)
        self.bid_bytes = b"".join(b32(d) + b32(k) for d, k in bids)
        self.status = [e[0] for e in expect]
        self.toggles = [e[1] for e in expect]

    def in_row(self, i):
        """bbp_prove_batch's input row of bid i: d,k,y,y_inv,q,z_img,seed || pub_list || toggle; all zero for a refused bid"""
        st, toggle, w = self.expect[i]
        if st != OK:
            return bytes(7 * 32 + 32 * self.N + 8)
        d, k = self.bids[i]
        return (b32(d) + b32(k) + b32(w["y"]) + b32(w["y_inv"]) + b32(w["q"]) + b32(w["z_img"]) + self.seed + b"".join(self.items)
                + toggle.to_bytes(8, "little"))

    def in_rows(self):
        return b"".join(self.in_row(i) for i in range(self.B))

    def tail(self, i):
        """score || z_img of bid i (zero for a refused bid)"""
        st, _, w = self.expect[i]
        return bytes(64) if st != OK else b32(w["q"]) + b32(w["z_img"])

    def rows(self, records):
        """record || score || z_img rows from B records packed back to back (zero rows for refused bids)"""
        rec = len(records) // self.B
        return b"".join((records[rec * i:rec * (i + 1)] + self.tail(i)) if self.status[i] == OK else bytes(rec + 64) for i in range(self.B))


def entropy(tag, B, N):
    """B rows of explicit prove entropy: 4 + N canonical blindings and a 32-byte rng seed each"""
    def h(i, j):
        return hashlib.sha512(b"bbp-round-ent" + tag.to_bytes(4, "little") + i.to_bytes(4, "little") + j.to_bytes(4, "little")).digest()
    return b"".join(b"".join(rs.sc_bytes(rs.sc_wide(h(i, j))) for j in range(4 + N)) + h(i, 4 + N)[:32] for i in range(B))


def honest(N, B, tag):
    """B accepted bids of one round: min(N, B) distinct bids sit at distinct list indices that include 0 and N - 1, bid i is distinct
    bid i mod that count (N = 1: every bid is the same bid -- one item can hold one x)."""
    rnd = random.Random(1000 * N + tag)
    seed = rnd.randrange(L)
    n = min(N, B)
    idx = [0, N - 1] + rnd.sample(range(1, N - 1), n - 2) if n >= 2 else [0]
    rnd.shuffle(idx)
    distinct = [(rnd.getrandbits(64), rnd.randrange(L)) for _ in range(n)]
    ws = [bb.witness(d, k, seed, _C) for d, k in distinct]
    items = [b32(rnd.randrange(L)) for _ in range(N)]
    for j in range(n):
        items[idx[j]] = b32(ws[j]["x"])
    bids = [distinct[i % n] for i in range(B)]
    expect = [(OK, idx[i % n], ws[i % n]) for i in range(B)]
    return Round(N, b32(seed), items, bids, expect)


def status_round(seed=None):
    """The statuses case, N = 8, B = 8: 0 x at indices 2 and 5 -> toggle 2; 1 x not in the list -> 4; 2 d = l -> 3; 3 k = l -> 3; 4 its item
    stored as x + l (index 0); 5 its item stored with bit 255 set (index 7); 6, 7 plain (indices 1, 3).  seed: an int (l: every row 3)."""
    rnd = random.Random(88)
    N = 8
    s = rnd.randrange(L) if seed is None else seed
    bids = [(rnd.getrandbits(64), rnd.randrange(L)) for _ in range(8)]
    bids[2] = (L, bids[2][1])
    bids[3] = (bids[3][0], L)
    ws = [bb.witness(d % L, k % L, s % L, _C) for d, k in bids]
    x = [w["x"] for w in ws]
    items = [b32(x[4] + L), b32(x[6]), b32(x[0]), b32(x[7]), b32(rnd.randrange(L)), b32(x[0]), b32(rnd.randrange(L)), b32(x[5] | (1 << 255))]
    expect = [(OK, 2, ws[0]), (BAD_ARG, 0, None), (FORMAT, 0, None), (FORMAT, 0, None), (OK, 0, ws[4]), (OK, 7, ws[5]), (OK, 1, ws[6]), (OK, 3, ws[7])]
    if s >= L:
        expect = [(FORMAT, 0, None)] * 8
    return Round(N, b32(s), items, bids, expect)


def subset(r, keep):
    """The round with only the bids `keep` (same table)"""
    return Round(r.N, r.seed, r.items, [r.bids[i] for i in keep], [r.expect[i] for i in keep])
