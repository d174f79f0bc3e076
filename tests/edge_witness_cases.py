"""Witnesses and blindings at their edges for the prove / verify tests (tests/test_edge_witness_host.py, tests/test_gpu_edge_witness.py,
tests/golden/make_golden.py --edge): d, k, seed in {0, 1, l - 1, 2^64 - 1, 2^64}, blindings that are zero, one, l - 1, carry patterns or
not reduced at all (ff..ff, l, l + 1, 2^255), lists whose items are all x or zero.  With a zero blinding V = v * B, so a zero value
commits to the identity: 32 zero bytes in the record.  Witnesses come from `oc.witness` (the C oracle, or anything with that method).

A case is a list of rows (one, but for d_wide).  A row is a dict in the layout of tests/prove_check_cases.py -- f = [d, k, y, y_inv, q,
z_img, seed] as ints, pub (32-byte items), toggle, x -- plus name, N, ent (the entropy row: 4 + N blindings as they travel, then the
32-byte rng seed) and the properties the case exists for, DECLARED here and checked on the oracle's record by the CPU tier:
identity_V (the commitment slots V_0 .. V_{3+N} that must be 32 zero bytes; 0 = d, 1 = k, 2 = y, 3 = y_inv, 4 + i = list bit i) and
score_zero (q == 0).  The seven scalars stay canonical (the host path refuses others); only the entropy is not."""
import hashlib

from oracle.ref_py import ristretto as rs
from tests import scalarmul_cases as smc

L = rs.L
FF = (1 << 256) - 1
D, K, Y, YI, Q, Z, SEED = range(7)
P7778 = smc.NAMED["777..78"]
CARRY = [P7778, smc.NAMED["777..77"], P7778 + 1, 1 << 252, (1 << 252) - 1, (1 << 252) + 1, smc.NAMED["all_9"], smc.NAMED["chain40"]]
NONCANON = [FF, L, L + 1, 1 << 255]
assert all(v < L for v in CARRY) and all(v >= L for v in NONCANON)

# name -> (N, toggle): the shapes of the GPU tier
TABLE = {"zero": (3, 1), "d0": (3, 0), "zero_blind": (3, 2), "one": (3, 0), "max": (3, 2), "d_wide": (3, 1), "noncanon_blind": (3, 1),
         "carry": (3, 0), "same_items": (8, 7), "zero_items": (8, 3), "n1_zero": (1, 0), "n202_zero_blind": (202, 101)}
# (name, N, toggle) of tests/golden/proofs_edge.json, proved by the big-int oracle
GOLDEN = [("zero", 2, 1), ("max", 1, 0), ("noncanon_blind", 1, 0)]


def b32(x):
    return x.to_bytes(32, "little")


def sc(b):
    return int.from_bytes(b, "little")


def _h(name, i, tag):
    return hashlib.sha512(b"bbp-edge-v1/" + name.encode() + b"/" + tag + i.to_bytes(4, "little")).digest()


def _scalar(name, i, tag):
    return rs.sc_wide(_h(name, i, tag))


def _bits(N, toggle):
    return {4 + i for i in range(N) if i != toggle}


def _row(oc, name, N, toggle, d, k, seed, blind, rng, identity_V=(), score_zero=False, items=None, stream=None):
    """blind: one int in [0, 2^256) for every blinding, or a list that is repeated to 4 + N; None = from the stream.  rng: 32 bytes or
    None.  items(x, pub): the list to use instead of the stream's (pub[toggle] is x already)."""
    stream = stream or name
    w = oc.witness(b32(d) + b32(k) + b32(seed))
    m, x, y, yi, q, z = (sc(w[32 * j:32 * j + 32]) for j in range(6))
    pub = [b32(_scalar(stream, j, b"pub")) for j in range(N)]
    pub[toggle] = b32(x)
    if items is not None:
        pub = items(x, pub)
        assert len(pub) == N and sc(pub[toggle]) == x
    if blind is None:
        blind = [_scalar(stream, j, b"blind") for j in range(4 + N)]
    elif isinstance(blind, int):
        blind = [blind]
    blind = [blind[j % len(blind)] for j in range(4 + N)]
    rng = _h(stream, 0, b"rng")[:32] if rng is None else rng
    return dict(name=name, N=N, f=[d, k, y, yi, q, z, seed], pub=pub, toggle=toggle, x=x, ent=b"".join(b32(v) for v in blind) + rng,
                identity_V=frozenset(identity_V), score_zero=score_zero)


def build(oc, name, N=None, toggle=None):
    """The rows of case `name`, at the table's shape or at another (the golden file's)."""
    if N is None:
        N, toggle = TABLE[name]
    u64 = lambda tag: sc(_h(name, 0, tag)[:8])
    s = lambda tag: _scalar(name, 0, tag)
    if name in ("zero", "n1_zero"):
        return [_row(oc, name, N, toggle, 0, 0, 0, 0, bytes(32), {0, 1} | _bits(N, toggle), True, stream="zero")]
    if name == "d0":
        return [_row(oc, name, N, toggle, 0, s(b"k"), s(b"seed"), None, None, (), True)]
    if name in ("zero_blind", "n202_zero_blind"):
        return [_row(oc, name, N, toggle, u64(b"d"), s(b"k"), s(b"seed"), 0, None, _bits(N, toggle))]
    if name == "one":
        return [_row(oc, name, N, toggle, 1, 1, 1, 1, b32(1))]
    if name == "max":
        return [_row(oc, name, N, toggle, (1 << 64) - 1, L - 1, L - 1, L - 1, b32(FF))]
    if name == "d_wide":  # the circuit has no range constraint on d
        return [_row(oc, "%s/%s" % (name, tag), N, toggle, d, s(b"k"), s(b"seed"), None, None, stream="%s/%s" % (name, tag))
                for tag, d in (("2^64", 1 << 64), ("l-1", L - 1))]
    if name == "noncanon_blind":  # l reduces to zero, but sits on k (slot 1) and, at N = 3, on the toggled bit (slot 5): V_5 = B
        return [_row(oc, name, N, toggle, u64(b"d"), s(b"k"), s(b"seed"), NONCANON, b32(FF))]
    if name == "carry":
        return [_row(oc, name, N, toggle, u64(b"d"), P7778, s(b"seed"), CARRY, b32(P7778))]
    if name == "same_items":  # the toggle the caller names is honoured; bbp_prove_round would say 0
        return [_row(oc, name, N, toggle, u64(b"d"), s(b"k"), s(b"seed"), 0, None, _bits(N, toggle), items=lambda x, pub: [b32(x)] * N)]
    if name == "zero_items":
        return [_row(oc, name, N, toggle, u64(b"d"), s(b"k"), s(b"seed"), None, None,
                     items=lambda x, pub: [bytes(32) if j % 2 == 0 and j != toggle else p for j, p in enumerate(pub)])]
    raise KeyError(name)


def all_rows(oc, N=None):
    """Every row of the table in its order; N: only the cases of that list length."""
    return [r for name, (n, _t) in TABLE.items() if N is None or n == N for r in build(oc, name)]


def golden_rows(oc):
    return [build(oc, name, N, toggle)[0] for name, N, toggle in GOLDEN]


def scalars7(r):
    return b"".join(b32(v) for v in r["f"])


def pub_list(r):
    return b"".join(r["pub"])


def prove_row(r):
    """bbp_prove_batch input row: scalars7 || pub_list || toggle (u64 LE)."""
    return scalars7(r) + pub_list(r) + int(r["toggle"]).to_bytes(8, "little")


def tail(r):
    """What follows the record in a verify row: score || z_img || seed || pub_list."""
    f = r["f"]
    return b32(f[Q]) + b32(f[Z]) + b32(f[SEED]) + pub_list(r)


def v_slot(N, i):
    """Byte range of commitment V_i in a compact record of list length N."""
    at = 1121 + 32 * i
    assert 0 <= i < 4 + N
    return at, at + 32


def identity_slots(record, N):
    return {i for i in range(4 + N) if record[slice(*v_slot(N, i))] == bytes(32)}


def _put(b, lo, hi, v):
    assert len(v) == hi - lo
    return b[:lo] + v + b[hi:]


def tampered(r, record, enc_B, max_slots=3):
    """[(label, record, tail)]: copies of the valid verify row (record, tail(r)) that every verifier must refuse -- an identity V with
    bit 0 of byte 0 set (not an encoding), an identity V replaced by B, a non-identity V replaced by the identity, a zero score
    replaced by 1, and A_I1 replaced by the identity (which, unlike V, the reference's validate_and_append_point refuses outright).
    At most max_slots identity slots are used: the first, the last and the middle one."""
    N, t = r["N"], tail(r)
    ident = sorted(r["identity_V"])
    if len(ident) > max_slots:
        ident = sorted({ident[0], ident[len(ident) // 2], ident[-1]})
    out = []
    for i in ident:
        lo, hi = v_slot(N, i)
        out.append(("V%d bit0" % i, _put(record, lo, hi, b"\x01" + bytes(31)), t))
        out.append(("V%d = B" % i, _put(record, lo, hi, enc_B), t))
    other = min(set(range(4 + N)) - set(r["identity_V"]))
    out.append(("V%d = identity" % other, _put(record, *v_slot(N, other), bytes(32)), t))
    if r["score_zero"]:
        out.append(("score = 1", record, b32(1) + t[32:]))
    out.append(("A_I1 = identity", _put(record, 1, 33, bytes(32)), t))
    return out
