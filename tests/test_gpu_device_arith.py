"""gpu tier: the PRODUCT's field, scalar, point and Keccak code as hipcc compiles it for gfx950 (tests/device_check.hip over the
csrc/ headers), against the big-int oracle at the edges where limb code goes wrong.  On the device several paths are different code
from the host tier's (tests/test_host_arith.py): the inline-asm multiply and squaring chains, the v_alignbit rotations, the
one-wavefront permutation, the MSM row loads.  Every check runs for the library as shipped and for -DBBP_FE_NO_CHAIN (the separate
carry pass), with the value batteries of tests/arith_cases.py."""
import ctypes
import hashlib
import random

import pytest

from oracle.ref_py import merlin, ristretto as rs
from tests import arith_cases as ac
from tests.test_oracle_kat import RFC9496_MULTIPLES

pytestmark = pytest.mark.gpu

P, L = rs.P, rs.L
M64 = (1 << 64) - 1

_i32p, _u8p = ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p
SIGNATURES = {
    "dc_fe_op": [ctypes.c_int, ctypes.c_int, _u8p, _u8p, _u8p],
    "dc_fe_limbs": [ctypes.c_int, ctypes.c_int, _i32p, _i32p, _i32p, _u8p],
    "dc_sc_op": [ctypes.c_int, ctypes.c_int, _u8p, _u8p, _u8p],
    "dc_sc_is_canonical": [ctypes.c_int, _u8p, _i32p],
    "dc_sc_naf": [ctypes.c_int, ctypes.c_int, _u8p, _i32p, _i32p, _i32p],
    "dc_ge_op": [ctypes.c_int, ctypes.c_int, _u8p, _u8p, _u8p, _i32p],
    "dc_from_uniform": [ctypes.c_int, _u8p, _u8p],
    "dc_madd_row": [ctypes.c_int, _u8p, _u8p, ctypes.c_int, _u8p, _i32p],
    "dc_rotl64": [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)],
    "dc_rotl64_const": [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    "dc_keccak_f": [ctypes.c_int, _u8p],
    "dc_keccak_f_wave": [ctypes.c_int, _u8p, _u8p],
    "dc_merlin_rng_bulk": [ctypes.c_int, _u8p, ctypes.c_int, _u8p, ctypes.c_int, _u8p, _u8p, _i32p],
}
NAF_SLOT = 32  # device_check.hip


def load(path):
    lib = ctypes.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    return lib


class Dev:
    """batched calls into one device-check library; a non-zero hipError_t fails the test"""

    def __init__(self, lib, variant):
        self.lib, self.variant = lib, variant
        self.chain = variant == "chain"

    def _ok(self, rc, what):
        assert rc == 0, "%s (%s): hipError_t %d" % (what, self.variant, rc)

    def fe_op(self, op, pairs):
        n = len(pairs)
        a = b"".join((x & (2**256 - 1)).to_bytes(32, "little") for x, _ in pairs)
        b = b"".join((y & (2**256 - 1)).to_bytes(32, "little") for _, y in pairs)
        out = ctypes.create_string_buffer(32 * n)
        self._ok(self.lib.dc_fe_op(op, n, a, b, out), "dc_fe_op %d" % op)
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def fe_limbs(self, op, pairs):
        n = len(pairs)
        a = (ctypes.c_int32 * (10 * n))(*[x for v, _ in pairs for x in v])
        b = (ctypes.c_int32 * (10 * n))(*[x for _, v in pairs for x in v])
        o10, o32 = (ctypes.c_int32 * (10 * n))(), ctypes.create_string_buffer(32 * n)
        self._ok(self.lib.dc_fe_limbs(op, n, a, b, o10, o32), "dc_fe_limbs %d" % op)
        return [(list(o10[10 * i:10 * i + 10]), o32.raw[32 * i:32 * i + 32]) for i in range(n)]

    def sc_op(self, op, a_list, b_list=None):
        n = len(a_list)
        width = 64
        a = b"".join(x.to_bytes(width, "little") for x in a_list)
        b = b"".join(y.to_bytes(32, "little") for y in (b_list or [0] * n))
        out = ctypes.create_string_buffer(32 * n)
        self._ok(self.lib.dc_sc_op(op, n, a, b, out), "dc_sc_op %d" % op)
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def ge_op(self, op, a_list, b_list=None):
        n = len(a_list)
        out, st = ctypes.create_string_buffer(32 * n), (ctypes.c_int32 * n)()
        self._ok(self.lib.dc_ge_op(op, n, b"".join(a_list), b"".join(b_list or [bytes(32)] * n), out, st), "dc_ge_op %d" % op)
        return [out.raw[32 * i:32 * i + 32] if st[i] == 1 else None for i in range(n)]


VARIANTS = ("chain", "nochain")


@pytest.fixture(scope="module", params=VARIANTS)
def dev(request, built, bbp):  # bbp: torch's HIP runtime loads first (conftest.py)
    return Dev(load(built.build_devcheck(request.param)), request.param)


def b32(x):
    return x.to_bytes(32, "little")


# ---- field -------------------------------------------------------------------------------------------------------------------
def test_field_battery(dev):
    """everything test_host_arith.test_field_ops asserts, on the device's asm chains; inversion and pow22523 on every value"""
    M = ac.M255
    vals, pairs, _ = ac.field_cases()
    masked = [(a & M, b & M) for a, b in pairs]
    want = {0: [(a + b) % P for a, b in masked], 1: [(a - b) % P for a, b in masked], 2: [a * b % P for a, b in masked],
            8: [a * (b0 & 0x3ffffff) % P for (a, _), (_, b0) in zip(masked, pairs)], 10: [ac.field_growth(a, b) for a, b in masked]}
    for op, w in want.items():
        got = dev.fe_op(op, pairs)
        bad = [(hex(pairs[i][0]), hex(pairs[i][1])) for i in range(len(pairs)) if got[i] != w[i]]
        assert not bad, (dev.variant, op, len(bad), bad[:3])
    singles = [(a, 0) for a in vals]
    vm = [a & M for a in vals]
    want = {3: [a * a % P for a in vm], 9: [2 * a * a % P for a in vm], 5: [a % P for a in vm], 6: [(-a) % P for a in vm],
            4: [pow(a % P, P - 2, P) for a in vm], 7: [pow(a % P, (P - 5) // 8, P) for a in vm]}
    for op, w in want.items():
        got = dev.fe_op(op, singles)
        bad = [hex(vals[i]) for i in range(len(vals)) if got[i] != w[i]]
        assert not bad, (dev.variant, op, len(bad), bad[:3])


def test_field_limbs_at_the_documented_bounds(dev):
    """field.h's limb contract on the device: multiply / square / sq2 at the input bound (1.65 * 2^26 / 2^25, where 19 g_even and
    38 f_odd reach 0.98 * 2^31) give the right value with carried limbs; towords / iszero / isneg / eq near multiples of p agree
    with x % p"""
    counts = ac.check_fe_limbs(dev.fe_limbs, chain=dev.chain)
    assert min(counts.values()) >= 500, counts


# ---- scalars -----------------------------------------------------------------------------------------------------------------
def test_scalar_battery(dev):
    cs = ac.scalar_cases()
    a, b = [x for x, _ in cs["pairs"]], [y for _, y in cs["pairs"]]
    for op, f in ((0, lambda x, y: (x + y) % L), (1, lambda x, y: (x - y) % L), (2, lambda x, y: x * y % L)):
        got = dev.sc_op(op, a, b)
        bad = [(hex(x), hex(y)) for x, y, g in zip(a, b, got) if g != f(x, y)]
        assert not bad, (dev.variant, op, len(bad), bad[:3])
    assert dev.sc_op(6, cs["vals"]) == [(-x) % L for x in cs["vals"]]
    assert dev.sc_op(7, cs["fermat"]) == [pow(x, L - 2, L) for x in cs["fermat"]]
    got = dev.sc_op(3, cs["inv"])  # safegcd, including the 3000-value random sample; 0 -> 0
    bad = [hex(x) for x, g in zip(cs["inv"], got) if g != (pow(x, L - 2, L) if x else 0)]
    assert not bad, (dev.variant, len(bad), bad[:3])
    assert dev.sc_op(4, cs["wide"]) == [w % L for w in cs["wide"]]
    assert dev.sc_op(5, cs["bits"]) == [(w & (2**255 - 1)) % L for w in cs["bits"]]
    vals = cs["bits"] + [L - 1, L, 0]
    out = (ctypes.c_int32 * len(vals))()
    assert dev.lib.dc_sc_is_canonical(len(vals), b"".join(b32(w) for w in vals), out) == 0
    assert list(out) == [1 if w < L else 0 for w in vals]


def test_naf_recoding(dev):
    """sc_for_each_naf_digit as the MSM kernels run it (__builtin_ctzll on the device), widths 12 and 9"""
    vals = ac.naf_values()
    n = len(vals)
    raw = b"".join(b32(v) for v in vals)
    for width in (12, 9):
        pos, dig, cnt = (ctypes.c_int32 * (NAF_SLOT * n))(), (ctypes.c_int32 * (NAF_SLOT * n))(), (ctypes.c_int32 * n)()
        assert dev.lib.dc_sc_naf(width, n, raw, pos, dig, cnt) == 0
        total = 0
        for i, v in enumerate(vals):
            k = cnt[i]
            assert 0 <= k <= NAF_SLOT, (width, hex(v), k)
            ac.check_naf(width, v, pos[NAF_SLOT * i:NAF_SLOT * i + k], dig[NAF_SLOT * i:NAF_SLOT * i + k])
            total += k
        assert total / n < (20.5 if width == 12 else 26.5)


# ---- ristretto -----------------------------------------------------------------------------------------------------------------
def test_ristretto_codec(dev):
    """RFC 9496: the multiples of the basepoint decode and re-encode; every bad encoding is rejected BY THE DECODER (status 0), so a
    wrong accept cannot hide behind a later equation failing; from_uniform (elligator) agrees with the oracle"""
    good = [bytes.fromhex(h) for h in RFC9496_MULTIPLES]
    assert dev.ge_op(0, good) == good
    bad = [bytes.fromhex(h) for h in ac.BAD_ENCODINGS]
    assert dev.ge_op(0, bad) == [None] * len(bad)
    us = ac.uniform_inputs(200)
    out = ctypes.create_string_buffer(32 * len(us))
    assert dev.lib.dc_from_uniform(len(us), b"".join(us), out) == 0
    for i, u in enumerate(us):
        assert out.raw[32 * i:32 * i + 32] == rs.encode(rs.from_uniform_bytes(u)), (dev.variant, u.hex())


def test_point_ops(dev):
    """dbl, add, sub, madd, msub against the oracle, including the identity and P + (-P)"""
    pts, partners, _ = ac.point_cases()
    enc = [rs.encode(p) for p in pts]
    assert dev.ge_op(1, enc) == [rs.encode(rs.pt_dbl(p)) for p in pts]
    a_idx = [i for i in range(len(pts)) for _ in partners[i]] + list(range(len(pts)))
    b_idx = [j for i in range(len(pts)) for j in partners[i]] + list(range(len(pts)))  # the last block: P op P
    a_enc, b_enc = [enc[i] for i in a_idx], [enc[j] for j in b_idx]
    plus = [rs.encode(rs.pt_add(pts[i], pts[j])) for i, j in zip(a_idx, b_idx)]
    minus = [rs.encode(rs.pt_add(pts[i], rs.pt_neg(pts[j]))) for i, j in zip(a_idx, b_idx)]
    assert minus[-len(pts):] == [rs.encode(rs.IDENT)] * len(pts)
    for op, want in ((2, plus), (3, minus), (4, plus), (5, minus)):
        assert dev.ge_op(op, a_enc, b_enc) == want, (dev.variant, op)
    # P + (-P) through add and madd: -P encoded by the oracle
    neg_enc = [rs.encode(rs.pt_neg(p)) for p in pts]
    assert dev.ge_op(2, enc, neg_enc) == [rs.encode(rs.IDENT)] * len(pts)
    assert dev.ge_op(4, enc, neg_enc) == [rs.encode(rs.IDENT)] * len(pts)


def test_madd_row(dev):
    """the MSM accumulate step (point.h load_row_at + ge_madd_row): the accumulator with Z != 1 (decoded, doubled twice), the row
    built by niels_to_row into a 128-byte device row; neg = 0 adds the point, neg = 1 (y+x / y-x swapped by load offset) subtracts"""
    pts, partners, _ = ac.point_cases()
    acc = [pts[i] for i in range(len(pts)) for _ in partners[i]] + pts
    q = [pts[j] for i in range(len(pts)) for j in partners[i]] + [rs.pt_dbl(rs.pt_dbl(p)) for p in pts]  # Q = 4 P: neg = 1 -> identity
    acc4 = [rs.pt_dbl(rs.pt_dbl(p)) for p in acc]  # what the kernel accumulates onto (device_check.hip ROW_DOUBLINGS)
    n = len(acc)
    a_raw, q_raw = b"".join(rs.encode(p) for p in acc), b"".join(rs.encode(p) for p in q)
    for neg in (0, 1):
        out, st = ctypes.create_string_buffer(32 * n), (ctypes.c_int32 * n)()
        assert dev.lib.dc_madd_row(n, a_raw, q_raw, neg, out, st) == 0
        assert list(st) == [1] * n
        for i in range(n):
            want = rs.pt_add(acc4[i], rs.pt_neg(q[i]) if neg else q[i])
            assert out.raw[32 * i:32 * i + 32] == rs.encode(want), (dev.variant, neg, i)
    assert rs.encode(rs.pt_add(acc4[-1], rs.pt_neg(q[-1]))) == rs.encode(rs.IDENT)


# ---- Keccak ------------------------------------------------------------------------------------------------------------------
ROT_WORDS = [0, 1, 2, 1 << 31, 1 << 32, 1 << 63, M64, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x0123456789ABCDEF, 0xFFFFFFFF00000000]


def _rot_words():
    rnd = random.Random(50)
    return ROT_WORDS + [rnd.getrandbits(64) for _ in range(53)]


def test_rotl64_runtime_and_literal_amounts(dev):
    """keccak.h rotl64 for every amount 0..63: as a runtime kernel argument and as a literal (one instantiation per amount)"""
    words = _rot_words()
    n = len(words)
    x = (ctypes.c_uint64 * n)(*words)
    rot = lambda v, r: ((v << r) | (v >> (64 - r))) & M64 if r else v
    for r in range(64):
        out = (ctypes.c_uint64 * n)()
        assert dev.lib.dc_rotl64(n, x, r, out) == 0
        assert list(out) == [rot(v, r) for v in words], (dev.variant, "runtime", r)
    out = (ctypes.c_uint64 * (64 * n))()
    assert dev.lib.dc_rotl64_const(n, x, out) == 0
    for i, v in enumerate(words):
        assert list(out[64 * i:64 * i + 64]) == [rot(v, r) for r in range(64)], (dev.variant, "literal", hex(v))


def _keccak_states():
    """zero, all ones, every single-bit state (pins each half-word's lane in the wave form's bit-interleaved layout), random"""
    sts = [bytes(200), b"\xff" * 200]
    for bit in range(1600):
        s = bytearray(200)
        s[bit // 8] = 1 << (bit % 8)
        sts.append(bytes(s))
    sts += [hashlib.shake_256(b"kf%d" % i).digest(200) for i in range(64)]
    return sts


def _keccak_ref(st):
    s = bytearray(st)
    merlin.keccak_f1600(s)
    return bytes(s)


def test_keccak_f_one_lane_and_wavefront(dev):
    sts = _keccak_states()
    want = [_keccak_ref(s) for s in sts]
    n = len(sts)
    buf = ctypes.create_string_buffer(b"".join(sts), 200 * n)
    assert dev.lib.dc_keccak_f(n, buf) == 0
    for i in range(n):
        assert buf.raw[200 * i:200 * i + 200] == want[i], (dev.variant, "one lane", i)
    out = ctypes.create_string_buffer(200 * 64 * n)
    assert dev.lib.dc_keccak_f_wave(n, b"".join(sts), out) == 0
    raw = out.raw
    for i in range(n):
        base = 200 * 64 * i
        for lane in range(64):  # every lane of the wavefront leaves with the permuted state
            assert raw[base + 200 * lane:base + 200 * lane + 200] == want[i], (dev.variant, "wave", i, lane)


def test_rng_bulk_draws_equal_generic_path(dev):
    """TranscriptRng on the device: merlin_rng_fill64_bulk == byte-wise STROBE fills == the oracle's TranscriptRng"""
    for count, wlen in [(1, 32), (7, 32), (50, 0), (300, 100)]:
        n = 4
        per = 64 * (count + 2)
        ws = [hashlib.shake_256(b"w%d.%d" % (count, i)).digest(wlen) if wlen else b"" for i in range(n)]
        ents = [bytes([0x21 + i]) * 32 for i in range(n)]
        g, b, ok = ctypes.create_string_buffer(per * n), ctypes.create_string_buffer(per * n), (ctypes.c_int32 * n)()
        assert dev.lib.dc_merlin_rng_bulk(n, b"".join(ws), wlen, b"".join(ents), count, g, b, ok) == 0
        assert list(ok) == [1] * n
        assert g.raw == b.raw, (dev.variant, count)
        for i in range(n):
            t = merlin.Transcript(b"BlindBidProofGadget")
            r = t.build_rng([(b"v_blinding", ws[i])], ents[i])
            assert b"".join(r.fill_bytes(64) for _ in range(count + 2)) == g.raw[per * i:per * (i + 1)], (dev.variant, count, i)
