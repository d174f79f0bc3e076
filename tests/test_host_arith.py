"""not-gpu tier: the PRODUCT's limb arithmetic headers (dusk_blindbidproof_amd/csrc/{field,scalar,point,keccak}.h),
compiled for the host by tests/host_check.cpp, against the big-int oracle.  Catches arithmetic bugs without a GPU;
the shipped library never runs this code on the CPU.  The value batteries live in tests/arith_cases.py, shared with the
device tier (tests/test_gpu_device_arith.py)."""
import ctypes
import hashlib

import pytest

from oracle.ref_py import merlin, ristretto as rs
from tests import arith_cases as ac

P, L = rs.P, rs.L


def b32(x):
    return x.to_bytes(32, "little")


@pytest.fixture(scope="module")
def lib(built):
    return ctypes.CDLL(built.build_hostcheck())


def test_field_ops(lib):
    def fe_op(op, a, b=0):
        out = ctypes.create_string_buffer(32)
        lib.hc_fe_op(op, b32(a), b32(b), out)
        return int.from_bytes(out.raw, "little")
    M = ac.M255
    vals, pairs, inv_vals = ac.field_cases()
    for a0, b0 in pairs:
        a, b = a0 & M, b0 & M
        assert fe_op(0, a0, b0) == (a + b) % P
        assert fe_op(1, a0, b0) == (a - b) % P
        assert fe_op(2, a0, b0) == (a * b) % P
        assert fe_op(8, a0, b0) == (a * (b0 & 0x3ffffff)) % P
        assert fe_op(10, a0, b0) == ac.field_growth(a, b)
        # round 4: the device path threads the carries through the column sums (field.h fe_chain_step / fe_chain_wrap, seed 2^25 +
        # 2^50 on even columns); the same functions over plain-C column sums must give the same field element, limbs carried
        assert fe_op(11, a0, b0) == (a * b) % P
        assert fe_op(12, a0, b0) == ac.field_growth(a, b)
    for a0 in vals:
        a = a0 & M
        assert fe_op(3, a0) == a * a % P
        assert fe_op(9, a0) == 2 * a * a % P
        assert fe_op(5, a0) == a % P
        assert fe_op(6, a0) == (-a) % P
    for a0 in inv_vals:
        a = a0 & M
        assert fe_op(4, a0) == pow(a % P, P - 2, P)
        assert fe_op(7, a0) == pow(a % P, (P - 5) // 8, P)


def test_field_limbs_at_the_documented_bounds(lib):
    """field.h's contract on raw limbs (tests/arith_cases.py limb generators): multiply / square / sq2 at the input bound give the
    right value with carried limbs; towords / iszero / isneg / eq near multiples of p agree with x % p.  Host C path: the separate
    carry pass (fe_carry64_prebiased)."""
    out10, out32 = (ctypes.c_int32 * 10)(), ctypes.create_string_buffer(32)

    def run(op, pairs):
        res = []
        for a, b in pairs:
            lib.hc_fe_limbs(op, (ctypes.c_int32 * 10)(*a), (ctypes.c_int32 * 10)(*b), out10, out32)
            res.append((list(out10), out32.raw))
        return res
    counts = ac.check_fe_limbs(run, chain=False)
    assert min(counts.values()) >= 500, counts


def test_scalar_ops(lib):
    def sc_op(op, a, b=b32(0)):
        out = ctypes.create_string_buffer(32)
        lib.hc_sc_op(op, a, b, out)
        return int.from_bytes(out.raw, "little")
    cs = ac.scalar_cases()
    for a, b in cs["pairs"]:
        assert sc_op(0, b32(a), b32(b)) == (a + b) % L
        assert sc_op(1, b32(a), b32(b)) == (a - b) % L
        assert sc_op(2, b32(a), b32(b)) == (a * b) % L
    for a in cs["vals"]:
        assert sc_op(6, b32(a)) == (-a) % L
    for a in cs["fermat"]:
        assert sc_op(7, b32(a)) == pow(a, L - 2, L)   # Fermat ladder (kept as a cross-check)
    # safegcd inversion: edge values, powers of two and their neighbours, small values, dense random sample; 0 -> 0
    for a in cs["inv"]:
        assert sc_op(3, b32(a)) == (pow(a, L - 2, L) if a else 0), hex(a)
    for w in cs["wide"]:
        assert sc_op(4, w.to_bytes(64, "little")) == w % L
    for w in cs["bits"]:
        assert sc_op(5, b32(w)) == (w & (2**255 - 1)) % L
        assert lib.hc_sc_is_canonical(b32(w)) == (1 if w < L else 0)
    assert lib.hc_sc_is_canonical(b32(L - 1)) == 1


def test_naf_recoding(lib):
    """sc_for_each_naf_digit (the MSM kernels' scalar recoding): value, oddness, magnitude, spacing, position and count bounds"""
    vals = ac.naf_values()
    total = {12: 0, 9: 0}
    for width in (12, 9):
        pos = (ctypes.c_int32 * 64)()
        dig = (ctypes.c_int32 * 64)()
        for v in vals:
            n = lib.hc_sc_naf(width, b32(v), pos, dig)
            ac.check_naf(width, v, pos[:n], dig[:n])
            total[width] += n
    assert total[12] / len(vals) < 20.5 and total[9] / len(vals) < 26.5  # ~253/13 and ~253/10 digits on average


def test_point_ops_and_codec(lib):
    out = ctypes.create_string_buffer(32)
    lib.hc_basepoint(out)
    assert out.raw == rs.encode(rs.BASEPOINT)
    pts, partners, scalars = ac.point_cases()
    enc = [rs.encode(p) for p in pts]

    def ge_op(op, a, b=bytes(32)):
        o = ctypes.create_string_buffer(32)
        return o.raw if lib.hc_ge_op(op, a, b, o) else None
    for i, (p, e) in enumerate(zip(pts, enc)):
        assert ge_op(0, e) == e
        assert ge_op(1, e) == rs.encode(rs.pt_dbl(p))
        for j in partners[i]:
            q, f = pts[j], enc[j]
            assert ge_op(2, e, f) == rs.encode(rs.pt_add(p, q))
            assert ge_op(3, e, f) == rs.encode(rs.pt_add(p, rs.pt_neg(q)))
            assert ge_op(4, e, f) == rs.encode(rs.pt_add(p, q))
            assert ge_op(5, e, f) == rs.encode(rs.pt_add(p, rs.pt_neg(q)))
    for h in ac.BAD_ENCODINGS:
        b = bytes.fromhex(h)
        assert rs.decode(b) is None, h
        assert ge_op(0, b) is None, h
    for u in ac.uniform_inputs():
        lib.hc_from_uniform(u, out)
        assert out.raw == rs.encode(rs.from_uniform_bytes(u))
    for i, s in enumerate(scalars):
        lib.hc_scalarmult(b32(s), enc[3 + i], out)
        assert out.raw == rs.encode(rs.pt_mul(s, pts[3 + i]))


def test_rng_bulk_draws_equal_generic_path(lib):
    """The register-resident steady-state TranscriptRng draw (keccak.h merlin_rng_fill64_bulk) == byte-wise STROBE."""
    for count, wlen in [(1, 32), (7, 32), (50, 0), (300, 100)]:
        n = 64 * (count + 2)
        a, b = ctypes.create_string_buffer(n), ctypes.create_string_buffer(n)
        w = hashlib.shake_256(b"w%d" % count).digest(wlen) if wlen else b""
        assert lib.hc_merlin_rng_bulk(w, wlen, b"\x21" * 32, count, a, b) == 1
        assert a.raw == b.raw
        t = merlin.Transcript(b"BlindBidProofGadget")
        r = t.build_rng([(b"v_blinding", w)], b"\x21" * 32)
        assert b"".join(r.fill_bytes(64) for _ in range(count + 2)) == a.raw


def test_gate_assignments_interpreted_native_and_oracle_agree(lib):
    """csrc/witness.h on the host: a_L, a_R, a_O of one proof from (a) the compiled gadget program interpreted, (b) the gadget wiring
    written out (what the cooperative opening launches run), (c) the big-int oracle's Prover driven through the same gadgets
    (oracle/ref_py, src/gadgets.rs in call order).  All three must be the same canonical scalars, for several list lengths, toggle
    positions (including one outside the list: no bit set) and an input above the group order."""
    import ctypes, random
    from oracle.ref_py import blindbid as bb, r1cs
    L = r1cs.L

    class ValuesOnly(r1cs.Prover):
        def __init__(self, values):
            r1cs._CSBase.__init__(self)
            self.v, self.vb = [x % L for x in values], []
            self.aL, self.aR, self.aO = [], [], []

    rnd = random.Random(81)
    mimc = bb.mimc_constants(bb.MIMC_ROUNDS)
    mimc_raw = b"".join(int(c).to_bytes(32, "little") for c in mimc)
    lib.hc_witness_gates.restype = ctypes.c_int
    for n, toggle in ((1, 0), (2, 1), (8, 3), (8, 2 ** 32 + 3), (13, 12), (40, 0)):
        seven = [rnd.randrange(L) for _ in range(7)]
        seven[0] = L + 5  # d is reduced on the way in
        items = [rnd.getrandbits(256) for _ in range(n)]
        raw = b"".join(x.to_bytes(32, "little") for x in seven) + b"".join(x.to_bytes(32, "little") for x in items) + toggle.to_bytes(8, "little")
        cap = 2048
        a, b = ctypes.create_string_buffer(3 * cap * 32), ctypes.create_string_buffer(3 * cap * 32)
        n_mul = lib.hc_witness_gates(n, raw, mimc_raw, a, b, cap)
        assert n_mul == 4 * 4 * bb.MIMC_ROUNDS + 3 * n + 2
        assert a.raw[:3 * n_mul * 32] == b.raw[:3 * n_mul * 32]
        d, k, y, y_inv, q, z_img, seed = [x % L for x in seven]
        cs = ValuesOnly([d, k, y, y_inv] + [1 if i == toggle else 0 for i in range(n)])
        t_v = [(r1cs.COMMITTED, 4 + i) for i in range(n)]
        bb.proof_gadget(cs, r1cs.LC.of((r1cs.COMMITTED, 0)), r1cs.LC.of((r1cs.COMMITTED, 1)), r1cs.LC.of((r1cs.COMMITTED, 3)), r1cs.LC.of(q),
                        r1cs.LC.of(z_img), r1cs.LC.of(seed), mimc, t_v, [r1cs.LC.of((x & ((1 << 255) - 1)) % L) for x in items])  # Scalar::from_bits (bid.rs:27): bit 255 cleared
        assert cs.n_mul == n_mul
        want = b"".join(int(x).to_bytes(32, "little") for x in cs.aL + cs.aR + cs.aO)
        assert a.raw[:3 * n_mul * 32] == want, n


def test_bit_interleaved_words_rotate_as_the_wave_keccak_assumes(lib):
    """keccak_wave.h keeps every 64-bit state word as (even bits, odd bits): a 64-bit rotation must be a 32-bit rotation of each
    half, with the halves changing places for odd amounts -- the rule the lane shifts and the rho-pi gather addresses are built from.
    All 64 amounts on random and edge words."""
    import ctypes, random
    lib.hc_kw_interleave.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.hc_kw_interleave.restype = ctypes.c_int
    rnd = random.Random(50)
    words = [0, 1, 2, 1 << 63, (1 << 64) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x0123456789ABCDEF] + [rnd.getrandbits(64) for _ in range(200)]
    for x in words:
        for r in range(64):
            assert lib.hc_kw_interleave(x, r) == 1, (hex(x), r)


def test_wave_keccak_model_permutes_like_keccak_f(lib):
    """tests/host_check.cpp hc_kw_keccak_f: the one-wavefront Keccak of keccak_wave.h restated on arrays of 64 lanes with the
    PRODUCT's lane tables (layout, theta / rho shift amounts, gather addresses, per-round iota vectors).  It must be Keccak-f[1600]."""
    import ctypes
    for seed in (b"a", b"bb", b"ccc", b""):
        st = bytearray(hashlib.shake_256(b"kw" + seed).digest(200)) if seed else bytearray(200)
        want = bytearray(st)
        merlin.keccak_f1600(want)
        buf = ctypes.create_string_buffer(bytes(st), 200)
        lib.hc_kw_keccak_f(buf)
        assert buf.raw == bytes(want)


def test_rotl64_every_amount(lib):
    """keccak.h rotl64 on the host for n = 0..63 (a rotation by 0 is x itself)"""
    lib.hc_rotl64.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.hc_rotl64.restype = ctypes.c_uint64
    m = (1 << 64) - 1
    for x in [0, 1, 1 << 63, m, 0x0123456789ABCDEF, 0xFFFFFFFF00000000]:
        for r in range(64):
            assert lib.hc_rotl64(x, r) == (((x << r) | (x >> (64 - r))) & m if r else x), (hex(x), r)


def test_keccak_and_merlin(lib):
    st = bytearray(hashlib.shake_256(b"st").digest(200))
    st2 = bytearray(st)
    merlin.keccak_f1600(st2)
    buf = ctypes.create_string_buffer(bytes(st), 200)
    lib.hc_keccak_f(buf)
    assert buf.raw == bytes(st2)
    o = ctypes.create_string_buffer(32)
    lib.hc_merlin_kat(b"test protocol", 13, b"some label", 10, b"some data", 9, b"challenge", 9, o, 32)
    assert o.raw.hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"  # merlin's own test vector
    for mlen in [0, 1, 150, 166, 167, 400]:
        msg = hashlib.shake_256(b"m%d" % mlen).digest(mlen) if mlen else b""
        n = 200
        o = ctypes.create_string_buffer(n)
        lib.hc_merlin_kat(b"BlindBidProofGadget", 19, b"lbl", 3, msg, mlen, b"ch", 2, o, n)
        t = merlin.Transcript(b"BlindBidProofGadget")
        t.append_message(b"lbl", msg)
        assert t.challenge_bytes(b"ch", n) == o.raw
        o = ctypes.create_string_buffer(2 * n)
        lib.hc_merlin_rng(b"BlindBidProofGadget", 19, b"v_blinding", 10, msg, mlen, b"\x07" * 32, o, n)
        t = merlin.Transcript(b"BlindBidProofGadget")
        r = t.build_rng([(b"v_blinding", msg)], b"\x07" * 32)
        assert r.fill_bytes(n) + r.fill_bytes(n) == o.raw
