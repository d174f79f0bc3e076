"""Value batteries for the arithmetic tests of both tiers: tests/test_host_arith.py (the product headers compiled for the host by
tests/host_check.cpp) and tests/test_gpu_device_arith.py (the same headers compiled for gfx950 by tests/device_check.hip).  Both
tiers read the same lists from here, so an edge added once is checked on the CPU and on the device.

Limb vectors are ten signed limbs in radix 2^25.5 (csrc/field.h): limb i weighs 2^OFF[i] and holds BITS[i] bits when carried.
Every limb generator stays inside the bound its consumer documents and checks that it does."""
import hashlib
import random

from oracle.ref_py import ristretto as rs

P, L = rs.P, rs.L
M255 = (1 << 255) - 1  # the loader ignores bit 255, like dalek's FieldElement::from_bytes

# ---- field: byte-level battery (fe_fromwords inputs) ---------------------------------------------------------------------------
EDGE = [0, 1, 2, 19, 38, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, 2**256 - 1, 2**256 - 38, 2**256 - 39,
        2**256 - 37, 2**32 - 1, 2**224, (2**256 - 1) ^ (2**128)]
LIMB_EDGES = [(1 << 26) - 1, ((1 << 25) - 1) << 26, M255, M255 - 18, M255 - 19, M255 - 20, (1 << 255) - (1 << 230),
              sum(1 << o for o in (25, 50, 76, 101, 127, 152, 178, 203, 229, 254))]


def field_cases():
    """(vals, pairs, inv_vals): single operands, (a, b) pairs for the binary ops, operands of inversion / pow22523."""
    rnd = random.Random(1)
    vals = EDGE + LIMB_EDGES + [rnd.getrandbits(256) for _ in range(200)]
    pairs = []
    for a0 in vals:
        for b0 in rnd.sample(vals, 5) + EDGE[:4] + [2**256 - 1, 2**256 - 38] + LIMB_EDGES[:3]:
            pairs.append((a0, b0))
    return vals, pairs, vals[:40]


def field_growth(a, b):
    """the field element hc_fe_op / dc_fe_op op 10 (and host op 12) return: three-term sums into a multiply, twice"""
    m1, m2, m3 = a * b % P, b * b % P, b * a * a % P
    r = (2 * m1 + m2) * (m3 - m2 - m1) % P
    return pow(r + m1 - m3, 2, P)


# ---- field: limb-level battery (dc_fe_limbs / hc_fe_limbs inputs) ---------------------------------------------------------------
BITS = [26, 25] * 5
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
# field.h:10-12: multiply / square accept |f_even| <= 1.65 * 2^26, |f_odd| <= 1.65 * 2^25 (1.65 = 33 / 20) ...
MUL_BOUND = [(33 << 24) // 5 if b == 26 else (33 << 23) // 5 for b in BITS]
# ... and return carried limbs: |h_even| <= 2^25, |h_odd| <= 2^24, plus the one small wrap carry into limb 1 (field.h fe_chain_wrap;
# 19 * c9 >> 26 < 2^17) and, where the carry pass visits column 4 twice (fe_carry64 / fe_carry64_prebiased), a carry into limb 5
CARRIED = [1 << (b - 1) for b in BITS]
CARRY_SLACK_CHAIN = {1: 1 << 17}
CARRY_SLACK_TWO_PASS = {1: 1 << 17, 5: 1 << 12}
# field.h:463: fe_towords (and so iszero / isneg / eq) accepts limbs up to 1.1 * 2^26 / 1.1 * 2^25
TOWORDS_BOUND = [(11 << 26) // 10 if b == 26 else (11 << 25) // 10 for b in BITS]


def limb_value(v):
    return sum(x << o for x, o in zip(v, OFF))


def within(v, bound, slack=None):
    slack = slack or {}
    return all(abs(x) <= bound[i] + slack.get(i, 0) for i, x in enumerate(v))


def _signed_radix(t, bound):
    """t as ten limbs (balanced digits, the top limb takes the rest), congruent to t mod p and inside `bound`"""
    v = []
    for b in BITS[:9]:
        d = t & ((1 << b) - 1)
        if d >= 1 << (b - 1):
            d -= 1 << b
        v.append(d)
        t = (t - d) >> b
    v.append(t)
    while abs(v[9]) > bound[9]:  # fold the excess of the top limb back through 2^255 = 19 (the value changes by a multiple of p)
        m = v[9] >> 25 if v[9] > 0 else -((-v[9]) >> 25)
        v[9] -= m << 25
        v[0] += 19 * m
    assert within(v, bound), v
    return v


def _move(v, i, m):
    """m * 2^BITS[i] from limb i + 1 into limb i: the same integer"""
    w = list(v)
    w[i] += m << BITS[i]
    w[i + 1] -= m
    return w


def _move_range(v, i, bound):
    s = 1 << BITS[i]
    lo = max(-((bound[i] + v[i]) // s), v[i + 1] - bound[i + 1])
    hi = min((bound[i] - v[i]) // s, v[i + 1] + bound[i + 1])
    return lo, hi


def near_multiples(bound, rnd, reshapes=6):
    """limb vectors whose value is k p + d, k in -2..2, d in {0, +-1, +-19} (so congruent to 0, +-1, +-19 mod p): the signed-radix
    form, then weight moved between neighbouring limbs -- at random and pushed all the way to the bound"""
    out = []
    for k in range(-2, 3):
        for d in (0, 1, -1, 19, -19):
            base = _signed_radix(k * P + d, bound)
            out.append(base)
            for r in range(reshapes):
                v = base
                order = list(range(9))
                rnd.shuffle(order)
                for i in order:
                    lo, hi = _move_range(v, i, bound)
                    if lo > hi:
                        continue
                    m = (hi if r % 3 == 1 else lo) if r % 3 else rnd.randint(lo, hi)
                    v = _move(v, i, m)
                assert within(v, bound) and (limb_value(v) - limb_value(base)) == 0, v
                out.append(v)
    return out


def limb_extremes(bound, rnd, n_random=400):
    """every limb at +max / -max, alternating signs, one limb at +-max with the rest zero, uniform random limbs in the bound"""
    out = [list(bound), [-x for x in bound],
           [x if i % 2 == 0 else -x for i, x in enumerate(bound)], [-x if i % 2 == 0 else x for i, x in enumerate(bound)],
           [x if (i // 2) % 2 == 0 else -x for i, x in enumerate(bound)]]
    for i in range(10):
        for s in (1, -1):
            v = [0] * 10
            v[i] = s * bound[i]
            out.append(v)
    out += [[rnd.randint(-b, b) for b in bound] for _ in range(n_random)]
    return out


def carried_sums(rnd, n=300):
    """three-term sums and differences of carried values, the largest operands point.h feeds a multiply (field.h:12)"""
    def carried():
        v = [rnd.randint(-c, c) for c in CARRIED]
        v[1] += rnd.randint(-(1 << 17), 1 << 17)
        return v
    ext = [c for c in CARRIED]
    ext[1] += 1 << 17
    out = [[3 * x for x in ext], [-3 * x for x in ext], [x if i % 2 else -x for i, x in enumerate(ext)]]
    for _ in range(n):
        a, b, c = carried(), carried(), carried()
        sa, sb = rnd.choice((1, -1)), rnd.choice((1, -1))
        out.append([x + sa * y + sb * z for x, y, z in zip(a, b, c)])
    for v in out:
        assert within(v, MUL_BOUND), v
    return out


def mul_operands():
    """operands for multiply / square / sq2 at the documented input bound"""
    rnd = random.Random(11)
    vs = limb_extremes(MUL_BOUND, rnd) + carried_sums(rnd) + near_multiples(MUL_BOUND, rnd)
    for v in vs:
        assert within(v, MUL_BOUND), v
    return vs


def mul_pairs(vs):
    rnd = random.Random(12)
    pairs = [(a, b) for a in vs[:25] for b in vs[:25]]  # every extreme against every extreme
    pairs += [(a, rnd.choice(vs)) for a in vs for _ in range(3)]
    return pairs


def towords_operands():
    """operands for fe_towords / iszero / isneg / eq, near multiples of p inside the 1.1 * 2^26 / 2^25 bound"""
    rnd = random.Random(13)
    vs = limb_extremes(TOWORDS_BOUND, rnd, n_random=200) + near_multiples(TOWORDS_BOUND, rnd, reshapes=12)
    for v in vs:
        assert within(v, TOWORDS_BOUND), v
    return vs


def eq_pairs(xs):
    """(a, b) with a - b = x limb for limb (x a towords operand), b carried: fe_eq(a, b) must be (x == 0 mod p)"""
    rnd = random.Random(14)
    out = []
    for x in xs:
        b = [rnd.randint(-c, c) for c in CARRIED]
        out.append(([u + w for u, w in zip(x, b)], b))
    return out


def carried_pairs(n=600):
    """(a, b) carried (with the limb-1 slack): the operands of op 4, mul(a + b, a - b), whose factors then reach 2^26 / 2^25"""
    rnd = random.Random(15)
    ext = list(CARRIED)
    vs = [ext, [-x for x in ext], [x if i % 2 else -x for i, x in enumerate(ext)]]
    vs += [[rnd.randint(-c, c) for c in CARRIED] for _ in range(n)]
    for v in vs:
        assert within(v, CARRIED, CARRY_SLACK_CHAIN), v
    return [(a, b) for a in vs[:3] for b in vs[:3]] + [(vs[i], vs[-1 - i]) for i in range(len(vs))]


# ---- scalars -----------------------------------------------------------------------------------------------------------------
def scalar_cases():
    """dict: vals, pairs (binary ops), fermat (Fermat-ladder inversion), inv (safegcd inversion), wide (64-byte reductions),
    bits (from_bits and is_canonical)"""
    rnd = random.Random(2)
    svals = [0, 1, 2, L - 1, L - 2, L // 2, 2**252, 2**252 - 1] + [rnd.randrange(L) for _ in range(200)]
    pairs = []
    for a in svals:
        for b in rnd.sample(svals, 5) + [0, 1, L - 1]:
            pairs.append((a, b))
    fermat = [a for a in svals[:30] if a]
    # safegcd inversion: edge values, powers of two and their neighbours, small values, dense random sample; 0 -> 0
    inv = svals + [3, 4, 5, 2**30 - 1, 2**30, 2**30 + 1, 2**60, 2**90 - 1, L - 3, (L + 1) // 2, (L - 1) // 2, 2**251, 2**252 + 1]
    inv += [2**k for k in range(0, 252, 7)] + [L - 2**k for k in range(1, 252, 11)] + [rnd.randrange(L) for _ in range(3000)]
    inv += [rnd.getrandbits(rnd.randrange(1, 252)) for _ in range(500)]
    wide = [0, 2**512 - 1, 2**256 - 1, 2**256, L, L << 256] + [rnd.getrandbits(512) for _ in range(200)]
    bits = [2**256 - 1, 2**255, 2**255 - 1, L, L + 1, 15 * L + 7] + [rnd.getrandbits(256) for _ in range(100)]
    return {"vals": svals, "pairs": pairs, "fermat": fermat, "inv": inv, "wide": wide, "bits": bits}


def naf_values():
    """scalars for the MSM kernels' NAF recoding (values < 2^253)"""
    rnd = random.Random(7)
    vals = [0, 1, 2, 3, L - 1, L - 2, 2**252, 2**253 - 1, 2**252 - 1, (2**253 - 1) // 3, 0xfff, 0x800, 0x7ff, 2**200 - 1,
            int("10" * 126, 2), int("01" * 126, 2), (1 << 253) - (1 << 241), sum(1 << (13 * i) for i in range(19))]
    vals += [rnd.getrandbits(253) for _ in range(3000)] + [rnd.getrandbits(rnd.randrange(1, 253)) for _ in range(500)]
    return vals


NAF_MAX_DIGITS = {12: 22, 9: 29}


def check_naf(width, v, pos, dig):
    """value, oddness, magnitude, spacing, position and count bounds of one recoding"""
    n = len(pos)
    assert n <= NAF_MAX_DIGITS[width], (width, hex(v), n)
    assert sum(d << p for p, d in zip(pos, dig)) == v, (width, hex(v))
    for i in range(n):
        assert dig[i] & 1 and abs(dig[i]) < (1 << (width - 1)) and 0 <= pos[i] <= 253, (width, hex(v), i)
        assert i == 0 or pos[i] >= pos[i - 1] + width, (width, hex(v), i)


# ---- ristretto -----------------------------------------------------------------------------------------------------------------
# RFC 9496 appendix A.3: encodings that must be rejected
BAD_ENCODINGS = [
    "00ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff", "f3ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f", "0100000000000000000000000000000000000000000000000000000000000000",
    "01ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f", "ed57ffd8c914fb201471d1c3d245ce3c746fcbe63a3679d51b6a516ebebe0e20",
    "c34c4e1826e5d403b78e246e88aa051c36ccf0aafebffe137d148a2bf9104562", "c940e5a4404157cfb1628b108db051a8d439e1a421394ec4ebccb9ec92a8ac78",
    "47cfc5497c53dc8e61c91d17fd626ffb1c49e2bca94eed052281b510b1117a24", "f1c6165d33367351b0da8f6e4511010c68174a03b6581212c71c0e1d026c3c72",
    "87260f7a2f12495118360f02c26a470f450dadf34a413d21042b43b9d93e1309", "26948d35ca62e643e26a83177332e6b6afeb9d08e4268b650f1f5bbd8d81d371",
    "4eac077a713c57b4f4397629a4145982c661f48044dd3f96427d40b147d9742f", "de6a7b00deadc788eb6b6c8d20c0ae96c2f2019078fa604fee5b87d6e989ad7b",
    "bcab477be20861e01e4a0e295284146a510150d9817763caf1a6f4b422d67042", "2a292df7e32cababbd9de088d1d1abec9fc0440f637ed2fba145094dc14bea08",
    "f4a9e534fc0d216c44b218fa0c42d99635a0127ee2e53c712f70609649fdff22", "8268436f8c4126196cf64b3c7ddbda90746a378625f9813dd9b8457077256731",
    "2810e5cbc2cc4d4eece54f61c6f69758e289aa7ab440b3cbeaa21995c2f4232b", "3eb858e78f5a7254d8c9731174a94f76755fd3941c0ac93735c07ba14579630e",
    "a45fdc55c76448c049a1ab33f17023edfb2be3581e9c7aade8a6125215e04220", "d483fe813c6ba647ebbfd3ec41adca1c6130c2beeee9d9bf065c8d151c5f396e",
    "8a2e1d30050198c65a54483123960ccc38aef6848e1ec8f5f780e8523769ba32", "32888462f8b486c68ad7dd9610be5192bbeaf3b443951ac1a8118419d9fa097b",
    "227142501b9d4355ccba290404bde41575b037693cef1f438c47f8fbf35d1165", "5c37cc491da847cfeb9281d407efc41e15144c876e0170b499a96a22ed31e01e",
    "445425117cb8c90edcbc7c1cc0e74f747f2c1efa5630a967c64f287792a48a4b", "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f"]


def point_cases():
    """(pts, partners, scalars): the identity, the basepoint and 16 random multiples; partners[i] indexes the points point i is
    combined with; four scalars for the double-and-add check"""
    rnd = random.Random(3)
    pts = [rs.IDENT, rs.BASEPOINT] + [rs.pt_mul(rnd.randrange(L), rs.BASEPOINT) for _ in range(16)]
    partners = [[0, 1, i, (i * 7 + 3) % len(pts)] for i in range(len(pts))]
    return pts, partners, [rnd.randrange(L) for _ in range(4)]


def uniform_inputs(n=40):
    return [hashlib.sha512(b"u%d" % i).digest() for i in range(n)]


# ---- limb-level checks, shared by both tiers ---------------------------------------------------------------------------------
LIMB_OPS = {"mul": 0, "sq": 1, "sq2": 2, "mul_small": 3, "addsub_mul": 4, "towords": 5, "iszero": 6, "isneg": 7, "eq": 8}
SMALL_FACTORS = [0, 1, 2, 19, 121666, (1 << 25) + 1, (1 << 26) - 1]


def check_fe_limbs(run, chain):
    """run(op, pairs) -> [(out limbs, out bytes)] for a list of (a limbs, b limbs) pairs (LIMB_OPS codes).  chain: True where fe_mul /
    fe_sq thread their carries through the column sums (the device default), False where a separate carry pass visits column 4
    twice (host C path, -DBBP_FE_NO_CHAIN).  Returns the number of evaluations per op."""
    slack = CARRY_SLACK_CHAIN if chain else CARRY_SLACK_TWO_PASS
    counts = {}

    def call(name, pairs):
        res = run(LIMB_OPS[name], pairs)
        assert len(res) == len(pairs)
        counts[name] = len(pairs)
        return res

    def carried_result(h, o, want, bound_slack, ctx):
        assert limb_value(h) % P == want, ctx
        assert int.from_bytes(o, "little") == want, ctx
        assert within(h, CARRIED, bound_slack), (ctx, h)

    ops = mul_operands()
    zero = [0] * 10
    pairs = mul_pairs(ops)
    for (a, b), (h, o) in zip(pairs, call("mul", pairs)):
        carried_result(h, o, limb_value(a) * limb_value(b) % P, slack, ("mul", a, b))
    singles = [(a, zero) for a in ops]
    for (a, _), (h, o) in zip(singles, call("sq", singles)):
        carried_result(h, o, limb_value(a) ** 2 % P, slack, ("sq", a))
    for (a, _), (h, o) in zip(singles, call("sq2", singles)):  # fe_sq, then fe_carry64 of the doubled limbs
        carried_result(h, o, 2 * limb_value(a) ** 2 % P, CARRY_SLACK_TWO_PASS, ("sq2", a))
    small = [(c, [s] + [0] * 9) for c in carried_sums(random.Random(16), n=100) for s in SMALL_FACTORS]
    for (a, b), (h, o) in zip(small, call("mul_small", small)):
        want = limb_value(a) * b[0] % P
        assert limb_value(h) % P == want and int.from_bytes(o, "little") == want, ("mul_small", a, b[0])
    cp = carried_pairs()
    for (a, b), (h, o) in zip(cp, call("addsub_mul", cp)):
        va, vb = limb_value(a), limb_value(b)
        carried_result(h, o, (va + vb) * (va - vb) % P, slack, ("addsub_mul", a, b))
    tw = [(x, zero) for x in towords_operands()]
    for (a, _), (h, o) in zip(tw, call("towords", tw)):
        assert int.from_bytes(o, "little") == limb_value(a) % P, ("towords", a)
    for (a, _), (h, o) in zip(tw, call("iszero", tw)):
        assert h[0] == (1 if limb_value(a) % P == 0 else 0) and int.from_bytes(o, "little") == limb_value(a) % P, ("iszero", a)
    for (a, _), (h, o) in zip(tw, call("isneg", tw)):
        assert h[0] == (limb_value(a) % P) & 1, ("isneg", a)
    eqp = eq_pairs([x for x, _ in tw])
    for (a, b), (h, o) in zip(eqp, call("eq", eqp)):
        assert h[0] == (1 if (limb_value(a) - limb_value(b)) % P == 0 else 0), ("eq", a, b)
    assert sum(1 for x, _ in tw if limb_value(x) % P == 0) >= 50  # the predicates do see their true case
    return counts
