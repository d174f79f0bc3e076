// The radix-16 scalar multiplications of the engine, for gfx950: the Pedersen comb (prover.hip k_commit*; table: setup.hip
// k_build_comb), the IPA tail tables and the carry-mask walk over them (prover.hip k_tail_tables / k_tail_lr) and the three
// data-dependent steps of the verifier's Straus sums (verifier.inc / verifier_mixed.inc k_varbase, k_varprep / k_varsum and their
// mixed-N twins).  k_commit* and k_tail_lr call the functions here.  k_build_comb, k_tail_tables and the Straus kernels keep their
// own copies of comb_build_column, tail_table_build and the straus_* steps (called from there, the kernels' instruction order
// changed): for those the functions below state the same code for the tests, and a change to either side belongs in both.  The
// copies have tests of their own: tests/test_gpu_varbase_kernels.py runs the shipped Straus kernels (bbp_debug_varbase) over the
// battery of tests/varbase_cases.py, tests/test_gpu_tables.py audits the comb and the tail table the shipped builders made at start-up.
//
// Everything here walks the signed radix-16 digits of a CANONICAL scalar (< l): the 8-entry tables are indexed by digit magnitude
// 1..8 and no caller feeds anything else.  Two recodings:
//   carry form   d = nibble_j + carry_j, carry_(j+1) = d > 8, digit d - 16 carry_(j+1): digits in [-7, 8]             (comb, tail)
//   offset form  sp = s + 0x88..8 over 256 bits, digit nibble_j(sp) - 8: digits in [-8, 7]                              (Straus)
// Functions without a wave shuffle are BBP_HD: tests/host_check.cpp compiles them for the CPU (tests/test_scalarmul_host.py),
// tests/device_check.hip for gfx950 (tests/test_gpu_scalarmul.py); tests/scalarmul_cases.py holds the scalars that reach their edges.
#pragma once
#include "point.h"
#include "scalar.h"

namespace bbp {

// ---------------------------------------------------------------------------------------------------------------
// K2: Pedersen commitments through the radix-16 comb (64 signed digits per scalar, 8 cached multiples each)
// ---------------------------------------------------------------------------------------------------------------
// one comb entry from HBM into registers (the host form reads the same 24 words one by one)
#if defined(__HIPCC__)
#define BBP_COMB_LOAD(n, entry)                                                                  \
    do {                                                                                         \
        const uint4* q_ = reinterpret_cast<const uint4*>(entry);                                 \
        uint4 q0 = q_[0], q1 = q_[1], q2 = q_[2], q3 = q_[3], q4 = q_[4], q5 = q_[5];            \
        (n).ypx = BBP_FE_LIT(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w);                    \
        (n).ymx = BBP_FE_LIT(q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w);                    \
        (n).xy2d = BBP_FE_LIT(q4.x, q4.y, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w);                   \
    } while (0)
#else
#define BBP_COMB_LOAD(n, entry)                     \
    do {                                            \
        const u32* w_ = (entry)->w;                 \
        (n).ypx = fe_fromwords(w_);                 \
        (n).ymx = fe_fromwords(w_ + 8);             \
        (n).xy2d = fe_fromwords(w_ + 16);           \
    } while (0)
#endif

// column j of one base's comb: out8[m - 1] = m * 16^j * p, m = 1..8
BBP_HD void comb_build_column(ge p, u32 j, niels_packed* out8) {
    for (u32 k = 0; k < 4 * j; k++) p = ge_dbl(p);
    ge m = p;
    for (int k = 0; k < 8; k++) {
        out8[k] = niels_pack(ge_to_niels(m, fe_invert(m.Z)));
        m = ge_add(m, p);
    }
}

BBP_HD ge comb_mul_add(ge acc, const niels_packed* __restrict__ comb_base, const sc& s) {
    u32 carry = 0;
    for (int j = 0; j < 64; j++) {
        u32 d = ((s.v[j >> 3] >> (4 * (j & 7))) & 15u) + carry;
        carry = d > 8u;
        u32 mag = carry ? 16u - d : d;
        if (mag) {
            ge_niels n;
            BBP_COMB_LOAD(n, comb_base + (size_t)j * 8 + (mag - 1));
            if (carry) {
                fe t = n.ypx;
                n.ypx = n.ymx;
                n.ymx = t;
                n.xy2d = fe_neg(n.xy2d);
            }
            acc = ge_madd(acc, n);
        }
    }
    return acc;  // canonical scalars are < 2^253: the top digit never carries out
}

// Small launches: a commitment on COMMIT_L lanes.  One lane walks 2 x 64 comb digits (~120 dependent mixed additions: 380 us for
// ONE proof's twelve commitments, and again for its five T commitments); here lane q of a group takes the digit positions
// j = q (mod COMMIT_L) of both scalars (every lane recodes the whole scalar -- the carries -- which is cheap) and three shuffle
// steps add the partial sums.  The sum is the same group element, its encoding the same bytes.
constexpr int COMMIT_L = 8;
BBP_HD ge comb_mul_add_part(ge acc, const niels_packed* __restrict__ comb_base, const sc& s, u32 q) {
    // the signed radix-16 digits of the whole scalar first (the carries are a chain): magnitudes as nibbles, signs as a bit mask;
    // then the lane's own eight positions q, q + 8, ... -- every lane of the wavefront adds at the same time
    u32 mags[8];
    u64 negs = 0;
    u32 carry = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        u32 mw = 0;
#pragma unroll
        for (int n = 0; n < 8; n++) {
            const u32 d = ((s.v[w] >> (4 * n)) & 15u) + carry;
            carry = d > 8u;
            mw |= (carry ? 16u - d : d) << (4 * n);
            negs |= (u64)carry << (8 * w + n);
        }
        mags[w] = mw;
    }
#pragma unroll 1
    for (int i = 0; i < 64 / COMMIT_L; i++) {
        u32 mw = mags[0];
#pragma unroll
        for (int w = 1; w < 8; w++) mw = i == w ? mags[w] : mw;
        const u32 j = q + (u32)COMMIT_L * (u32)i, mag = (mw >> (4 * q)) & 15u, neg = (u32)(negs >> j) & 1u;
        if (mag) {
            ge_niels n;
            BBP_COMB_LOAD(n, comb_base + (size_t)j * 8 + (mag - 1));
            if (neg) {
                fe t = n.ypx;
                n.ypx = n.ymx;
                n.ymx = t;
                n.xy2d = fe_neg(n.xy2d);
            }
            acc = ge_madd(acc, n);
        }
    }
    return acc;
}
#if defined(__HIPCC__)
__device__ __forceinline__ ge commit_group_sum(ge acc) {  // lane 0 of every COMMIT_L-lane group ends up with the group's sum
#pragma unroll 1
    for (int d = COMMIT_L / 2; d >= 1; d >>= 1) {
        ge other;
        const u32* w = reinterpret_cast<const u32*>(&acc);
        u32* o = reinterpret_cast<u32*>(&other);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(ge) / 4); i++) o[i] = (u32)__shfl_down((int)w[i], d, 64);
        acc = ge_add(acc, other);  // (lanes whose partner lies in the next group add something nobody reads)
    }
    return acc;
}
#endif

// ---------------------------------------------------------------------------------------------------------------
// IPA tail on explicit folded generators (rounds FOLD_ROUND..11, vectors of length <= 32)
// ---------------------------------------------------------------------------------------------------------------
// Tail tables: for a point P the multiples m * 2^(w k) * P, m = 1..8, k = 0..TAIL_PIECES-1, w = 256 / TAIL_PIECES.  A scalar
// multiplication over such a table is (w - 4) doublings + 64 additions (signed radix-16 digits, the pieces share the doublings)
// instead of 252 + 64 + 7, and the tables of the 64 materialised generators are built once and used by all five tail rounds.
// Four 64-bit pieces: 60 doublings per multiplication, 192 to build a table; eight 32-bit pieces: 28 and 224 (+ 28 additions): the
// tail launches are chain-bound, a table serves five rounds.
#ifndef BBP_TAIL_PIECES
#define BBP_TAIL_PIECES 8
#endif
constexpr int TAIL_PIECES = BBP_TAIL_PIECES, TAIL_PIECE_BITS = 256 / TAIL_PIECES, TAIL_DIGITS = TAIL_PIECE_BITS / 4;
constexpr int TAIL_TAB = 8 * TAIL_PIECES;
static_assert(TAIL_PIECES == 4 || TAIL_PIECES == 8 || TAIL_PIECES == 16, "tail table geometry");

// the table of one point: T[8 k + m - 1] = m * 2^(w k) * P
BBP_HD void tail_table_build(ge P, ge* T) {
#pragma unroll 1
    for (int k = 0; k < TAIL_PIECES; k++) {
        ge cur = P;
        T[8 * k] = P;
#pragma unroll 1
        for (int i = 1; i < 8; i++) {
            cur = ge_add(cur, P);
            T[8 * k + i] = cur;
        }
        if (k < TAIL_PIECES - 1) {
#pragma unroll 1
            for (int i = 0; i < TAIL_PIECE_BITS; i++) P = ge_dbl(P);
        }
    }
}

// pieces k_lo <= k < k_hi only: the partial product sum_k 2^(w k) * (piece k of s) * P
BBP_HD ge ge_scalarmul_pieces(const sc& s, const ge* __restrict__ T, int k_lo = 0, int k_hi = TAIL_PIECES) {
    // carry mask of the signed radix-16 recoding: bit j = carry INTO digit j (a canonical scalar never carries out of digit 63)
    u64 cm = 0;
    u32 c = 0;
    for (int j = 0; j < 64; j++) {
        u32 v = ((s.v[j >> 3] >> (4 * (j & 7))) & 15u) + c;
        c = v > 8u;
        if (j < 63) cm |= (u64)c << (j + 1);
    }
    ge acc = ge_identity();
    for (int r = TAIL_DIGITS - 1; r >= 0; r--) {
        if (r != TAIL_DIGITS - 1) {
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
        }
        for (int k = k_lo; k < k_hi; k++) {
            const int j = TAIL_DIGITS * k + r;
            const int d = (int)((s.v[j >> 3] >> (4 * (j & 7))) & 15u) + (int)((cm >> j) & 1u) - 16 * (int)((j < 63) ? ((cm >> (j + 1)) & 1u) : 0u);
            if (d != 0) {
                ge q = T[8 * k + (d > 0 ? d : -d) - 1];
                if (d < 0) q = ge_neg(q);
                acc = ge_add(acc, q);
            }
        }
    }
    return acc;
}

// s1 * P1 + s2 * P2 over tail tables T1, T2 with ONE doubling chain (two terms per lane: measured out of k_tail_lr)
BBP_HD ge ge_scalarmul_pieces_pair(const sc& s1, const ge* __restrict__ T1, const sc& s2, const ge* __restrict__ T2) {
    u64 cm1 = 0, cm2 = 0;
    u32 c1 = 0, c2 = 0;
    for (int j = 0; j < 64; j++) {
        const u32 v1 = ((s1.v[j >> 3] >> (4 * (j & 7))) & 15u) + c1, v2 = ((s2.v[j >> 3] >> (4 * (j & 7))) & 15u) + c2;
        c1 = v1 > 8u;
        c2 = v2 > 8u;
        if (j < 63) {
            cm1 |= (u64)c1 << (j + 1);
            cm2 |= (u64)c2 << (j + 1);
        }
    }
    ge acc = ge_identity();
    for (int r = TAIL_DIGITS - 1; r >= 0; r--) {
        if (r != TAIL_DIGITS - 1) {
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
        }
#pragma unroll 1
        for (int kk = 0; kk < 2 * TAIL_PIECES; kk++) {  // piece k of scalar 1, then piece k of scalar 2: one addition site
            const int k = kk >> 1;
            const bool second = kk & 1;
            const int j = TAIL_DIGITS * k + r;
            const u32 word = second ? s2.v[j >> 3] : s1.v[j >> 3];
            const u64 cm = second ? cm2 : cm1;
            const int d = (int)((word >> (4 * (j & 7))) & 15u) + (int)((cm >> j) & 1u) - 16 * (int)((j < 63) ? ((cm >> (j + 1)) & 1u) : 0u);
            if (d != 0) {
                ge q = (second ? T2 : T1)[8 * k + (d > 0 ? d : -d) - 1];
                if (d < 0) q = ge_neg(q);
                acc = ge_add(acc, q);
            }
        }
    }
    return acc;
}

// k_tail_lr puts one side of a proof (L or R) on TAIL_SIDE lanes: lane j walks G/H term j, and the B term sB * B has no lane of its
// own -- btab has the geometry of every other table, so the TAIL_PIECES x TAIL_DIGITS signed digits of sB are dealt to the side's
// lanes, TAIL_SHARE_DIGITS each: lane j takes piece j % TAIL_PIECES, digits r0 .. r0 + TAIL_SHARE_DIGITS - 1 with
// r0 = TAIL_SHARE_DIGITS * (j / TAIL_PIECES).  A lane adds its share into its own accumulator in the iteration that handles digit r
// (every lane's doubling chain passes through every r, so the weight 16^r * 2^(w k) comes out right); the side's sum is then
// sum_j s_j P_j + sB B.
constexpr int TAIL_SIDE = 32, TAIL_SHARE_DIGITS = TAIL_PIECES * TAIL_DIGITS / TAIL_SIDE;
static_assert(TAIL_SHARE_DIGITS >= 1 && TAIL_SHARE_DIGITS * TAIL_SIDE == TAIL_PIECES * TAIL_DIGITS && TAIL_DIGITS % TAIL_SHARE_DIGITS == 0 &&
                  (TAIL_DIGITS / TAIL_SHARE_DIGITS) * TAIL_PIECES == TAIL_SIDE,
              "the shares of the B term tile its digits: every (piece, digit) belongs to exactly one lane of the side");

// carry mask of the signed radix-16 recoding (carry form): bit j = carry INTO digit j (a canonical scalar never carries out of digit 63)
BBP_HD u64 tail_carry_mask(const sc& s) {
    u64 cm = 0;
    u32 c = 0;
    for (int j = 0; j < 64; j++) {
        u32 v = ((s.v[j >> 3] >> (4 * (j & 7))) & 15u) + c;
        c = v > 8u;
        if (j < 63) cm |= (u64)c << (j + 1);
    }
    return cm;
}
// digit j of s, in [-7, 8]
BBP_HD int tail_digit(const sc& s, u64 cm, int j) {
    u32 word = s.v[0];  // (selects, not an indexed read: the scalar stays in registers when j is not known at compile time)
#pragma unroll
    for (int w = 1; w < 8; w++) word = (j >> 3) == w ? s.v[w] : word;
    return (int)((word >> (4 * (j & 7))) & 15u) +(int)((cm >> j) & 1u) - 16 * (int)((j < 63) ? ((cm >> (j + 1)) & 1u) : 0u);
}

struct tail_share {
    int k, r0;                  // piece, first digit position within the piece
    int d[TAIL_SHARE_DIGITS];   // digits r0, r0 + 1, .. of piece k
};
BBP_HD tail_share tail_share_of(const sc& sB, u32 lane /* of the side, < TAIL_SIDE */) {
    const u64 cm = tail_carry_mask(sB);
    tail_share sh;
    sh.k = (int)(lane % TAIL_PIECES);
    sh.r0 = TAIL_SHARE_DIGITS * (int)(lane / TAIL_PIECES);
    for (int i = 0; i < TAIL_SHARE_DIGITS; i++) sh.d[i] = tail_digit(sB, cm, TAIL_DIGITS * sh.k + sh.r0 + i);
    return sh;
}

// s * P over P's table T, plus the share `sh` of the B term over B's table TB: ge_scalarmul_pieces with one more slot per digit
// position, taken by the lanes whose share holds that position.  ONE addition site for the table's pieces and the share.
BBP_HD ge ge_scalarmul_pieces_shared(const sc& s, const ge* __restrict__ T, const tail_share& sh, const ge* __restrict__ TB) {
    const u64 cm = tail_carry_mask(s);
    ge acc = ge_identity();
    for (int r = TAIL_DIGITS - 1; r >= 0; r--) {
        if (r != TAIL_DIGITS - 1) {
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
        }
        const int i = r - sh.r0;
        const bool mine = i >= 0 && i < TAIL_SHARE_DIGITS;
        int dB = 0;
        for (int q = 0; q < TAIL_SHARE_DIGITS; q++) dB = q == i ? sh.d[q] : dB;
#pragma unroll 1
        for (int kk = 0; kk < TAIL_PIECES + 1; kk++) {  // pieces 0 .. TAIL_PIECES - 1 of s, then the share's digit
            const bool own = kk < TAIL_PIECES;
            if (!own && !mine) break;
            const int k = own ? kk : sh.k;
            const int d = own ? tail_digit(s, cm, TAIL_DIGITS * k + r) : dB;
            if (d != 0) {
                ge q = (own ? T : TB)[8 * k + (d > 0 ? d : -d) - 1];
                if (d < 0) q = ge_neg(q);
                acc = ge_add(acc, q);
            }
        }
    }
    return acc;
}
#if defined(__HIPCC__)
__device__ __forceinline__ ge tail_side_sum(ge acc) {  // the first lane of each TAIL_SIDE-lane half of the wavefront ends up with the half's sum
#pragma unroll 1
    for (int d = TAIL_SIDE / 2; d >= 1; d >>= 1) {
        ge other;
        const u32* w = reinterpret_cast<const u32*>(&acc);
        u32* o = reinterpret_cast<u32*>(&other);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(ge) / 4); i++) o[i] = (u32)__shfl_down((int)w[i], d, TAIL_SIDE);
        acc = ge_add(acc, other);  // (lanes whose partner lies past the half add something nobody reads)
    }
    return acc;
}
#endif

// ---------------------------------------------------------------------------------------------------------------
// K9: the data-dependent steps of the verifier's Straus sums (each kernel keeps its own loops over points, digits and lanes)
// ---------------------------------------------------------------------------------------------------------------
// digit words of s: sp = s + 0x88..8 with the carries between words; digit j of s is nibble j of sp minus 8, in [-8, 7]
BBP_HD void straus_recode(u32* sp, const sc& s) {
    u64 cy = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        cy += (u64)s.v[i] + 0x88888888u;
        sp[i] = (u32)cy;
        cy >>= 32;
    }
}

// tab[m - 1] = m * P, m = 1..8
BBP_HD void straus_table(ge* tab, const ge& P) {
    tab[0] = P;
    ge cur = P;
    for (int i = 1; i < 8; i++) {
        cur = ge_add(cur, P);
        tab[i] = cur;
    }
}

// acc + (digit j of the point whose digit words are sp) * (the point whose table is tab)
template <class J>
BBP_HD ge straus_digit_step(ge acc, const ge* tab, const u32* sp, J j) {
    const int d = (int)((sp[j >> 3] >> (4 * (j & 7))) & 15u) - 8;
    if (d != 0) {
        ge e = tab[(d > 0 ? d : -d) - 1];
        if (d < 0) e = ge_neg(e);
        acc = ge_add(acc, e);
    }
    return acc;
}

}  // namespace bbp
