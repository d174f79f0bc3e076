// The per-proof batch buffer, stated once: the list of its arrays (BBP_BATCH_ARRAYS) and what is generated from it -- the fields of
// BatchDev, the carve of one reservation, the view of a slice, the per-proof strides the launches pass -- with the word offsets of the
// encoding and point blocks.  prover.hip and verifier.inc execute these values: no host code restates a stride, and the kernels name
// the same constants where they index an array by its proof
// (DESIGN.md "The batch buffer").  Plain arithmetic, no HIP calls: the CPU test tier compiles it too (tests/host_check.cpp); the
// helpers that kernels use are BBP_HD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "keccak.h"
#include "point.h"
#include "prove_io.h"
#include "prove_plan.h"
#include "scalar.h"

namespace bbp {

// ---- the inner-product argument's sizes (the circuit pads to IPA_N multipliers for every N) -----------------------------------------
constexpr u32 IPA_N = 2048;               // generators per side = length of the IPA vectors
constexpr u32 IPA_HALF = IPA_N / 2;       // G terms (and H terms) of a round's L or R
constexpr u32 IPA_TERMS = IPA_N + 1;      // terms of a round's L or R with the c w B term; powers y^0 .. y^2048
constexpr u32 IPA_ROUNDS = 11;            // log2(IPA_N)
constexpr int FOLD_CLS = (int)(IPA_N >> (FOLD_ROUND - 1));  // 32 folded generators per side (context.h "IPA tail")

// slots of the per-proof `misc` scalar block
enum MiscSlot : int {
    MS_Y = 0, MS_Z, MS_U, MS_X, MS_W, MS_YINV, MS_T1, MS_T2, MS_T3, MS_T4, MS_T5, MS_T6, MS_TB1, MS_TB2, MS_TB3, MS_TB4, MS_TB5,
    MS_TB6, MS_TX, MS_TXB, MS_EBL, MS_UJ, MS_UJI, MS_A0, MS_B0, MS_R, MS_ALLINV, MS_WC, MS_DELTA, MS_RHO /* aggregated verification: the proof's random weight */, MS_COUNT = 32
};

// What the layout needs of the circuit; a mixed verify front end: the largest of each over the call's N (the per-row strides).
struct BatchDims {
    u32 m = 0, n_mul = 0, n_cons = 0, n_cst = 0;
    void widen(const BatchDims& o) {
        m = m > o.m ? m : o.m, n_mul = n_mul > o.n_mul ? n_mul : o.n_mul;
        n_cons = n_cons > o.n_cons ? n_cons : o.n_cons, n_cst = n_cst > o.n_cst ? n_cst : o.n_cst;
    }
};

// ---- the encoding block (u32 words) and the point block of one proof ----------------------------------------------------------------
// enc, 8 words a record: V[m] | A_I1 A_O1 S1 | T_1 T_3 T_4 T_5 T_6 | (L_r R_r), r = 1..11 -- k_assemble walks the records m .. m + 30
BBP_HD u32 enc_words(u32 m) { return (m + 8 + 22) * 8; }              // per-proof stride
BBP_HD u32 enc_rec(u32 k) { return 8 * k; }                           // record k of the block
BBP_HD u32 enc_V(u32 i) { return enc_rec(i); }                        // V_i
BBP_HD u32 enc_A(u32 m) { return enc_rec(m); }                        // A_I1; A_O1 and S1 follow
BBP_HD u32 enc_T(u32 m) { return enc_rec(m + 3); }                    // T_1; T_3, T_4, T_5, T_6 follow
BBP_HD u32 enc_LR(u32 m, u32 r) { return enc_rec(m + 8 + 2 * (r - 1)); }  // L_r; R_r follows
// pts: V[m] | A_I1 A_O1 S1 | T_1 T_3 T_4 T_5 T_6
BBP_HD u32 pts_count(u32 m) { return m + 8; }                         // per-proof stride
BBP_HD size_t pts_T(u32 m) { return (size_t)m + 3; }                  // T_1

// ---- the one list: field, element type, elements per proof (d: the BatchDims), in the order of the carve ---------------------------
#define BBP_BATCH_ARRAYS(X)                                                                                          \
    X(cst, sc, d.n_cst)                      /* the constant table (circuit.h CST_*) */                              \
    X(v, sc, d.m)                            /* committed values */                                                  \
    X(vb, sc, d.m)                           /* ... and their blindings */                                           \
    X(ai1, sc, 1 + 2 * d.n_mul)              /* i_blinding, a_L, a_R */                                              \
    X(ao1, sc, 1 + d.n_mul)                  /* o_blinding, a_O */                                                   \
    X(s1, sc, 1 + 2 * d.n_mul)               /* s_blinding, s_L, s_R */                                              \
    X(tr, merlin_transcript, 1)                                                                                      \
    X(rng, merlin_transcript, 1)                                                                                     \
    X(misc, sc, MS_COUNT)                    /* MiscSlot */                                                          \
    X(zpow, sc, d.n_cons + 1)                /* z^0 .. z^n_cons */                                                   \
    X(ypow, sc, IPA_TERMS)                                                                                           \
    X(yipow, sc, IPA_N)                                                                                              \
    X(wl, sc, IPA_N)                         /* n_mul weights, zero padded by the verifier */                        \
    X(wr, sc, IPA_N)                                                                                                 \
    X(wo, sc, IPA_N)                                                                                                 \
    X(wv, sc, d.m)                                                                                                   \
    X(l1, sc, d.n_mul)                                                                                               \
    X(r0, sc, d.n_mul)                                                                                               \
    X(r1, sc, d.n_mul)                                                                                               \
    X(r3, sc, d.n_mul)                                                                                               \
    X(a, sc, IPA_N)                          /* IPA vectors, folded in place */                                      \
    X(b, sc, IPA_N)                                                                                                  \
    X(g, sc, IPA_N)                          /* per-generator accumulated factors */                                 \
    X(h, sc, IPA_N)                                                                                                  \
    X(lr, sc, 2 * IPA_TERMS)                 /* scalars of L and R of the current round */                           \
    X(pts, ge, pts_count(d.m))                                                                                       \
    X(lrpts, ge, 2)                                                                                                  \
    X(fpts, ge, 2 * FOLD_CLS)                /* explicit folded generators of the IPA tail: F_G then F_H */          \
    X(enc, u32, enc_words(d.m))                                                                                      \
    X(entropy, u8, entropy_row_bytes(d.m - 4)) /* the caller's row: blindings, then the rng seed */

// All per-proof arrays of a batch: every pointer is [B][stride], the stride being the list's count.
struct BatchDev {
#define X(name, T, count) T* name = nullptr;
    BBP_BATCH_ARRAYS(X)
#undef X
};
// elements per proof of every array, for launch arguments
struct BatchStrides {
#define X(name, T, count) u32 name = 0;
    BBP_BATCH_ARRAYS(X)
#undef X
};
inline BatchStrides batch_strides(const BatchDims& d) {
    BatchStrides s;
#define X(name, T, count) s.name = (u32)(count);
    BBP_BATCH_ARRAYS(X)
#undef X
    return s;
}
// byte offset of every array in one reservation, and its size
struct BatchOffsets {
#define X(name, T, count) size_t name = 0;
    BBP_BATCH_ARRAYS(X)
#undef X
    size_t bytes = 0;
};
// the carve of B proofs: every array 256-aligned behind the one before
inline BatchOffsets batch_offsets(u32 B, const BatchDims& d) {
    BatchOffsets o;
#define X(name, T, count) o.name = o.bytes, o.bytes += align256((size_t)(count) * sizeof(T) * B);
    BBP_BATCH_ARRAYS(X)
#undef X
    return o;
}
inline BatchDev batch_carve(u8* base, const BatchOffsets& o) {
    BatchDev bd;
#define X(name, T, count) bd.name = reinterpret_cast<T*>(base + o.name);
    BBP_BATCH_ARRAYS(X)
#undef X
    return bd;
}
// pointers of `bd` advanced to proof `first`
inline BatchDev batch_view(const BatchDev& bd, const BatchDims& d, u32 first) {
    BatchDev v = bd;
#define X(name, T, count) v.name += (size_t)first * (size_t)(count);
    BBP_BATCH_ARRAYS(X)
#undef X
    return v;
}

}  // namespace bbp
