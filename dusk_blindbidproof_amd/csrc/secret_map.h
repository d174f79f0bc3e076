// Secret wiping (include/bbp.h "Secret wiping"): the one list of what the context owns, each buffer classed SECRET or PUBLIC.  The rule
// is DEFAULT-SECRET: whatever a prove-side call writes is SECRET unless it is named PUBLIC here, with the reason.
//   BBP_CTX_DEVICE_BUFFERS / BBP_CTX_PINNED_BUFFERS   every buffer of the context: wipe.hip expands these two lists, and nothing else, for
//                                                     the wipe-everything pass, the residue count and the pattern scan
//   BBP_BATCH_SECRET / BBP_BATCH_PUBLIC               the arrays inside a batch buffer.  They are the record of why a batch buffer is
//                                                     SECRET and what of it is not; no engine path expands them, because a batch buffer is
//                                                     erased as a whole (below), and the CPU tier (tests/secret_map_check.cpp) holds them
//                                                     against BBP_BATCH_ARRAYS
// The call paths erase what they wrote through DevBuf::dirty (context.h).  No HIP calls: the CPU test tier compiles it too; DESIGN.md
// "Secret wiping" has the placement rules.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "batch_layout.h"
#include "secure_zero.h"

namespace bbp {

// ---- the per-proof batch arrays (batch_layout.h BBP_BATCH_ARRAYS), each classed exactly once ----------------------------------------
// SECRET: the witness and everything computed from it or from a blinding before the proof's public values exist.
#define BBP_BATCH_SECRET(X)                                                                                                      \
    X(cst, sc, d.n_cst)              /* the witness head writes the bid's scalars into it */                                    \
    X(v, sc, d.m)                                                                                                                \
    X(vb, sc, d.m)                                                                                                               \
    X(ai1, sc, 1 + 2 * d.n_mul)                                                                                                  \
    X(ao1, sc, 1 + d.n_mul)                                                                                                      \
    X(s1, sc, 1 + 2 * d.n_mul)                                                                                                   \
    X(tr, merlin_transcript, 1)      /* public by content, but cheap, and its rng sibling is not */                             \
    X(rng, merlin_transcript, 1)     /* TranscriptRng: keyed with the witness and the caller's seed */                          \
    X(misc, sc, MS_COUNT)            /* t_i, their blindings, y^-1 next to public challenges */                                 \
    X(wv, sc, d.m)                                                                                                               \
    X(l1, sc, d.n_mul)                                                                                                           \
    X(r0, sc, d.n_mul)                                                                                                           \
    X(r1, sc, d.n_mul)                                                                                                           \
    X(r3, sc, d.n_mul)                                                                                                           \
    X(a, sc, IPA_N)                  /* l(x), r(x) before the folds */                                                           \
    X(b, sc, IPA_N)                                                                                                              \
    X(g, sc, IPA_N)                                                                                                              \
    X(h, sc, IPA_N)                                                                                                              \
    X(lr, sc, 2 * IPA_TERMS)         /* scalars of L and R: halves of a and b */                                                \
    X(pts, ge, pts_count(d.m))       /* extended coordinates before encoding */                                                 \
    X(lrpts, ge, 2)                                                                                                              \
    X(fpts, ge, 2 * FOLD_CLS)                                                                                                    \
    X(entropy, u8, entropy_row_bytes(d.m - 4))
// PUBLIC: functions of the Fiat-Shamir challenges y and z (which the verifier recomputes from the record) and of the circuit alone, and
// the encodings that go into the record.
#define BBP_BATCH_PUBLIC(X)                                                                                                      \
    X(zpow, sc, d.n_cons + 1)        /* powers of z */                                                                           \
    X(ypow, sc, IPA_TERMS)           /* powers of y */                                                                           \
    X(yipow, sc, IPA_N)              /* powers of y^-1 */                                                                        \
    X(wl, sc, IPA_N)                 /* the circuit's weights flattened by z */                                                  \
    X(wr, sc, IPA_N)                                                                                                             \
    X(wo, sc, IPA_N)                                                                                                             \
    X(enc, u32, enc_words(d.m))      /* the 32-byte encodings of the record */
// A batch buffer is nevertheless wiped as a whole, public arrays included: the carve moves with B (every array starts behind B rows of
// the one before), so what one call leaves in a public array lies inside a secret array of the next call's carve, and a buffer whose
// secret arrays are to read zero over its whole capacity cannot keep it.

enum SecretClass : int { SC_PUBLIC = 0, SC_SECRET = 1 };

// how often `name` is classed (the CPU tier asserts exactly once for every name of BBP_BATCH_ARRAYS)
inline int batch_class_count(const char* name, int* cls) {
    int n = 0;
    auto same = [](const char* a, const char* b) {
        while (*a && *a == *b) a++, b++;
        return *a == *b;
    };
#define X(f, T, count) if (same(name, #f)) n++, *cls = SC_SECRET;
    BBP_BATCH_SECRET(X)
#undef X
#define X(f, T, count) if (same(name, #f)) n++, *cls = SC_PUBLIC;
    BBP_BATCH_PUBLIC(X)
#undef X
    return n;
}

// ---- spans ----------------------------------------------------------------------------------------------------------------------
// k_wipe_spans stores 16 bytes per lane and step: a span is a 16-aligned offset and a multiple of 16 bytes.
constexpr size_t WIPE_GRAIN = 16;
inline size_t wipe_round(size_t n) { return (n + WIPE_GRAIN - 1) / WIPE_GRAIN * WIPE_GRAIN; }
struct ByteSpan {
    size_t off, bytes;
    const char* name;
};
constexpr int BATCH_SPANS_MAX = 32;
struct BatchSpans {
    int n = 0;
    ByteSpan s[BATCH_SPANS_MAX];
};
// The rows [0, B) of every array of class `cls` (or of both: cls < 0) in the carve of B proofs.  The per-proof strides are multiples
// of 8 bytes (a transcript is 216), not of 16: a span is B rows rounded up to the grain, which stays inside the array's own 256-aligned
// slot of the carve -- asserted here for every array, not handled at run time.  false: an assertion failed (no engine path continues).
inline bool batch_spans(u32 B, const BatchDims& d, int cls, BatchSpans& out) {
    const BatchOffsets o = batch_offsets(B, d);
    bool ok = true;
    out.n = 0;
    auto add = [&](size_t off, size_t stride, const char* name) {
        const size_t bytes = wipe_round(stride * B);
        if (off % 256 || stride % 8 || bytes > align256(stride * B) || off + bytes > o.bytes || out.n >= BATCH_SPANS_MAX) {
            ok = false;
            return;
        }
        out.s[out.n++] = ByteSpan{off, bytes, name};
    };
    if (cls != SC_PUBLIC) {
#define X(f, T, count) add(o.f, (size_t)(count) * sizeof(T), #f);
        BBP_BATCH_SECRET(X)
#undef X
    }
    if (cls != SC_SECRET) {
#define X(f, T, count) add(o.f, (size_t)(count) * sizeof(T), #f);
        BBP_BATCH_PUBLIC(X)
#undef X
    }
    return ok;
}

// ---- the context's buffers (context.h) ----------------------------------------------------------------------------------------------
// X(name, field, count, secret): `field` is a DevBuf lvalue of the context `c` for index i < count; `secret`, an expression in i, its
// class; `name` is what bbp_debug_secret_residue reports.  P is bbp_ctx::PROVE_BUFS, V bbp_ctx::VERIFY_SLOT, S bbp_ctx::IO_SLOTS.
#define BBP_CTX_DEVICE_BUFFERS(X, P, V, S)                                                                                              \
    X("batch", c->batch[i], P + bbp_ctx::VLANES, i < P)      /* the prover's batch buffers; [P + lane]: a verifier lane's (public) */   \
    X("raw", c->raw[i], 4, true)                             /* TranscriptRng draws: blinding vectors before reduction */               \
    X("sorted", c->sorted, 1, true)                          /* the prover's MSM scratch: digits of secret scalars, bucket sums, */     \
    X("pts", c->pts, 1, true)                                /* unencoded points; slots V + lane are the verifier lanes' (public) */    \
    X("slice_sorted", c->slice_sorted[i], V + bbp_ctx::VLANES, i < V)                                                                   \
    X("slice_pts", c->slice_pts[i], V + bbp_ctx::VLANES, i < V)                                                                         \
    X("slice_fold", c->slice_fold[i], bbp_ctx::MAX_SLICES, true)                                                                        \
    /* slice_vtab: small multiples of a proof's folded generators F_G, F_H -- functions of the challenges and the public generators, */  \
    /* public by content like the batch array fpts they are built from; both are wiped because neither is argued public, and the */     \
    /* tables are the largest part of what a call erases (DESIGN.md "Secret wiping", cost) */                                            \
    X("slice_vtab", c->slice_vtab[i], bbp_ctx::MAX_SLICES, true)                                                                        \
    X("scal", c->scal, 1, true)                              /* the MSM hook's scalars are its caller's secret */                       \
    X("enc", c->enc, 1, true)                                /* ... and their result before it is handed over */                        \
    X("io_in", c->io_in, 1, true)                            /* bbp_witness_batch: d, k, seed in; y, y^-1, q out */                     \
    X("io_out", c->io_out, 1, true)                                                                                                     \
    X("io_ent", c->io_ent, 1, true)                          /* (no path reserves it today: classed so that one that does is covered) */ \
    X("io.in", c->io[i].in, S + bbp_ctx::IO_VSLOTS, i < S)   /* prove staging slots: rows, entropy and row keys, records and a round */ \
    X("io.ent", c->io[i].ent, S + bbp_ctx::IO_VSLOTS, i < S) /* call's toggles; slots S.. are the verify calls' (public) */             \
    X("io.out", c->io[i].out, S + bbp_ctx::IO_VSLOTS, i < S)                                                                            \
    X("rnd", c->rnd[i].buf, bbp_ctx::CHECK_RING, true)       /* round rings: bids' results, expanded rows; score records, gathered bids */ \
    X("sel", c->sel_dev, 1, true)                            /* bbp_prove_round_select phase A: every bid of the call, its score record */ \
    /* PUBLIC: checked proving's verify rows (record || q || z_img || seed || list, what any verifier is handed), verifier statuses and  \
       witness masks -- a mask is zero for a satisfied row and names the failed relation of a refused one, which the caller is told as   \
       status and message anyway */                                                                                                     \
    X("io.chk", c->io[i].chk, S + bbp_ctx::IO_VSLOTS, false)                                                                            \
    X("chk", c->chk[i].buf, bbp_ctx::CHECK_RING, false)                                                                                 \
    X("idx", c->idx, 1, false)                               /* index lists: functions of N */                                          \
    X("vl.misc", c->vl[i].misc, bbp_ctx::VLANES, false)      /* the verifier lanes: everything a verifier reads is public */            \
    X("vl.agg", c->vl[i].agg, bbp_ctx::VLANES, false)                                                                                   \
    X("vl.agg_io", c->vl[i].agg_io, bbp_ctx::VLANES, false)                                                                             \
    /* bbp_verify_round_best: proof rows, their claimed scores and the verifier's verdicts are what any verifier is handed or tells */   \
    X("best", c->best_dev, 1, false)                         /* keys, candidate and winner records, statuses, selections; the one-per-bidder calls: z_img of every row, the identity table (row indices), three counters; the many-rounds calls: round_of, row offsets, floors, per-round counters and segments; an offer to many standings (StandingsLayout): per-standing counters, the table of the standings' base pointers and K, working headers, serials, rank orders and the rows' local indices -- copies of standings' entries and addresses, nothing of a prover */ \
    X("best.rows", c->best_rows, 1, false)                   /* the _dev form's gathered rows and verifier entropy rows of one tranche */ \
    X("stand", c->stand[i], bbp_ctx::STANDINGS, false)       /* a standing's entries: claimed scores, z_img, serials of rows that verified -- verify-side data only */
// X(name, pointer, capacity, count, secret): the pinned mirrors of the staging slots
#define BBP_CTX_PINNED_BUFFERS(X, S)                                                                                                    \
    X("io.h_in", c->io[i].h_in, c->io[i].h_in_cap, S + bbp_ctx::IO_VSLOTS, i < S)                                                        \
    X("io.h_out", c->io[i].h_out, c->io[i].h_cap, S + bbp_ctx::IO_VSLOTS, i < S)                                                        \
    X("sel.h", c->sel_h, c->sel_h_cap, 1, true)              /* ... and its mirror: the bids going up, scores and selection coming down */ \
    X("best.h", c->best_h, c->best_h_cap, 1, false)          /* bbp_verify_round_best's mirror: claimed scores up, verdicts and ranks down (public) */
// Scratch discipline: a call reads only what it wrote itself, the resident tables, or state named here.  The test hook
// bbp_debug_poison_scratch fills every buffer of the two lists above EXCEPT these, so a buffer is poisoned unless it is exempt, and
// exempting one is a line here with the reason its contents outlive a call.  X(name, reason): `name` as in the lists above.
#define BBP_POISON_EXEMPT(X)                                                                                                            \
    X("stand", "a standing's entries live from bbp_standing_open to bbp_standing_close: every offer reads what the offers before it committed")
inline bool poison_exempt(const char* name) {
    auto same = [](const char* a, const char* b) {
        while (*a && *a == *b) a++, b++;
        return *a == *b;
    };
#define X(n, reason) if (same(name, n)) return true;
    BBP_POISON_EXEMPT(X)
#undef X
    return false;
}
// Not DevBufs, all PUBLIC, walked by the scan from wipe.hip: the resident tables gens, ptable, btab, comb, mimc_c (functions of public
// constants) and the verifier lanes' pinned ns_ring.  Not walked: the compiled circuits' lists and vctab (uploaded from host tables that
// are functions of N), and the counter words health, chk_counts, agg_count and the pinned h_flag.
}  // namespace bbp
