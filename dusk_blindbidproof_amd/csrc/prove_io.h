// What the rows of a prove call are and where a call keeps them: the row sizes of the prove side, named once, and the staging layout
// of one host-pointer prove call (bbp_prove_batch, bbp_prove_round) with its two siblings for the device forms' scratch rings.
// capi_prove.hip lays its buffers out by these values and bbp_reserve (capi_ctx.hip) sizes them by the same values (DESIGN.md "The host prove call").
// Plain arithmetic, no HIP calls: pool.cpp, prover.hip, the capi_*.hip units, round_bids.h and the CPU test tier (tests/host_check.cpp)
// include it; the helpers that kernels use are BBP_HD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bbp.h"
#include "field.h"
#include "verify_rows.h"

namespace bbp {

// ---- rows ----------------------------------------------------------------------------------------------------------------------
// bbp_prove_batch's input row: d,k,y,y_inv,q,z_img,seed (32 bytes each) || pub_list (N x 32) || toggle (u64 LE)
constexpr u32 PROVE_IN_Q = 4 * 32;           // byte offset of q; z_img and seed follow (the verify tail's first 96 bytes)
constexpr u32 PROVE_IN_LIST = 7 * 32;        // byte offset of the list
constexpr u32 PROVE_IN_LIST_WORD = 7 * 8;    // ... in 32-bit words
BBP_HD size_t prove_in_bytes(u32 N) { return 7 * 32 + 32 * (size_t)N + 8; }
BBP_HD size_t prove_in_words(u32 N) { return 7 * 8 + 8 * (size_t)N + 2; }
BBP_HD size_t prove_in_toggle(u32 N) { return PROVE_IN_LIST + 32 * (size_t)N; }  // byte offset of the toggle
BBP_HD u32 prove_in_toggle_word(u32 N) { return PROVE_IN_LIST_WORD + 8 * N; }
// the prover's entropy row (bbp_entropy_size): 4 + N blindings, then the rng seed
BBP_HD size_t entropy_row_bytes(u32 N) { return 32 * (4 + (size_t)N) + 32; }
// what a verify row holds behind its record: q || z_img || seed || pub_list
BBP_HD size_t verify_tail_bytes(u32 N) { return 96 + 32 * (size_t)N; }
BBP_HD size_t verify_tail_words(u32 N) { return 3 * 8 + 8 * (size_t)N; }
constexpr u32 VERIFY_TAIL_LIST_WORD = 3 * 8;
// one bid of a round call: d || k
constexpr size_t ROUND_BID_BYTES = BBP_ROUND_BID_BYTES;
inline size_t round_table_bytes(u32 N) { return 32 * (1 + (size_t)N); }  // seed || pub_list

inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// Scratch of one device pass of a round call (round_bids.h), byte offsets (256-aligned): the two round offsets k_round_consts reads,
// its flag, its reduced block, the RB_WORDS words per bid
constexpr u32 RB_WORDS = 36;
struct RoundScratch {
    size_t roff, rflag, rblk, rb, end;
};
inline RoundScratch round_scratch(u32 B, u32 N) {
    RoundScratch s;
    s.roff = 0;
    s.rflag = 256;
    s.rblk = 512;
    s.rb = s.rblk + align256(round_table_bytes(N));
    s.end = s.rb + align256(4 * (size_t)RB_WORDS * B);
    return s;
}

// Scratch of one selection pass (round_select.h), byte offsets (256-aligned): a RoundScratch for the `cap` bids that are expanded (its
// header serves the scoring too), the selection's state, the RS_WORDS words per bid of all B bids, the gathered bids
constexpr u32 RS_WORDS = 10;
constexpr size_t RS_STATE_BYTES = 4096;
struct SelectScratch {
    RoundScratch rs;
    size_t state, recs, gbids, end;
};
inline SelectScratch select_scratch(u32 B, u32 cap, u32 N) {
    SelectScratch s;
    s.rs = round_scratch(cap, N);
    s.state = s.rs.end;
    s.recs = s.state + RS_STATE_BYTES;
    s.gbids = s.recs + align256(4 * (size_t)RS_WORDS * B);
    s.end = s.gbids + align256(ROUND_BID_BYTES * cap);
    return s;
}
// Phase A of bbp_prove_round_select (context.h sel_dev and its pinned mirror sel_h): what is uploaded (bids, table), what is fetched
// (counts, sel, statuses, scores when asked for), the pass's scratch.  cap: entries of sel, at most B.  The mirror holds the uploaded
// region and then the fetched one.
struct SelectStaging {
    size_t bids, tab, up_bytes, counts, sel, status, scores, down_bytes, scratch, bytes, h_bytes;
    SelectScratch ss;
    SelectStaging(u32 B, u32 cap, u32 N, bool want_scores) : ss(select_scratch(B, 0, N)) {
        bids = 0;
        tab = align256(ROUND_BID_BYTES * B);
        up_bytes = tab + round_table_bytes(N);
        counts = align256(up_bytes);
        sel = counts + 256;
        status = sel + align256(4 * (size_t)cap);
        scores = status + align256(4 * (size_t)B);
        down_bytes = scores + (want_scores ? 32 * (size_t)B : 0) - counts;
        scratch = align256(counts + down_bytes);
        bytes = scratch + ss.end;
        h_bytes = up_bytes + down_bytes;
    }
};

// ---- the device forms' scratch rings (context.h chk, rnd) -----------------------------------------------------------------------------
// one entry of bbp_prove_batch_checked_dev: the check's scratch (verify rows, verifier statuses) as a staging slot's `chk`, then the
// witness masks
struct CheckRing {
    size_t vstatus, scratch_bytes, mask, bytes;
    CheckRing(u32 B, u32 N) {
        vstatus = align256(verify_row_bytes(N) * B);
        scratch_bytes = vstatus + 4 * (size_t)B;
        mask = align256(scratch_bytes);
        bytes = mask + 4 * (size_t)B;
    }
};
// one entry of bbp_prepare_round_dev / bbp_prove_round_dev: the pass's scratch; a prove call: its prove-input rows and its records
// behind it
struct RoundRing {
    RoundScratch rs;
    size_t rows, recs, bytes;
    RoundRing(u32 B, u32 N, bool prove) : rs(round_scratch(B, N)) {
        rows = rs.end;
        recs = rows + align256(prove_in_bytes(N) * B);
        bytes = prove ? recs + proof_record_bytes(N) * B : rs.end;
    }
};

// ---- the staging slot of one host-pointer prove call (context.h IoSlot) -----------------------------------------------------------
// Byte offsets into the slot's four device buffers and what of them travels through the pinned mirrors.  round: the call is a
// bbp_prove_round (raw bids and the round's table come in, rows record || score || z_img go out); check: checked proving; dev_draw:
// the prover's entropy is drawn on the device (only the check's weights are uploaded then); hedged (with dev_draw): each row is drawn
// under a key of its own (hedge.h), and the slot's entropy buffer holds the B row keys behind everything else.
struct ProveStaging {
    u32 B, N;
    bool round, check, dev_draw, hedged;
    size_t in_stride, ent_stride, rec, res_stride;  // per row: prove input, entropy, record, what the caller's `out` holds
    // `in`: the first uploaded region (the rows; a round call: the bids) at 0, then for a round call the table, the pass's scratch
    // and the rows the pass writes
    size_t in_first_stride, in_first_bytes, in_tab, in_tab_bytes, in_scratch, in_rows, in_upload, in_cap;
    RoundScratch rs;
    // `ent`: the prover's rows at 0 -- drawn there or uploaded -- then the check's weights, 32 bytes per row (always uploaded)
    // hedged: the row keys, 32 bytes per row, at ent_keys (0 bytes otherwise: ent_cap is then what it was)
    size_t ent_drawn, ent_up_off, ent_up_bytes, ent_keys, ent_keys_bytes, ent_cap;
    size_t ent_check(u32 first) const { return ent_stride * B + 32 * (size_t)first; }
    // `out`: what the caller receives at 0 (records; a round call: its output rows, the raw records lie at out_recs, unfetched), the
    // check's info block (statuses, witness masks, the count and the rows of rejected records), a round call's toggles and pass
    // statuses.  Everything the host reads lies below out_fetch.
    size_t out_recs, out_info, out_status, out_mask, out_fail_n, out_fail_idx, out_tog, out_pass_st, out_fetch, out_cap;
    // `chk` (checked calls): verify rows at 0, then the verifier's statuses
    size_t chk_vstatus, chk_bytes;
    size_t h_in_bytes, h_out_bytes;  // the pinned mirrors

    ProveStaging(u32 B_, u32 N_, bool round_, bool check_, bool dev_draw_, bool hedged_ = false)
        : B(B_), N(N_), round(round_), check(check_), dev_draw(dev_draw_), hedged(dev_draw_ && hedged_), rs(round_scratch(B_, N_)) {
        const size_t b = B;
        in_stride = prove_in_bytes(N), ent_stride = entropy_row_bytes(N), rec = proof_record_bytes(N);
        res_stride = round ? round_row_bytes(N) : rec;
        in_first_stride = round ? ROUND_BID_BYTES : in_stride, in_first_bytes = in_first_stride * b;
        in_tab = round ? align256(in_first_bytes) : 0;
        in_tab_bytes = round ? round_table_bytes(N) : 0;
        in_scratch = round ? align256(in_tab + in_tab_bytes) : 0;
        in_rows = round ? in_scratch + rs.end : 0;
        in_upload = round ? in_tab + in_tab_bytes : in_first_bytes;
        in_cap = in_rows + in_stride * b;

        ent_drawn = dev_draw ? ent_stride * b : 0;
        ent_up_off = ent_drawn;
        ent_up_bytes = (ent_stride * b - ent_drawn) + (check ? 32 * b : 0);
        ent_keys = ent_up_off + ent_up_bytes;  // a multiple of 32
        ent_keys_bytes = hedged ? 32 * b : 0;
        ent_cap = ent_keys + ent_keys_bytes;

        const size_t info_bytes = check ? 4 * (3 * b + 1) : 0;
        out_info = round || check ? align256(res_stride * b) : res_stride * b;
        out_status = out_info, out_mask = out_status + 4 * b, out_fail_n = out_mask + 4 * b, out_fail_idx = out_fail_n + 4;
        out_tog = round ? align256(out_info + info_bytes) : out_info + info_bytes;
        out_pass_st = out_tog + (round ? 8 * b : 0);
        out_fetch = out_pass_st + (round ? 4 * b : 0);
        out_recs = round ? align256(out_fetch) : 0;
        out_cap = round ? out_recs + rec * b : out_fetch;

        const CheckRing c(B, N);
        chk_vstatus = c.vstatus, chk_bytes = check ? c.scratch_bytes : 0;
        h_in_bytes = in_upload + ent_up_bytes;
        h_out_bytes = out_fetch;
    }
};

}  // namespace bbp
