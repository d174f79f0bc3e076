// Proving a round from raw bids (bbp_prepare_round_dev, bbp_prove_round[_dev]): what the reference's Go caller does upstream of
// Proof::prove for every bid of a round -- the witness (src/gadgets.rs:20-33, :70-86) and the bid's place in the public list -- from
// the round (seed || pub_list, once) and the bid (d || k, 64 bytes).  The per-row logic is host + device so that the CPU tier checks
// it against the big-int oracle (tests/round_bids_check.cpp); the kernels at the bottom are the device pass:
//   k_round_consts   (verifier_mixed.inc, unchanged)  the table, reduced once per call: seed flag, seed mod l, N x Scalar::from_bits
//   k_round_bids     one lane per bid: four MiMC chains, the search of the reduced list for x, y^-1, q -> RB_WORDS words per bid
//   k_round_expand   one lane per 32-bit word: bbp_prove_batch's input rows (list words from the ONE table), tails, toggles, statuses
//   k_round_rows     one lane per byte: record || score || z_img, the rows bbp_verify_rounds takes
#pragma once
#include "../../include/bbp.h"
#include "prove_io.h"
#include "witness_check.h"

namespace bbp {

// what k_round_bids leaves per bid, as 32-bit words (RB_WORDS of them, prove_io.h): y, y_inv, q, z_img (8 each), toggle (u64 LE),
// status, one word of padding.  A refused bid (status != BBP_OK) has every other word zero.
enum : u32 { RB_Y = 0, RB_YINV = 8, RB_Q = 16, RB_ZIMG = 24, RB_TOGGLE = 32, RB_STATUS = 34 };
static_assert(RB_STATUS + 2 == RB_WORDS, "prove_io.h sizes the pass's scratch by RB_WORDS");
// k_round_expand's outputs per bid, in words: the prove-input row (56 + 8 N + 2), then score || z_img, the toggle, the status
enum : u32 { RB_TAIL_WORDS = 16, RB_EXTRA_WORDS = RB_TAIL_WORDS + 2 + 1 };

BBP_HD u32 rb_le32(const u8* b) { return (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24); }
BBP_HD u32 round_in_words(u32 N) { return prove_in_toggle_word(N) + 2; }  // prove_in_words(N) in 32 bits: the toggle's two words end the row

// One bid against the reduced round.  bid: d || k (64 bytes, any alignment); rblk: seed mod l, then the N items as Scalar::from_bits
// values (k_round_consts' block for R = 1); seed_flag: BBP_ERR_FORMAT for a non-canonical seed, else BBP_OK; out: RB_WORDS words.
// Order of the checks (include/bbp.h): seed, then d and k canonical (x is undefined otherwise), then the search -- the LOWEST index
// whose item equals x = mimc(d, mimc(k, 0)); none: BBP_ERR_BAD_ARG, no witness exists.  The list is read at addresses every lane
// shares (scalar loads on the device); the loop runs downwards so that the lowest match is the last one kept, without a branch.
// In mimc(left, key) the seed is the chain's INPUT, its key is x (for y) or m (for z_img), both the bid's own: there is no per-call
// key schedule to hoist.
BBP_HD void round_bid_eval(u32 N, const u8* bid, const sc* rblk, int32_t seed_flag, const sc* mimc_c, u32* out) {
#pragma unroll
    for (u32 i = 0; i < RB_WORDS; i++) out[i] = 0;
    u32 dw[8], kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        dw[i] = rb_le32(bid + 4 * i);
        kw[i] = rb_le32(bid + 32 + 4 * i);
    }
    if (seed_flag != BBP_OK || !sc_is_canonical(dw) || !sc_is_canonical(kw)) {
        out[RB_STATUS] = (u32)BBP_ERR_FORMAT;
        return;
    }
    const sc d = wc_load(dw), k = wc_load(kw), seed = rblk[0];
    const sc m = wc_mimc(k, sc_zero(), mimc_c);
    const sc x = wc_mimc(d, m, mimc_c);
    u32 toggle = N;
    for (u32 i = N; i-- > 0;) toggle = sc_eq(rblk[1 + i], x) ? i : toggle;
    if (toggle >= N) {
        out[RB_STATUS] = (u32)BBP_ERR_BAD_ARG;
        return;
    }
    const sc y = wc_mimc(seed, x, mimc_c), z = wc_mimc(seed, m, mimc_c);
    const sc yi = sc_invert(y), q = sc_mul(d, yi);
    for (int i = 0; i < 8; i++) {
        out[RB_Y + i] = y.v[i];
        out[RB_YINV + i] = yi.v[i];
        out[RB_Q + i] = q.v[i];
        out[RB_ZIMG + i] = z.v[i];
    }
    out[RB_TOGGLE] = toggle;
    out[RB_STATUS] = (u32)BBP_OK;
}

// Word w < round_in_words(N) of the bid's prove-input row d,k,y,y_inv,q,z_img,seed || pub_list || toggle: d and k from the bid, the
// five scalars and the toggle from rb (round_bid_eval), seed and list RAW from the table (seed || pub_list is contiguous in both: row
// word 48 + j is table word j).  A refused bid's row is all zero: the stand-in bbp_prove_batch uses, so the batch keeps its geometry.
BBP_HD u32 round_expand_word(u32 N, u32 w, const u8* bid, const u8* table, const u32* rb) {
    if (rb[RB_STATUS] != (u32)BBP_OK) return 0;
    if (w < 16) return rb_le32(bid + 4 * w);
    if (w < 48) return rb[w - 16];
    if (w < 56 + 8 * N) return rb_le32(table + 4 * (size_t)(w - 48));
    return rb[RB_TOGGLE + (w - 56 - 8 * N)];
}

// Byte o < bbp_round_row_size(N) of the bid's output row record || score || z_img (score = q); all zero for a refused bid
BBP_HD u8 round_row_byte(u32 N, u32 o, const u8* record, const u32* rb) {
    const u32 rec = BBP_R1CS_PROOF_BYTES + 32 * (4 + N);
    if (rb[RB_STATUS] != (u32)BBP_OK) return 0;
    if (o < rec) return record[o];
    const u32 t = o - rec;  // < 64: q, then z_img -- adjacent in rb
    return (u8)(rb[RB_Q + (t >> 2)] >> (8 * (t & 3)));
}

// (the scratch of one device pass, RoundScratch / round_scratch: prove_io.h)

#if defined(__HIPCC__) && defined(BBP_ROUND_BIDS_KERNELS)  // the kernels: compiled by the one unit that launches them (capi.h)
// One lane per bid; the four chains are 1440 dependent Montgomery products, so the wave lives for milliseconds and is fenced onto
// CUs of its own by its launch (serial_lds_bytes), like k_prepare_bids.  Writes the bid's RB_WORDS words, nothing else.
// n_dev (NULL: all B): a device-side count -- only the first min(B, *n_dev) bids exist (bbp_select_round_dev sizes the launch by its cap).
__global__ void __launch_bounds__(64) k_round_bids(u32 B, u32 N, const u8* __restrict__ bids, const sc* __restrict__ rblk,
                                                   const int32_t* __restrict__ rflag, const sc* __restrict__ mimc, u32* __restrict__ rb,
                                                   const u32* __restrict__ n_dev) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B || (n_dev && p >= n_dev[0])) return;
    u32 o[RB_WORDS];
    round_bid_eval(N, bids + BBP_ROUND_BID_BYTES * (size_t)p, rblk, rflag[0], mimc, o);
    u32* dst = rb + (size_t)RB_WORDS * p;
#pragma unroll
    for (u32 i = 0; i < RB_WORDS; i++) dst[i] = o[i];
}

// One lane per output word, consecutive lanes on consecutive words of a bid: per bid the prove-input row, then (each unless NULL)
// score || z_img into tails, the toggle, the status.  n = B * (round_in_words(N) + RB_EXTRA_WORDS) lanes.  n_dev: as k_round_bids'.
__global__ void __launch_bounds__(256) k_round_expand(u32 n, u32 N, const u8* __restrict__ bids, const u8* __restrict__ table,
                                                      const u32* __restrict__ rb, u32* __restrict__ prove_in, u32* __restrict__ tails,
                                                      u32* __restrict__ toggles, int32_t* __restrict__ status, const u32* __restrict__ n_dev) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const u32 pw = round_in_words(N), per = pw + RB_EXTRA_WORDS, p = g / per, w = g - p * per;
    if (n_dev && p >= n_dev[0]) return;
    const u32* r = rb + (size_t)RB_WORDS * p;
    if (w < pw) {
        if (prove_in) prove_in[(size_t)pw * p + w] = round_expand_word(N, w, bids + BBP_ROUND_BID_BYTES * (size_t)p, table, r);
    } else if (w < pw + RB_TAIL_WORDS) {
        if (tails) tails[(size_t)RB_TAIL_WORDS * p + (w - pw)] = r[RB_Q + (w - pw)];
    } else if (w < pw + RB_TAIL_WORDS + 2) {
        if (toggles) toggles[2 * (size_t)p + (w - pw - RB_TAIL_WORDS)] = r[RB_TOGGLE + (w - pw - RB_TAIL_WORDS)];
    } else if (status)
        status[p] = (int32_t)r[RB_STATUS];
}

// One lane per byte of the output rows (records are 1121 + 32 m bytes -- odd -- so byte-granular, like k_check_rows)
__global__ void __launch_bounds__(256) k_round_rows(u32 B, u32 N, const u8* __restrict__ recs, const u32* __restrict__ rb, u8* __restrict__ rows) {
    const size_t rec = BBP_R1CS_PROOF_BYTES + 32 * (4 + (size_t)N), row = rec + 64;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= row * B) return;
    const size_t p = i / row;
    rows[i] = round_row_byte(N, (u32)(i - p * row), recs + rec * p, rb + (size_t)RB_WORDS * p);
}
#endif

}  // namespace bbp
