// Best valid proofs of many rounds (bbp_verify_rounds_best, bbp_verify_rounds_best_dev, bbp_debug_rounds_best): the single-round rules
// of round_best.h kept per round, step t of every round that still runs verified in ONE engine call.  The rules (include/bbp.h "Best
// valid proofs of many rounds") are stated once, in plain C++, by rounds_best_host -- round_best_host per round, indices mapped back;
// the kernels at the bottom are held to it (tests/rounds_best_check.cpp on the host, tests/test_gpu_rounds_best.py on the device):
//   k_bests_keys     one lane per row: the 32 score bytes at any alignment, screened against l and the floor of the row's round -> the
//                    candidate and winner records of round_best.h (RS_TOGGLE carries the round), the initial status, ncand[round]++
//   k_bests_scan     an exclusive scan over R entries by one workgroup that loops: candidate counts -> segment starts, and every step
//                    take[r] -> the step's offsets (and, the _dev form, the byte offsets of the step's packed rows)
//   k_bests_place    candidate indices into their round's segment, in any order
//   k_bests_plan     one lane per round: the rows round r contributes to step t (bests_take), or the winners it reports
//   k_bests_select   one 256-lane workgroup per round that contributes: a radix select in LDS, most significant byte first, over the
//                    32 key bytes extended by the complemented row index -- every extended key is distinct, so the first take[r]
//                    members under (key descending, index ascending) are exactly those at or above the take[r]-th extended key, and
//                    the answer does not depend on the segment's order.  No cross-workgroup protocol.
//   k_bests_gather   the _dev form: a step's rows, of mixed sizes, packed back to back by round; k_best_gather's copy
//   k_bests_mark     a step's statuses scattered; the row leaves the candidates, an OK row enters the winners; examined[r], ok[r]
// A round's segment is walked by its ONE workgroup: every pass costs time linear in the segment, and a selection has 36 passes.  That
// is correct and slow for a very large round; the intended shape is many rounds of modest size (one large round: R == 1, which runs
// round_best.h's driver over round_select.h's many-workgroup selection).
#pragma once
#include <string.h>

#include "round_best.h"

namespace bbp {

constexpr u32 BESTS_EXT_BYTES = 36;  // 32 key bytes, then the complemented index, most significant byte first
constexpr u32 BESTS_PIV_WORDS = 9;   // an extended key as words: the key's eight, then the complemented index

// byte pos (0: most significant) of the extended key of row idx
BBP_HD u32 bests_ext_byte(const u32* q, u32 idx, u32 pos) { return pos < 32 ? rs_key_byte(q, pos) : (~idx >> (8 * (35 - pos))) & 0xffu; }
BBP_HD void bests_piv_set(u32* piv, u32 pos, u32 byte) {
    if (pos < 32)
        piv[7 - (pos >> 2)] |= byte << (24 - 8 * (pos & 3));
    else
        piv[8] |= byte << (8 * (35 - pos));
}
// the first p bytes (0..36) of the extended key of row idx are those of piv
BBP_HD bool bests_prefix_eq(const u32* q, u32 idx, const u32* piv, u32 p) {
    if (rs_cmp_top(q, piv, p < 32 ? p : 32) != 0) return false;
    return p <= 32 || ((~idx ^ piv[8]) >> (8 * (36 - p))) == 0;
}
// extended key of row idx >= piv: the row comes at or before the pivot in the candidate order
BBP_HD bool bests_ext_ge(const u32* q, u32 idx, const u32* piv) {
    const int c = rs_cmp_top(q, piv, 32);
    return c ? c > 0 : ~idx >= piv[8];
}
// a before b in the candidate order == extended key of a > extended key of b
BBP_HD bool bests_ext_before(const u32* qa, u32 ia, const u32* qb, u32 ib) {
    const int c = rs_cmp_top(qa, qb, 32);
    return c ? c > 0 : ~ia > ~ib;
}
// one radix pass: hist counts the members that match the pivot so far, by their next byte; the bin that holds the want-th member from
// the top, and how many of that bin's members are still wanted.  false: fewer than `want` members matched.
BBP_HD bool bests_pick_bin(const u32* hist, u32 want, u32* bin, u32* want_in_bin) {
    u32 above = 0;
    for (int b = 255; b >= 0; b--) {
        if (above + hist[b] >= want) return *bin = (u32)b, *want_in_bin = want - above, true;
        above += hist[b];
    }
    return false;
}
// the rows round r contributes to step t: nothing once it has stopped (K valid rows, or no candidate left), else tranche t
BBP_HD u32 bests_take(u32 K, u32 tranche, u32 t, u32 n_candidates, u32 examined, u32 ok) {
    const u32 live = n_candidates - examined;
    if (live == 0 || (K && ok >= K)) return 0;
    return best_tranche_rows(best_tranche0(K, tranche, n_candidates), t, live);
}
// the winners round r reports
BBP_HD u32 bests_winners(u32 K, u32 ok) { return K && K < ok ? K : ok; }

// Screening of the numbers, in the header's order (the NULL checks come first and are the caller's); *done: the call ends here.
// round_of may be null (R == 1 only).
inline int32_t rounds_best_screen(u32 R, const u32* round_Ns, u32 B, const u32* round_of, bool* done) {
    *done = true;
    if (R == 0 || R > BBP_BEST_MAX_ROUNDS) return BBP_ERR_BAD_ARG;
    for (u32 r = 0; r < R; r++)
        if (round_Ns[r] == 0) return BBP_ERR_BAD_ARG;
    for (u32 r = 0; r < R; r++)
        if (round_Ns[r] > BBP_MAX_ITEMS) return BBP_ERR_GENS_LEN;
    if (B > BBP_SELECT_MAX_BIDS) return BBP_ERR_BAD_ARG;
    if (B == 0) return BBP_OK;
    if (!round_of && R > 1) return BBP_ERR_BAD_ARG;
    for (u32 i = 0; round_of && i < B; i++)
        if (round_of[i] >= R) return BBP_ERR_BAD_ARG;
    *done = false;
    return BBP_OK;
}

// The rules.  keys: B x 8 words; round_of: B entries (null: round 0); verdicts: B; floors: R x 8 words; best_out: R x cap; n_best,
// n_candidates, n_examined: R entries each; status: B.  Round r: round_best_host over its rows in ascending index.
inline void rounds_best_host(u32 R, u32 B, const u32* round_of, const u32* keys, const int32_t* verdicts, const u32* floors, u32 K, u32 tranche, u32 cap,
                             u32* best_out, u32* n_best, u32* n_candidates, u32* n_examined, u32* n_steps, int32_t* status) {
    std::vector<std::vector<u32>> rows(R);
    for (u32 i = 0; i < B; i++) rows[round_of ? round_of[i] : 0].push_back(i);
    u32 steps = 0;
    for (u32 r = 0; r < R; r++) {
        const u32 n = (u32)rows[r].size();
        std::vector<u32> k(8 * (size_t)n + 8), best(cap);
        std::vector<int32_t> v(n), st(n);
        for (u32 j = 0; j < n; j++) {
            memcpy(&k[8 * (size_t)j], keys + 8 * (size_t)rows[r][j], 32);
            v[j] = verdicts[rows[r][j]];
        }
        round_best_host(n, k.data(), v.data(), floors + 8 * (size_t)r, K, tranche, cap, best.data(), &n_best[r], &n_candidates[r], &n_examined[r], st.data());
        for (u32 j = 0; j < n; j++) status[rows[r][j]] = st[j];
        for (u32 j = 0; j < n_best[r] && j < cap; j++) best_out[(size_t)r * cap + j] = rows[r][best[j]];
        // the tranches this round ran: the least t whose tranches hold n_examined rows
        const u32 T0 = best_tranche0(K, tranche, n_candidates[r]);
        u32 t = 0;
        for (unsigned long long seen = 0; seen < n_examined[r]; t++) seen += best_tranche_rows(T0, t, 0xffffffffu);
        steps = t > steps ? t : steps;
    }
    if (n_steps) *n_steps = steps;
}

// What k_bests_select computes, pass by pass, on the host: of the members seg[0..n) (row indices, any order) whose record is open, the
// first `take` in the candidate order -> out, in segment order.  Returns how many it wrote (take, when that many are open).
inline u32 bests_select_host(u32 n, const u32* seg, const u32* recs, u32 take, u32* out) {
    u32 piv[BESTS_PIV_WORDS] = {}, want = take, n_out = 0;
    if (take == 0) return 0;
    for (u32 pass = 0; pass < BESTS_EXT_BYTES; pass++) {
        u32 hist[256] = {};
        for (u32 m = 0; m < n; m++) {
            const u32* r = recs + (size_t)RS_WORDS * seg[m];
            if (r[RS_STATUS] == (u32)BBP_OK && bests_prefix_eq(r + RS_Q, seg[m], piv, pass)) hist[bests_ext_byte(r + RS_Q, seg[m], pass)]++;
        }
        u32 bin = 0;
        if (bests_pick_bin(hist, want, &bin, &want)) bests_piv_set(piv, pass, bin);
    }
    for (u32 m = 0; m < n; m++) {
        const u32* r = recs + (size_t)RS_WORDS * seg[m];
        if (r[RS_STATUS] == (u32)BBP_OK && bests_ext_ge(r + RS_Q, seg[m], piv) && n_out < take) out[n_out++] = seg[m];
    }
    return n_out;
}

// Where a call keeps its state: byte offsets (256-aligned) into the context's best_dev and its pinned mirror best_h.
//   device   ctr: 8 R + 2 words that one copy fetches -- per round ncand, examined, ok, take, tranches, fill (word offsets c_*: multiples of
//            R), then off (R + 1: the step's offsets, the step's rows at [R]) and seg (R + 1: the segment starts); offb (R + 1 u64: byte
//            offsets of a step's packed rows), floors (R x 8 words), rb (R: the row size of every round), round_of (B), rowoff (B u64:
//            where row i starts), cand (the segments), sel, keys (the host forms: the staged key bytes), the records, statuses, one
//            step's verdicts, the ranked pairs
//   pinned   what goes up (floors, rb, round_of, rowoff, keys), a step's verdicts going up, then what comes down: ctr, sel, pairs, statuses
struct BestsLayout {
    size_t ctr, offb, floors, rb, round_of, rowoff, cand, sel, keys, recs, win, status, tstat, pairs, bytes;
    size_t h_floors, h_rb, h_round_of, h_rowoff, h_keys, h_tstat, h_ctr, h_sel, h_pairs, h_status, h_bytes;
    u32 c_ncand, c_examined, c_ok, c_take, c_tranches, c_fill, c_off, c_seg, c_words;
    BestsLayout(u32 B, u32 R, bool host_keys) {
        const size_t b = B, r = R;
        c_ncand = 0, c_examined = R, c_ok = 2 * R, c_take = 3 * R, c_tranches = 4 * R, c_fill = 5 * R, c_off = 6 * R, c_seg = 7 * R + 1, c_words = 8 * R + 2;
        ctr = 0;
        offb = ctr + align256(4 * (size_t)c_words);
        floors = offb + align256(8 * (r + 1));
        rb = floors + align256(32 * r);
        round_of = rb + align256(4 * r);
        rowoff = round_of + align256(4 * b);
        cand = rowoff + (host_keys ? 0 : align256(8 * b));
        sel = cand + align256(4 * b);
        keys = sel + align256(4 * b);
        recs = keys + (host_keys ? align256(32 * b) : 0);
        win = recs + align256(4 * (size_t)RS_WORDS * b);
        status = win + align256(4 * (size_t)RS_WORDS * b);
        tstat = status + align256(4 * b);
        pairs = tstat + align256(4 * b);
        bytes = pairs + align256(4 * (size_t)BEST_PAIR_WORDS * b);
        h_floors = 0;
        h_rb = h_floors + align256(32 * r);
        h_round_of = h_rb + align256(4 * r);
        h_rowoff = h_round_of + align256(4 * b);
        h_keys = h_rowoff + (host_keys ? 0 : align256(8 * b));
        h_tstat = h_keys + (host_keys ? align256(32 * b) : 0);
        h_ctr = h_tstat + align256(4 * b);
        h_sel = h_ctr + align256(4 * (size_t)c_words);
        h_pairs = h_sel + align256(4 * b);
        h_status = h_pairs + align256(4 * (size_t)BEST_PAIR_WORDS * b);
        h_bytes = h_status + align256(4 * b);
    }
};

#ifdef __HIPCC__
constexpr u32 BESTS_T = 256;  // k_bests_scan, k_bests_select: one workgroup of four waves

// One lane per row.  The key is read byte by byte: at base + rowoff[i] + rb[round] - 64 (the _dev form: the score sits 64 bytes before
// the row's end), or, rowoff null, at base + 32 i (the staged keys).  round_of null: round 0.
__global__ void __launch_bounds__(BEST_T) k_bests_keys(u32 B, const u8* __restrict__ base, const unsigned long long* __restrict__ rowoff,
                                                       const u32* __restrict__ rb, const u32* __restrict__ round_of, const u32* __restrict__ floors,
                                                       u32* __restrict__ recs, u32* __restrict__ win, int32_t* __restrict__ status, u32* ncand) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const u32 rd = round_of ? round_of[i] : 0;
    const u8* p = rowoff ? base + rowoff[i] + rb[rd] - 64 : base + 32 * (size_t)i;
    u32 k[8];
#pragma unroll
    for (int w = 0; w < 8; w++) k[w] = rb_le32(p + 4 * w);
    const int32_t s = best_screen_key(k, floors + 8 * (size_t)rd);
    u32 *r = recs + (size_t)RS_WORDS * i, *v = win + (size_t)RS_WORDS * i;
#pragma unroll
    for (int w = 0; w < 8; w++) r[RS_Q + w] = k[w], v[RS_Q + w] = k[w];
    r[RS_STATUS] = s == BBP_OK ? (u32)BBP_OK : BEST_OUT, r[RS_TOGGLE] = rd;
    v[RS_STATUS] = BEST_OUT, v[RS_TOGGLE] = rd;
    status[i] = s == BBP_ERR_FORMAT ? (int32_t)BBP_ERR_FORMAT : (int32_t)BBP_ROW_SKIPPED;
    if (s == BBP_OK) atomicAdd(&ncand[rd], 1u);
}

// One workgroup, looping over R in spans of BESTS_T: out[r] = in[0] + .. + in[r - 1], out[R] the total; with sizes (the row size of
// every round) also outb[r] = the bytes of in[0] rows of size sizes[0], .. in front of round r's.
__global__ void __launch_bounds__(BESTS_T) k_bests_scan(u32 R, const u32* __restrict__ in, const u32* __restrict__ sizes, u32* __restrict__ out,
                                                        unsigned long long* __restrict__ outb) {
    __shared__ u32 s[BESTS_T];
    __shared__ unsigned long long sb[BESTS_T];
    const u32 tid = threadIdx.x;
    u32 carry = 0;
    unsigned long long carryb = 0;
    for (u32 base = 0; base < R; base += BESTS_T) {
        const u32 r = base + tid, v = r < R ? in[r] : 0;
        const unsigned long long vb = sizes && r < R ? (unsigned long long)v * sizes[r] : 0;
        s[tid] = v, sb[tid] = vb;
        __syncthreads();
        for (u32 d = 1; d < BESTS_T; d <<= 1) {
            const u32 a = tid >= d ? s[tid - d] : 0;
            const unsigned long long ab = tid >= d ? sb[tid - d] : 0;
            __syncthreads();
            s[tid] += a, sb[tid] += ab;
            __syncthreads();
        }
        if (r < R) {
            out[r] = carry + s[tid] - v;
            if (outb) outb[r] = carryb + sb[tid] - vb;
        }
        carry += s[BESTS_T - 1], carryb += sb[BESTS_T - 1];
        __syncthreads();
    }
    if (tid == 0) {
        out[R] = carry;
        if (outb) outb[R] = carryb;
    }
}

// One lane per row: a candidate's index into its round's segment (fill[r]: zero before the launch, ncand[r] after it).
__global__ void __launch_bounds__(BEST_T) k_bests_place(u32 B, const u32* __restrict__ recs, const u32* __restrict__ seg, u32* fill, u32* __restrict__ cand) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const u32* r = recs + (size_t)RS_WORDS * i;
    if (r[RS_STATUS] != (u32)BBP_OK) return;
    const u32 rd = r[RS_TOGGLE], at = atomicAdd(&fill[rd], 1u);
    if (seg[rd] + at < seg[rd + 1]) cand[seg[rd] + at] = i;
}

// One lane per round.  finish == 0: take[r] = the rows round r contributes to step t, and tranches[r] = t + 1 when it contributes;
// finish != 0: take[r] = the winners it reports.
__global__ void __launch_bounds__(BEST_T) k_bests_plan(u32 R, u32 t, u32 K, u32 tranche, u32 finish, const u32* __restrict__ ncand,
                                                       const u32* __restrict__ examined, const u32* __restrict__ ok, u32* __restrict__ take,
                                                       u32* __restrict__ tranches) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (finish) {
        take[r] = bests_winners(K, ok[r]);
        return;
    }
    const u32 n = bests_take(K, tranche, t, ncand[r], examined[r], ok[r]);
    take[r] = n;
    if (n) tranches[r] = t + 1;
}

// One workgroup per round; a round with take[r] == 0 leaves at once.  Members: cand[seg[r] .. seg[r + 1]) whose record in recs is open.
// 36 passes fix the extended key of the take[r]-th member from the top, a byte a pass: a 256-bin histogram in LDS of the members that
// match the pivot so far, suffix sums over the bins, the one bin that holds the wanted member.  Then every member at or above the pivot
// goes to sel[off[r] ..], at most take[r] of them whatever the records hold.
__global__ void __launch_bounds__(BESTS_T) k_bests_select(const u32* __restrict__ recs, const u32* __restrict__ cand, const u32* __restrict__ seg,
                                                          const u32* __restrict__ take, const u32* __restrict__ off, u32* __restrict__ sel) {
    const u32 rd = blockIdx.x, tid = threadIdx.x, tk = take[rd];
    if (tk == 0) return;
    const u32 lo = seg[rd], hi = seg[rd + 1];
    __shared__ u32 hist[BESTS_T], sfx[BESTS_T + 1], piv_s[BESTS_PIV_WORDS], want_s, n_out;
    if (tid < BESTS_PIV_WORDS) piv_s[tid] = 0;
    if (tid == 0) want_s = tk, n_out = 0, sfx[BESTS_T] = 0;
    u32 piv[BESTS_PIV_WORDS];
    for (u32 pass = 0; pass < BESTS_EXT_BYTES; pass++) {
        hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (u32 w = 0; w < BESTS_PIV_WORDS; w++) piv[w] = piv_s[w];
        for (u32 m = lo + tid; m < hi; m += BESTS_T) {
            const u32 i = cand[m];
            const u32* r = recs + (size_t)RS_WORDS * i;
            if (r[RS_STATUS] == (u32)BBP_OK && bests_prefix_eq(r + RS_Q, i, piv, pass)) atomicAdd(&hist[bests_ext_byte(r + RS_Q, i, pass)], 1u);
        }
        __syncthreads();
        sfx[tid] = hist[tid];
        __syncthreads();
        for (u32 d = 1; d < BESTS_T; d <<= 1) {  // sfx[b] = members in bins b .. 255
            const u32 a = tid + d < BESTS_T ? sfx[tid + d] : 0;
            __syncthreads();
            sfx[tid] += a;
            __syncthreads();
        }
        const u32 want = want_s;
        const bool mine = sfx[tid] >= want && sfx[tid + 1] < want;  // at most one lane: the suffix sums do not increase
        __syncthreads();
        if (mine) bests_piv_set(piv_s, pass, tid), want_s = want - sfx[tid + 1];
        __syncthreads();
    }
#pragma unroll
    for (u32 w = 0; w < BESTS_PIV_WORDS; w++) piv[w] = piv_s[w];
    const u32 o = off[rd];
    for (u32 m = lo + tid; m < hi; m += BESTS_T) {
        const u32 i = cand[m];
        const u32* r = recs + (size_t)RS_WORDS * i;
        if (r[RS_STATUS] == (u32)BBP_OK && bests_ext_ge(r + RS_Q, i, piv)) {
            const u32 at = atomicAdd(&n_out, 1u);
            if (at < tk) sel[o + at] = i;
        }
    }
}

// One workgroup per row of a step, or of the part of it that starts at step row `first` (n: the step's rows): row i = sel[first + j],
// rb[round_of[i]] bytes at rows + rowoff[i] (any alignment) -> out_rows + offb[round] + (first + j - off[round]) rb - part_base, the
// rows of a round behind one another, the rounds in ascending order; its entropy row -> row j of out_ent.  k_best_gather's copy: aligned
// 32-bit stores, a stored word put together from the two aligned source words that hold it, or -- where those would reach outside the
// source row -- from its four bytes.
__global__ void __launch_bounds__(BEST_GATHER_T) k_bests_gather(u32 n, u32 first, unsigned long long part_base, const u32* __restrict__ sel,
                                                                const u32* __restrict__ round_of, const u32* __restrict__ rbs, const u32* __restrict__ off,
                                                                const unsigned long long* __restrict__ offb, const unsigned long long* __restrict__ rowoff,
                                                                const u8* __restrict__ rows, const u8* __restrict__ ent, u8* __restrict__ out_rows,
                                                                u8* __restrict__ out_ent) {
    const u32 j = blockIdx.x, tid = threadIdx.x;
    if (first + j >= n) return;
    const u32 i = sel[first + j], rd = round_of ? round_of[i] : 0, rb = rbs[rd];
    if (first + j < off[rd] || first + j >= off[rd + 1]) return;  // (not a row of its round's part of the step: nothing is written)
    const u8* s = rows + rowoff[i];
    u8* d = out_rows + (offb[rd] + (unsigned long long)(first + j - off[rd]) * rb - part_base);
    if (tid < 32) out_ent[32 * (size_t)j + tid] = ent[32 * (size_t)i + tid];
    u32 head = (u32)(-(uintptr_t)d & 3);
    head = head < rb ? head : rb;
    if (tid < head) d[tid] = s[tid];
    const u32 nd = (rb - head) / 4, sh = (u32)((uintptr_t)(s + head) & 3);
    const u32* sw = (const u32*)(s + head - sh);
    u32* dw = (u32*)(d + head);
    for (u32 k = tid; k < nd; k += BEST_GATHER_T) {
        u32 v;
        if (sh == 0)
            v = sw[k];
        else if (head + 4 * k >= sh && head + 4 * k - sh + 8 <= rb)
            v = (sw[k] >> (8 * sh)) | (sw[k + 1] << (32 - 8 * sh));
        else
            v = rb_le32(s + head + 4 * k);
        dw[k] = v;
    }
    const u32 done = head + 4 * nd;
    if (tid < rb - done) d[done + tid] = s[done + tid];
}

// One lane per row of the step (n rows).  status[sel[j]] = tstat[j]; the row leaves the candidate records; an OK row enters the
// winners'; examined and ok of the row's round count it.
__global__ void __launch_bounds__(BEST_T) k_bests_mark(u32 n, const u32* __restrict__ sel, const int32_t* __restrict__ tstat, int32_t* __restrict__ status,
                                                       u32* __restrict__ recs, u32* __restrict__ win, u32* examined, u32* ok) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 i = sel[j];
    const int32_t st = tstat[j];
    u32* r = recs + (size_t)RS_WORDS * i;
    const u32 rd = r[RS_TOGGLE];
    status[i] = st;
    r[RS_STATUS] = BEST_OUT;
    atomicAdd(&examined[rd], 1u);
    if (st == BBP_OK) {
        win[(size_t)RS_WORDS * i + RS_STATUS] = (u32)BBP_OK;
        atomicAdd(&ok[rd], 1u);
    }
}
#endif

}  // namespace bbp
