// Selecting a round's bids (bbp_select_round_dev, bbp_prove_round_select, bbp_debug_round_select): score every bid of a round, keep
// the K best at or above a floor, prove only those.  The rules (include/bbp.h "Selecting a round's bids") are stated once, in plain
// C++, by round_select_host; the kernels at the bottom are held to it (tests/round_select_check.cpp on the host,
// tests/test_gpu_round_select.py on the device):
//   k_round_scores   one lane per bid, a throughput launch: three MiMC chains, the list search, y^-1, q -> RS_WORDS words per bid
//   k_round_select_* radix select of the K-th key from the most significant byte down, then an ordered compaction, over many workgroups
//   k_round_gather   the selected bids, in index order, for k_round_bids / k_round_expand (round_bids.h)
#pragma once
#include <algorithm>

#include "round_bids.h"

namespace bbp {

// the score record of one bid, as 32-bit words: q (8, little-endian words of the canonical score), status, toggle.  A refused bid
// (status != BBP_OK) has every other word zero.
enum : u32 { RS_Q = 0, RS_STATUS = 8, RS_TOGGLE = 9 };
static_assert(RS_TOGGLE + 1 == RS_WORDS, "prove_io.h sizes the selection's scratch by RS_WORDS");

// a >= b, both 256-bit integers as eight little-endian words: most significant word first
BBP_HD bool rs_ge256(const u32* a, const u32* b) {
    for (int w = 7; w >= 0; w--)
        if (a[w] != b[w]) return a[w] > b[w];
    return true;
}
// the qualifying predicate: an accepted bid whose score is at or above the floor
BBP_HD bool rs_qualifies(const u32* rec, const u32* floor) { return rec[RS_STATUS] == (u32)BBP_OK && rs_ge256(rec + RS_Q, floor); }

// the top nb bytes (0..32) of a against those of b: -1, 0, 1.  Byte 0 of that order is the most significant byte of word 7.
BBP_HD int rs_cmp_top(const u32* a, const u32* b, u32 nb) {
    for (int w = 7; w >= 0 && nb > 0; w--) {
        u32 x = a[w], y = b[w];
        if (nb < 4) {
            const u32 sh = 8 * (4 - nb);
            x >>= sh, y >>= sh, nb = 0;
        } else
            nb -= 4;
        if (x != y) return x > y ? 1 : -1;
    }
    return 0;
}
BBP_HD u32 rs_key_byte(const u32* q, u32 pos) { return (q[7 - (pos >> 2)] >> (24 - 8 * (pos & 3))) & 0xffu; }  // pos 0 = most significant

// floor32 as the caller passes it (unsigned 256-bit little-endian, any alignment) -> words
struct RsFloor {
    u32 w[8];
};
BBP_HD RsFloor rs_floor_load(const u8* floor32) {
    RsFloor f;
    for (int i = 0; i < 8; i++) f.w[i] = rb_le32(floor32 + 4 * i);
    return f;
}

// The rules.  records: B x RS_WORDS; floor: 8 words; sel: room for B indices.  Q = accepted bids at or above the floor; K == 0 or
// |Q| <= K: all of Q, else the K members that come first under (score descending, index ascending); sel lists them by ascending index.
inline void round_select_host(u32 B, const u32* records, const u32* floor, u32 K, u32* sel, u32* n_sel, u32* n_qualified) {
    u32 nq = 0;
    for (u32 i = 0; i < B; i++)
        if (rs_qualifies(records + (size_t)RS_WORDS * i, floor)) sel[nq++] = i;
    *n_qualified = nq;
    *n_sel = nq;
    if (K == 0 || nq <= K) return;
    auto better = [&](u32 a, u32 b) {  // a comes before b: score descending, index ascending
        const int c = rs_cmp_top(records + (size_t)RS_WORDS * a + RS_Q, records + (size_t)RS_WORDS * b + RS_Q, 32);
        return c ? c > 0 : a < b;
    };
    std::sort(sel, sel + nq, better);
    std::sort(sel, sel + K);
    *n_sel = K;
}

// Screening of bbp_prove_round_select, before anything runs; the first failing check decides.  *done: the call ends here with the
// status returned (B == 0).  The NULL checks are the caller's (they name pointers); these are the checks on the numbers.
BBP_HD int32_t round_select_screen(u32 N, u32 B, bool* done) {
    *done = true;
    if (N == 0) return BBP_ERR_BAD_ARG;
    if (N > BBP_MAX_ITEMS) return BBP_ERR_GENS_LEN;
    if (B > BBP_SELECT_MAX_BIDS) return BBP_ERR_BAD_ARG;
    *done = B == 0;
    return BBP_OK;
}

// One bid's score record against the reduced round (rblk, seed_flag, mimc_c as round_bid_eval's).  The same checks in the same order
// as round_bid_eval; three chains: z_img = mimc(seed, m) is not needed to select.
BBP_HD void round_score_eval(u32 N, const u8* bid, const sc* rblk, int32_t seed_flag, const sc* mimc_c, u32* out) {
#pragma unroll
    for (u32 i = 0; i < RS_WORDS; i++) out[i] = 0;
    u32 dw[8], kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        dw[i] = rb_le32(bid + 4 * i);
        kw[i] = rb_le32(bid + 32 + 4 * i);
    }
    if (seed_flag != BBP_OK || !sc_is_canonical(dw) || !sc_is_canonical(kw)) {
        out[RS_STATUS] = (u32)BBP_ERR_FORMAT;
        return;
    }
    const sc d = wc_load(dw);
    const sc m = wc_mimc(wc_load(kw), sc_zero(), mimc_c);
    const sc x = wc_mimc(d, m, mimc_c);
    u32 toggle = N;
    for (u32 i = N; i-- > 0;) toggle = sc_eq(rblk[1 + i], x) ? i : toggle;
    if (toggle >= N) {
        out[RS_STATUS] = (u32)BBP_ERR_BAD_ARG;
        return;
    }
    const sc q = sc_mul(d, sc_invert(wc_mimc(rblk[0], x, mimc_c)));
#pragma unroll
    for (int i = 0; i < 8; i++) out[RS_Q + i] = q.v[i];
    out[RS_TOGGLE] = toggle;
    out[RS_STATUS] = (u32)BBP_OK;
}

#if defined(__HIPCC__) && defined(BBP_ROUND_SELECT_KERNELS)  // the kernels: compiled by the one unit that launches them (capi.h)
// One lane per bid, 64-lane workgroups so that a small call still spreads over the CUs, no LDS: the waves of several workgroups share
// a SIMD and hide each other's multiply latency (DESIGN.md "Selecting a round's bids" has the register and occupancy figures).
// Writes the bid's record, its status and -- unless NULL -- its score.
constexpr u32 RS_SCORE_T = 64;
__global__ void __launch_bounds__(RS_SCORE_T) k_round_scores(u32 B, u32 N, const u8* __restrict__ bids, const sc* __restrict__ rblk,
                                                             const int32_t* __restrict__ rflag, const sc* __restrict__ mimc,
                                                             u32* __restrict__ recs, int32_t* __restrict__ status, u32* __restrict__ scores) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    u32 o[RS_WORDS];
    round_score_eval(N, bids + BBP_ROUND_BID_BYTES * (size_t)p, rblk, rflag[0], mimc, o);
    u32* dst = recs + (size_t)RS_WORDS * p;
#pragma unroll
    for (u32 i = 0; i < RS_WORDS; i++) dst[i] = o[i];
    status[p] = (int32_t)o[RS_STATUS];
    if (scores) {
#pragma unroll
        for (u32 i = 0; i < 8; i++) scores[8 * (size_t)p + i] = o[RS_Q + i];
    }
}
#endif

// The selection, over many workgroups: workgroup g of G walks bids [g span, (g + 1) span), RS_SEL_T lanes each (rs_geom).  Its state
// between launches is one RsState in device memory, zeroed before the first launch.
//   k_round_select_pass   x 32, one per key byte from the most significant down; only when |Q| > K > 0 does more than the first do any
//                         work.  Per workgroup a 256-bin LDS histogram of byte `pass` over the members of Q that match the pivot's bytes
//                         so far, added to the state's; the workgroup that finishes LAST (a ticket drawn behind a fence) takes the sums,
//                         walks the bins from the top to the one that holds the K-th key, appends that byte to the pivot and keeps how
//                         many of that bin are still to take.  As soon as a bin is taken whole (honest scores: after three or four
//                         bytes) `stop` is set and the remaining launches return at once; after byte 31 the pivot is the K-th key itself.
//   k_round_select_count  members above the pivot (on the bytes decided) and equal to it, per workgroup; the last workgroup turns the
//                         counts into exclusive sums and writes counts = {n_sel, n_qualified}
//   k_round_select_write  ordered compaction: a member is selected when its key is above the pivot, or equal to it and among the first
//                         `rem` such members by index.  Exclusive sums across workgroups, wave ballots and a scan of the wave totals
//                         inside one: sel is in ascending index order whatever the hardware's timing.  sel[j] is written for j < cap.
constexpr u32 RS_SEL_T = 256, RS_SEL_G_MAX = 256;
struct RsGeom {
    u32 G, span;
};
BBP_HD RsGeom rs_geom(u32 B) {
    RsGeom g;
    g.G = (B + 4 * RS_SEL_T - 1) / (4 * RS_SEL_T);
    g.G = g.G < 1 ? 1 : g.G > RS_SEL_G_MAX ? RS_SEL_G_MAX : g.G;
    g.span = ((B + g.G - 1) / g.G + RS_SEL_T - 1) / RS_SEL_T * RS_SEL_T;
    return g;
}
struct RsState {
    u32 hist[256];
    u32 piv[8];
    u32 rem, stop, nb, nq;  // stop: 1 the pivot is decided on nb bytes, 2 all of Q is selected (nb = 0, rem = all ones)
    u32 done;               // the workgroups that have finished the current launch
    u32 wg_q[RS_SEL_G_MAX], wg_e[RS_SEL_G_MAX];  // per workgroup: members above / equal to the pivot, then their exclusive sums
};
static_assert(sizeof(RsState) <= RS_STATE_BYTES, "prove_io.h reserves RS_STATE_BYTES for the selection's state");

#if defined(__HIPCC__) && defined(BBP_ROUND_SELECT_KERNELS)
// true in exactly one workgroup of the launch: the one whose lanes arrive here last.  Everything the others wrote before is visible to it.
__device__ inline bool rs_last_workgroup(RsState* st) {
    __shared__ u32 s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&st->done, 1u) == gridDim.x - 1;
    __syncthreads();
    if (s_last) __threadfence();
    return s_last != 0;
}

__global__ void __launch_bounds__(RS_SEL_T) k_round_select_pass(u32 B, u32 span, const u32* __restrict__ recs, RsFloor floor, u32 K, u32 pass, RsState* st) {
    __shared__ u32 h[256];
    if (st->stop) return;  // (written by an earlier launch: every lane of every workgroup reads the same)
    const u32 tid = threadIdx.x, lo = blockIdx.x * span, hi = lo + span < B ? lo + span : B;
    u32 piv[8];
#pragma unroll
    for (int w = 0; w < 8; w++) piv[w] = st->piv[w];
    h[tid] = 0;
    __syncthreads();
    for (u32 i = lo + tid; i < hi; i += RS_SEL_T) {
        const u32* r = recs + (size_t)RS_WORDS * i;
        if (rs_qualifies(r, floor.w) && rs_cmp_top(r + RS_Q, piv, pass) == 0) atomicAdd(&h[rs_key_byte(r + RS_Q, pass)], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&st->hist[tid], h[tid]);
    if (!rs_last_workgroup(st)) return;
    h[tid] = atomicExch(&st->hist[tid], 0u);  // the sums of all workgroups; zero again for the next pass
    __syncthreads();
    if (tid != 0) return;
    st->done = 0;
    u32 rem = pass == 0 ? K : st->rem;
    if (pass == 0) {
        u32 nq = 0;
        for (u32 b = 0; b < 256; b++) nq += h[b];
        st->nq = nq;
        if (K == 0 || nq <= K) {  // all of Q: no byte decided, every member "equal", none turned away
            st->stop = 2, st->rem = 0xffffffffu, st->nb = 0;
            return;
        }
    }
    u32 b = 255;
    for (; b > 0 && h[b] < rem; b--) rem -= h[b];  // the bins above b are taken whole; bin b holds the K-th key
    st->piv[7 - (pass >> 2)] = piv[7 - (pass >> 2)] | (b << (24 - 8 * (pass & 3)));
    st->rem = rem, st->nb = pass + 1;
    if (h[b] == rem || pass == 31) st->stop = 1;  // this bin too is taken whole, or the pivot is the whole key
}

__global__ void __launch_bounds__(RS_SEL_T) k_round_select_count(u32 B, u32 span, const u32* __restrict__ recs, RsFloor floor, u32* __restrict__ counts,
                                                                 RsState* st) {
    __shared__ u32 cq[RS_SEL_T], ce[RS_SEL_T];
    const u32 tid = threadIdx.x, lo = blockIdx.x * span, hi = lo + span < B ? lo + span : B, nb = st->nb;
    u32 piv[8];
#pragma unroll
    for (int w = 0; w < 8; w++) piv[w] = st->piv[w];
    u32 q = 0, e = 0;
    for (u32 i = lo + tid; i < hi; i += RS_SEL_T) {
        const u32* r = recs + (size_t)RS_WORDS * i;
        if (rs_qualifies(r, floor.w)) {
            const int c = rs_cmp_top(r + RS_Q, piv, nb);
            q += c > 0, e += c == 0;
        }
    }
    cq[tid] = q, ce[tid] = e;
    __syncthreads();
    for (u32 d = RS_SEL_T / 2; d >= 1; d >>= 1) {
        if (tid < d) cq[tid] += cq[tid + d], ce[tid] += ce[tid + d];
        __syncthreads();
    }
    if (tid == 0) st->wg_q[blockIdx.x] = cq[0], st->wg_e[blockIdx.x] = ce[0];
    if (!rs_last_workgroup(st)) return;
    cq[tid] = tid < gridDim.x ? atomicAdd(&st->wg_q[tid], 0u) : 0;  // (gridDim.x <= RS_SEL_G_MAX = RS_SEL_T)
    ce[tid] = tid < gridDim.x ? atomicAdd(&st->wg_e[tid], 0u) : 0;
    __syncthreads();
    if (tid != 0) return;
    st->done = 0;
    u32 sq = 0, se = 0;
    for (u32 g = 0; g < gridDim.x; g++) {
        const u32 a = cq[g], b = ce[g];
        st->wg_q[g] = sq, st->wg_e[g] = se;
        sq += a, se += b;
    }
    const u32 rem = st->rem;
    counts[0] = sq + (se < rem ? se : rem), counts[1] = st->nq;
}

__global__ void __launch_bounds__(RS_SEL_T) k_round_select_write(u32 B, u32 span, const u32* __restrict__ recs, RsFloor floor, u32 cap, u32* __restrict__ sel,
                                                                 const RsState* __restrict__ st) {
    __shared__ u32 wq[2][RS_SEL_T / 64], we[2][RS_SEL_T / 64];
    const u32 tid = threadIdx.x, lo = blockIdx.x * span, hi = lo + span < B ? lo + span : B, nb = st->nb, rem = st->rem;
    const u32 lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    u32 piv[8];
#pragma unroll
    for (int w = 0; w < 8; w++) piv[w] = st->piv[w];
    u32 q_run = st->wg_q[blockIdx.x], e_run = st->wg_e[blockIdx.x];  // members above the pivot / equal to it at lower indices (every lane keeps both)
    for (u32 base = lo, par = 0; base < hi; base += RS_SEL_T, par ^= 1) {
        const u32 i = base + tid;
        bool q = false, e = false;
        if (i < hi) {
            const u32* r = recs + (size_t)RS_WORDS * i;
            if (rs_qualifies(r, floor.w)) {
                const int c = rs_cmp_top(r + RS_Q, piv, nb);
                q = c > 0, e = c == 0;
            }
        }
        const unsigned long long bq = __ballot(q), be = __ballot(e);
        if (lane == 0) wq[par][wave] = (u32)__popcll(bq), we[par][wave] = (u32)__popcll(be);
        __syncthreads();  // (one per step: the next step writes the other half of wq / we)
        u32 oq = 0, oe = 0, tq = 0, te = 0;
#pragma unroll
        for (u32 w = 0; w < RS_SEL_T / 64; w++) {
            const u32 a = wq[par][w], b = we[par][w];
            oq += w < wave ? a : 0, oe += w < wave ? b : 0;
            tq += a, te += b;
        }
        const u32 e_before = e_run + oe + (u32)__popcll(be & below);  // equal members at lower indices
        const u32 pos = q_run + oq + (u32)__popcll(bq & below) + (e_before < rem ? e_before : rem);
        if ((q || (e && e_before < rem)) && pos < cap) sel[pos] = i;
        q_run += tq, e_run += te;
    }
}

// One lane per byte of the gathered bids: row j < min(n_sel, cap) is bid sel[j] (bids of any alignment)
__global__ void __launch_bounds__(256) k_round_gather(u32 cap, const u32* __restrict__ sel, const u32* __restrict__ counts, const u8* __restrict__ bids,
                                                      u8* __restrict__ out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x, j = g / BBP_ROUND_BID_BYTES;
    if (j >= cap || j >= counts[0]) return;
    out[g] = bids[BBP_ROUND_BID_BYTES * (size_t)sel[j] + (g - j * BBP_ROUND_BID_BYTES)];
}
#endif

}  // namespace bbp
