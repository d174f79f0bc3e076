// Standings of many rounds (bbp_standings_offer, bbp_debug_standings_offer): one burst of rows, mixed over S open standings, offered to
// all of them in one call, step t of every standing that still runs verified in ONE engine call.  The rules (include/bbp.h "Standings of
// many rounds") are stated once, in plain C++, by standings_offer_host -- standing_offer_host per standing over its rows in ascending
// index, indices mapped back, steps counted, as rounds_best_distinct_host is built from round_best_distinct_host; the kernels at the bottom
// are held to it (tests/standings_check.cpp on the host, tests/test_gpu_standings.py on the device).
// WORKING rows of a call: W = sum K_s + B.  Standing s owns the entry slots [E_s, E_s + K_s), E the exclusive prefix of K; offer row i is
// working row sum K + i; a working round_of names the standing of every working row.  Within a standing ascending working index is
// "entries in rank order, then offer rows in call order": the invariant round_standing.h's tie-break argument rests on.  A call is a
// many-rounds one-per-bidder call (rounds_best_distinct.h) over the working rows with S "rounds": segments, scan, place, select, mark,
// settle and holders are rounds_best.h's and rounds_best_distinct.h's kernels, unchanged.  A standing's segment holds its candidates and,
// behind them, its K entry slots, so that the selection over the WINNER records with take[s] = K_s is the cut to K.  On top of them:
//   k_stands_seed      one lane per entry slot: the S standings' own allocations (through a table of base pointers) into the working
//                      winner and candidate records, ids, serials; lane 0 of a standing its working header; order
//   k_stands_enter     a launch of its own behind it: every held entry enters the identity table as its identity's holder, and every
//                      entry slot takes its place in its standing's segment behind the candidates (the segment starts are known by then)
//   k_stands_displace  one lane per entry slot, behind a step's holders: an entry's winner record closes when a row of the step took its
//                      (standing, z_img); sel's first sum K words are emptied for the selection of the winners that follows
//   k_stands_merge     one 256-lane workgroup per standing that took part in the step: the winners the selection kept into rank order
//                      by counting, keys in LDS -> that standing's order, count, bar and last; the trip flag on request
//   k_stands_leave     one lane per working row: k_stand_leave's two tests against the header of the row's OWN standing -- rank, not
//                      membership; left[s] and dups[s] counted per standing
//   k_stands_plan      one lane per standing: the segment sizes (candidates + K_s), the rows of step t (stands_take: no stop at K), or the
//                      winners to keep (K_s for a standing that took part in step t)
//   k_stands_commit    one lane per (standing, slot): the working standing into each standing's own allocation, the only memory written
#pragma once
#include "round_standing.h"
#include "rounds_best_distinct.h"

namespace bbp {

// the rows standing s contributes to step t: tranche t of its live candidates, nothing once none is live.  A standing that runs has run
// every step so far, so the step is its tranche number.  T_0 = max(tranche, K_s).
BBP_HD u32 stands_take(u32 K, u32 tranche, u32 t, u32 n_candidates, u32 examined, u32 dups, u32 left) {
    const unsigned long long gone = (unsigned long long)examined + dups + left;
    if (gone >= n_candidates) return 0;
    return best_tranche_rows(best_tranche0(K, tranche, n_candidates), t, n_candidates - (u32)gone);
}

// The rules.  states: the S standings; standing_of: B entries (null: standing 0); keys, ids: B x 8 words; verdicts: B; entered_out: S x
// cap; n_entered, n_candidates, n_examined, n_duplicates: S entries each; n_steps (may be null): the most tranches any standing ran;
// status: B; table_log2 (may be null): S entries, as standing_offer_host takes them.  Standing s: standing_offer_host over its rows in
// ascending index -- identities never meet across standings.  BBP_ERR_INTERNAL from any standing: no state changes.
inline int32_t standings_offer_host(u32 S, StandingState* states, u32 B, const u32* standing_of, const u32* keys, const u32* ids, const int32_t* verdicts,
                                    u32 tranche, u32 cap, u32* entered_out, u32* n_entered, u32* n_candidates, u32* n_examined, u32* n_duplicates, u32* n_steps,
                                    int32_t* status, const u32* table_log2 = nullptr) {
    std::vector<std::vector<u32>> rows(S);
    for (u32 i = 0; i < B; i++) rows[standing_of ? standing_of[i] : 0].push_back(i);
    std::vector<StandingState> next(states, states + S);
    std::vector<int32_t> st_all(B);
    u32 steps = 0;
    for (u32 s = 0; s < S; s++) {
        const u32 n = (u32)rows[s].size();
        std::vector<u32> k(8 * (size_t)n + 8), id(8 * (size_t)n + 8), entered(cap);
        std::vector<int32_t> v(n), st(n);
        for (u32 j = 0; j < n; j++) {
            memcpy(&k[8 * (size_t)j], keys + 8 * (size_t)rows[s][j], 32);
            memcpy(&id[8 * (size_t)j], ids + 8 * (size_t)rows[s][j], 32);
            v[j] = verdicts[rows[s][j]];
        }
        u32 ran = 0;
        if (standing_offer_host(next[s], n, k.data(), id.data(), v.data(), tranche, cap, entered.data(), &n_entered[s], &n_candidates[s], &n_examined[s],
                                &n_duplicates[s], st.data(), table_log2 ? table_log2[s] : 0, &ran))
            return BBP_ERR_INTERNAL;
        for (u32 j = 0; j < n; j++) st_all[rows[s][j]] = st[j];
        for (u32 j = 0; j < n_entered[s] && j < cap; j++) entered_out[(size_t)s * cap + j] = rows[s][entered[j]];
        steps = ran > steps ? ran : steps;
    }
    for (u32 s = 0; s < S; s++) states[s] = next[s];
    for (u32 i = 0; i < B; i++) status[i] = st_all[i];
    if (n_steps) *n_steps = steps;
    return BBP_OK;
}

// What the kernels know of standing s: a row of the parameter table, uploaded once per call.
enum : u32 {
    STANDS_P_PTR = 0 /* two words: the standing's own allocation */,
    STANDS_P_K = 2,
    STANDS_P_E = 3,    // its first entry slot
    STANDS_P_ROWS = 4, // the rows of the call that are offered to it
    STANDS_P_KEYS = 5, // byte offsets of StandingLayout(K)
    STANDS_P_IDS = 6,
    STANDS_P_SERIALS = 7,
    STANDS_P_WORDS = 8
};
constexpr u32 STANDS_H_STRIDE = 16;  // a working header: STAND_H_WORDS words, LAST a working index

// The extra state of a call, behind the state BestsDistinctLayout(BestsLayout(W, S, false), W, S, .., true) describes (same allocations:
// the context's best_dev and its pinned mirror).  sctr: per standing the candidates that left by the bar (their status stays
// BBP_ROW_SKIPPED), fetched with the other counters; par: the parameter table; whdr: S working headers; wserial: the entries' serials;
// order: every standing's rank order at [E_s ..], working indices; local: per offer row its index among the rows of its standing.
struct StandingsLayout {
    size_t sctr, par, whdr, wserial, order, local, bytes;
    size_t h_sctr, h_par, h_local, h_whdr, h_order, h_bytes;
    StandingsLayout(const BestsDistinctLayout& D, u32 S, u32 sumK, u32 B) {
        const size_t s = S, k = sumK, b = B;
        sctr = D.bytes;
        par = sctr + align256(4 * s);
        whdr = par + align256(4 * (size_t)STANDS_P_WORDS * s);
        wserial = whdr + align256(4 * (size_t)STANDS_H_STRIDE * s);
        order = wserial + align256(8 * k);
        local = order + align256(4 * k);
        bytes = local + align256(4 * b);
        h_sctr = D.h_bytes;
        h_par = h_sctr + align256(4 * s);
        h_local = h_par + align256(4 * (size_t)STANDS_P_WORDS * s);
        h_whdr = h_local + align256(4 * b);
        h_order = h_whdr + align256(4 * (size_t)STANDS_H_STRIDE * s);
        h_bytes = h_order + align256(4 * k);
    }
};

#ifdef __HIPCC__
// the standing that owns entry slot e < sum K (S <= BBP_STANDING_MAX_OPEN rows of par, E ascending); S when there is none
__device__ inline u32 stands_owner(const u32* __restrict__ par, u32 S, u32 e) {
    for (u32 s = 0; s < S; s++) {
        const u32* p = par + (size_t)STANDS_P_WORDS * s;
        if (e >= p[STANDS_P_E] && e - p[STANDS_P_E] < p[STANDS_P_K]) return s;
    }
    return S;
}
__device__ inline const u8* stands_alloc(const u32* p) {
    return (const u8*)(uintptr_t)(((unsigned long long)p[STANDS_P_PTR + 1] << 32) | p[STANDS_P_PTR]);
}

// One lane per entry slot e < sumK.  Everything read is a standing's own allocation or the parameter table.
__global__ void __launch_bounds__(BEST_T) k_stands_seed(u32 S, u32 sumK, const u32* __restrict__ par, u32* __restrict__ recs, u32* __restrict__ win,
                                                        u32* __restrict__ ids, int32_t* __restrict__ status, u32* __restrict__ whdr, u32* __restrict__ wserial,
                                                        u32* __restrict__ order) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= sumK) return;
    const u32 s = stands_owner(par, S, e);
    if (s >= S) return;
    const u32* p = par + (size_t)STANDS_P_WORDS * s;
    const u32 K = p[STANDS_P_K], E = p[STANDS_P_E], j = e - E;
    const u8* st = stands_alloc(p);
    const u32 *st_hdr = (const u32*)st, *st_keys = (const u32*)(st + p[STANDS_P_KEYS]), *st_ids = (const u32*)(st + p[STANDS_P_IDS]),
              *st_serials = (const u32*)(st + p[STANDS_P_SERIALS]);
    const u32 count = st_hdr[STAND_H_COUNT] < K ? st_hdr[STAND_H_COUNT] : K;
    if (j == 0) {
        u32* h = whdr + (size_t)STANDS_H_STRIDE * s;
        for (u32 w = 0; w < STAND_H_WORDS; w++) h[w] = st_hdr[w];
        h[STAND_H_COUNT] = count, h[STAND_H_LAST] = E + K - 1;  // (read only while count == K)
    }
    const bool held = j < count;
    u32 *r = recs + (size_t)RS_WORDS * e, *v = win + (size_t)RS_WORDS * e;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const u32 k = held ? st_keys[8 * (size_t)j + w] : 0;
        r[RS_Q + w] = k, v[RS_Q + w] = k;
        ids[8 * (size_t)e + w] = held ? st_ids[8 * (size_t)j + w] : 0;
    }
    r[RS_STATUS] = BEST_OUT, r[RS_TOGGLE] = s;
    v[RS_STATUS] = held ? (u32)BBP_OK : BEST_OUT, v[RS_TOGGLE] = s;
    status[e] = BBP_ROW_SKIPPED;
    wserial[2 * (size_t)e] = held ? st_serials[2 * (size_t)j] : 0, wserial[2 * (size_t)e + 1] = held ? st_serials[2 * (size_t)j + 1] : 0;
    order[e] = e;
}

// Behind the seed and behind the segment starts (k_bests_scan over the segment sizes), one lane per entry slot: the slot's place in its
// standing's segment -- behind the ncand[s] candidates, which k_bests_place fills -- and a held entry's place in the identity table.
// Entries of one standing have distinct identities: every insert claims an empty slot.
__global__ void __launch_bounds__(BEST_T) k_stands_enter(u32 S, u32 sumK, const u32* __restrict__ par, const u32* __restrict__ win, const u32* __restrict__ ids,
                                                         const u32* __restrict__ round_of, const u32* __restrict__ ncand, const u32* __restrict__ seg,
                                                         u32* __restrict__ cand, u32* table, u32 mask, u32* flag) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= sumK) return;
    const u32 s = stands_owner(par, S, e);
    if (s >= S) return;
    const u32 at = seg[s] + ncand[s] + (e - par[(size_t)STANDS_P_WORDS * s + STANDS_P_E]);
    if (at < seg[s + 1]) cand[at] = e;
    if (win[(size_t)RS_WORDS * e + RS_STATUS] == (u32)BBP_OK) bests_table_insert(table, mask, ids, round_of, win + RS_Q, RS_WORDS, e, sumK, flag);
}

// Behind k_bests_holders, one lane per entry slot: an entry whose identity a row of the step now holds is no winner any more.  (A row of
// the OFFER is never displaced: rows of later steps come after it in rank order.)  sel[e] is emptied: the selection of the winners
// writes min(K_s, winners) entries somewhere in sel[0 .. sumK), and the merge counts what it finds.
__global__ void __launch_bounds__(BEST_T) k_stands_displace(u32 sumK, const u32* __restrict__ ids, const u32* __restrict__ round_of,
                                                            const u32* __restrict__ table, u32 mask, u32* __restrict__ win, u32* __restrict__ sel, u32* flag) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= sumK) return;
    sel[e] = BEST_EMPTY;
    if (win[(size_t)RS_WORDS * e + RS_STATUS] != (u32)BBP_OK) return;
    if (bests_table_find(table, mask, ids, round_of, round_of[e], ids + 8 * (size_t)e, flag) != e) win[(size_t)RS_WORDS * e + RS_STATUS] = BEST_OUT;
}

// One workgroup per standing, behind the selection over the winner records; a standing with take[s] == 0 (it took no part in the step)
// leaves at once.  sel[off[s] ..] holds the at most K_s winners that stay, in any order, then BEST_EMPTY.  Their keys and indices go to
// LDS; every winner counts the winners that come before it in rank order (key descending, working index ascending: a total order, so
// the counts are a permutation) and writes its index there.  trip: bit s set -> the flag is raised (bbp_debug_standing_trip).
__global__ void __launch_bounds__(STAND_MERGE_T) k_stands_merge(u32 W, const u32* __restrict__ par, const u32* __restrict__ take, const u32* __restrict__ off,
                                                                const u32* __restrict__ sel, const u32* __restrict__ win, u32* __restrict__ whdr,
                                                                u32* __restrict__ order, unsigned long long trip, u32* flag) {
    __shared__ u32 key[8 * BBP_STANDING_MAX_K], idx[BBP_STANDING_MAX_K], n_s;
    const u32 s = blockIdx.x, tid = threadIdx.x;
    if (take[s] == 0) return;
    const u32* p = par + (size_t)STANDS_P_WORDS * s;
    const u32 K = p[STANDS_P_K], E = p[STANDS_P_E], o = off[s];
    if (K > BBP_STANDING_MAX_K) return;
    if (tid == 0) n_s = 0;
    __syncthreads();
    for (u32 j = tid; j < K; j += STAND_MERGE_T) {
        const u32 i = sel[o + j];
        idx[j] = i;
        if (i < W) atomicAdd(&n_s, 1u);
    }
    __syncthreads();
    const u32 n = n_s;  // (the selection fills a prefix)
    for (u32 x = tid; x < 8 * n; x += STAND_MERGE_T) key[x] = idx[x >> 3] < W ? win[(size_t)RS_WORDS * idx[x >> 3] + RS_Q + (x & 7)] : 0;
    __syncthreads();
    u32* h = whdr + (size_t)STANDS_H_STRIDE * s;
    for (u32 j = tid; j < n; j += STAND_MERGE_T) {
        u32 rank = 0;
        for (u32 m = 0; m < n; m++) {
            const int c = rs_cmp_top(key + 8 * m, key + 8 * j, 32);
            rank += c > 0 || (c == 0 && idx[m] < idx[j]);
        }
        order[E + rank] = idx[j];
        if (n == K && rank == K - 1) {
            h[STAND_H_LAST] = idx[j];
            for (int w = 0; w < 8; w++) h[STAND_H_BAR + w] = key[8 * j + w];
        }
    }
    if (tid == 0) {
        h[STAND_H_COUNT] = n;
        if ((trip >> s) & 1) atomicOr(flag, BEST_FLAG_TRIP);
    }
}

// The leave pass, one lane per working row; recs: the candidate records, whose keys order every working row.  A live candidate that does
// not come before entry K-1 of ITS standing leaves (its status stays BBP_ROW_SKIPPED, left[s] counts it); otherwise one whose identity's
// holder comes BEFORE it in rank order leaves with BBP_ROW_DUPLICATE (dups[s]).
__global__ void __launch_bounds__(BEST_T) k_stands_leave(u32 W, const u32* __restrict__ par, u32* __restrict__ recs, const u32* __restrict__ ids,
                                                         const u32* __restrict__ round_of, const u32* __restrict__ table, u32 mask,
                                                         const u32* __restrict__ whdr, int32_t* __restrict__ status, u32* left, u32* dups, u32* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = i < W;
    const u32 s = in_range ? round_of[i] : 0;
    bool gone = false, dup = false;
    if (in_range && recs[(size_t)RS_WORDS * i + RS_STATUS] == (u32)BBP_OK) {
        const u32* h = whdr + (size_t)STANDS_H_STRIDE * s;
        const u32 last = h[STAND_H_LAST];
        if (h[STAND_H_COUNT] >= par[(size_t)STANDS_P_WORDS * s + STANDS_P_K] && last < W && !best_before_at(recs + RS_Q, RS_WORDS, i, last))
            gone = true;
        else {
            const u32 holder = bests_table_find(table, mask, ids, round_of, s, ids + 8 * (size_t)i, flag);
            dup = holder != BEST_EMPTY && best_before_at(recs + RS_Q, RS_WORDS, holder, i);
        }
        if (gone || dup) recs[(size_t)RS_WORDS * i + RS_STATUS] = BEST_OUT;
        if (dup) status[i] = BBP_ROW_DUPLICATE;
    }
    bests_wave_add(left, s, in_range, gone);
    bests_wave_add(dups, s, in_range, dup);
}

// One lane per standing.  STANDS_PLAN_SEGMENTS: out[s] = ncand[s] + K_s, the size of its segment.  STANDS_PLAN_STEP: take[s] = the rows
// it contributes to step t, and tranches[s] = t + 1 when it contributes.  STANDS_PLAN_WINNERS: take[s] = K_s when it took part in step t,
// else 0 -- the selection over the winner records then is the cut to K.
enum : u32 { STANDS_PLAN_SEGMENTS = 0, STANDS_PLAN_STEP = 1, STANDS_PLAN_WINNERS = 2 };
__global__ void __launch_bounds__(BEST_T) k_stands_plan(u32 S, u32 mode, u32 t, u32 tranche, const u32* __restrict__ par, const u32* __restrict__ ncand,
                                                        const u32* __restrict__ examined, const u32* __restrict__ dups, const u32* __restrict__ left,
                                                        u32* __restrict__ out, u32* __restrict__ tranches) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const u32 K = par[(size_t)STANDS_P_WORDS * s + STANDS_P_K];
    if (mode == STANDS_PLAN_SEGMENTS)
        out[s] = ncand[s] + K;
    else if (mode == STANDS_PLAN_WINNERS)
        out[s] = tranches[s] == t + 1 ? K : 0;
    else {
        const u32 n = stands_take(K, tranche, t, ncand[s], examined[s], dups[s], left[s]);
        out[s] = n;
        if (n) tranches[s] = t + 1;
    }
}

// One lane per (standing, slot): entry j of standing s of the new standing is working row order[E_s + j] -- key and id from the working
// arrays, the serial an entry's own or, for an offer row, offered_s + its index among the rows offered to s.  Everything read is the
// call's scratch; only the standings' allocations are written.
__global__ void __launch_bounds__(BEST_T) k_stands_commit(u32 S, u32 sumK, u32 W, const u32* __restrict__ par, const u32* __restrict__ whdr,
                                                          const u32* __restrict__ order, const u32* __restrict__ win, const u32* __restrict__ ids,
                                                          const u32* __restrict__ wserial, const u32* __restrict__ local) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= sumK) return;
    const u32 s = stands_owner(par, S, e);
    if (s >= S) return;
    const u32* p = par + (size_t)STANDS_P_WORDS * s;
    const u32 K = p[STANDS_P_K], j = e - p[STANDS_P_E];
    u8* st = (u8*)stands_alloc(p);
    u32 *st_hdr = (u32*)st, *st_keys = (u32*)(st + p[STANDS_P_KEYS]), *st_ids = (u32*)(st + p[STANDS_P_IDS]), *st_serials = (u32*)(st + p[STANDS_P_SERIALS]);
    const u32* h = whdr + (size_t)STANDS_H_STRIDE * s;
    const u32 count = h[STAND_H_COUNT] < K ? h[STAND_H_COUNT] : K;
    const unsigned long long offered = ((unsigned long long)h[STAND_H_OFFERED + 1] << 32) | h[STAND_H_OFFERED];
    if (j == 0) {
        const unsigned long long now = offered + p[STANDS_P_ROWS];
        st_hdr[STAND_H_COUNT] = count, st_hdr[STAND_H_LAST] = count == K ? K - 1 : 0;
        st_hdr[STAND_H_OFFERED] = (u32)now, st_hdr[STAND_H_OFFERED + 1] = (u32)(now >> 32);
        for (int w = 0; w < 8; w++) st_hdr[STAND_H_BAR + w] = h[STAND_H_BAR + w];
    }
    if (j >= count) return;
    const u32 i = order[e];
    if (i >= W) return;
    for (int w = 0; w < 8; w++) st_keys[8 * (size_t)j + w] = win[(size_t)RS_WORDS * i + RS_Q + w], st_ids[8 * (size_t)j + w] = ids[8 * (size_t)i + w];
    const unsigned long long serial = i < sumK ? ((unsigned long long)wserial[2 * (size_t)i + 1] << 32) | wserial[2 * (size_t)i] : offered + local[i - sumK];
    st_serials[2 * (size_t)j] = (u32)serial, st_serials[2 * (size_t)j + 1] = (u32)(serial >> 32);
}
#endif

}  // namespace bbp
