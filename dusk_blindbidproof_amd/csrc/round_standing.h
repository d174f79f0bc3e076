// Standing of a round (bbp_standing_open, bbp_standing_offer, bbp_standing_read, bbp_standing_close, bbp_debug_standing_offer): the K best
// valid rows of a round so far, one per z_img, kept on the device while candidate rows arrive in bursts.  The rules (include/bbp.h
// "Standing of a round") are stated once, in plain C++, by standing_offer_host over a StandingState; the kernels at the bottom are held
// to it (tests/round_standing_check.cpp on the host, tests/test_gpu_round_standing.py on the device).
// An offer is a one-per-bidder call (round_best.h) over WORKING rows: rows 0..K-1 are the standing's entries in rank order (a row past
// the count is no member of anything), row K + j is row j of the offer.  A working index orders two rows of equal key as their serials
// do -- every entry was offered before every row of the offer, entries among themselves are kept in rank order -- so the identity
// table's row indices and best_before_at's tie-break mean what they mean there.  Keys, ids, selection, mark, settle and holders are
// round_best.h's and round_select.h's kernels; on top of them:
//   k_stand_seed      the entries into the working arrays: winner records that are open, candidate records that are not, ids, serials;
//                     every entry enters the identity table as its identity's holder; the working header (count, bar, last) and order
//   k_stand_displace  behind a tranche's holders: the winner record of an ENTRY closes when a row of the tranche took its identity
//   k_stand_merge     one workgroup: the winners the selection kept (the call's K, over the winner records) into rank order -> order,
//                     count, and once K are held the bar (the key of entry K-1) and its working index
//   k_stand_leave     the leave pass, one lane per working row: a live candidate that does not come before entry K-1 leaves (its status
//                     stays BBP_ROW_SKIPPED); otherwise one whose identity's holder comes BEFORE it in rank order leaves with
//                     BBP_ROW_DUPLICATE.  Rank, not membership (k_best_drop's test): a bidder may improve
//   k_stand_commit    the working standing into the standing's own allocation, once, at the end of an offer that succeeded
// A holder that the cut to K forgets stays in the table.  That is harmless: it comes after entry K-1, so a row it comes before has
// already left by the bar, and a row that comes before it is an improvement and displaces it on entering.
#pragma once
#include <vector>

#include "round_best.h"
#include "standing_handles.h"

namespace bbp {

constexpr u32 BEST_FLAG_TRIP = 4;  // bbp_debug_standing_trip: raised by k_stand_merge on request, so that a test sees an offer fail half-way
// dctr word 3, behind round_best.h's three: the live candidates that left by the bar (their status stays BBP_ROW_SKIPPED)
constexpr u32 STAND_D_LEFT = 3;
static_assert(STAND_D_LEFT == BEST_D_WORDS - 1, "the tally fetches BEST_D_WORDS words");

// The standing's own allocation: a header of 256 bytes, then K keys, K ids (8 words each) and K serials (2 words each).
enum : u32 { STAND_H_COUNT = 0, STAND_H_LAST = 1, STAND_H_OFFERED = 2 /* two words */, STAND_H_BAR = 4 /* eight words */, STAND_H_WORDS = 12 };
struct StandingLayout {
    size_t hdr, keys, ids, serials, bytes;
    explicit StandingLayout(u32 K) {
        hdr = 0;
        keys = 256;
        ids = keys + align256(32 * (size_t)K);
        serials = ids + align256(32 * (size_t)K);
        bytes = serials + align256(8 * (size_t)K);
    }
};
// What an offer adds behind the one-per-bidder state of BestDistinctLayout (K + B working rows): the working header, the entries'
// serials and the rank order; and in the pinned mirror what comes down at the end: header and order.
struct StandingWork {
    size_t whdr, wserial, order, bytes;
    size_t h_whdr, h_order, h_bytes;
    StandingWork(const BestDistinctLayout& D, u32 K) {
        whdr = D.bytes;
        wserial = whdr + 256;
        order = wserial + align256(8 * (size_t)K);
        bytes = order + align256(4 * (size_t)K);
        h_whdr = D.h_bytes;
        h_order = h_whdr + 256;
        h_bytes = h_order + align256(4 * (size_t)K);
    }
};

// a + 1 for a < 2^256 - 1 (a bar is a canonical scalar)
BBP_HD void stand_inc256(const u32* a, u32* out) {
    u32 carry = 1;
    for (int w = 0; w < 8; w++) {
        out[w] = a[w] + carry;
        carry = carry && out[w] == 0;
    }
}
// the floor an offer screens by: the standing's floor, or bar + 1 when the standing is full and that is higher -- at the start of an
// offer every new serial is later than every held one, so "comes before entry K-1" is "key >= bar + 1"
BBP_HD void stand_screen_floor(const u32* floor, bool full, const u32* bar, u32* out) {
    u32 b1[8];
    stand_inc256(bar, b1);
    const bool up = full && !rs_ge256(floor, b1);
    for (int w = 0; w < 8; w++) out[w] = up ? b1[w] : floor[w];
}

// The state of a standing as the host rule sees it: entries in rank order.
struct StandingState {
    u32 K = 0;
    u32 floor[8] = {};
    unsigned long long offered = 0;
    std::vector<u32> keys, ids;  // count x 8 words each
    std::vector<unsigned long long> serials;
    u32 count() const { return (u32)serials.size(); }
};

// The rules.  keys, ids: B x 8 words; verdicts: what verification says of row i (read for examined rows only); entered_out: room for cap
// entries; status: B entries.  table_log2: 0 for the call's own sizing (from K + B working rows), or an explicit size.  Returns BBP_OK,
// or BBP_ERR_INTERNAL with S untouched when a bounded loop of the identity table ran out.  ran (may be null): the tranches that ran.
inline int32_t standing_offer_host(StandingState& S, u32 B, const u32* keys, const u32* ids, const int32_t* verdicts, u32 tranche, u32 cap, u32* entered_out,
                                   u32* n_entered, u32* n_candidates, u32* n_examined, u32* n_duplicates, int32_t* status, u32 table_log2 = 0,
                                   u32* ran = nullptr) {
    const u32 K = S.K, n0 = S.count(), W = K + B;
    *n_entered = *n_candidates = *n_examined = *n_duplicates = 0;
    if (ran) *ran = 0;
    if (B == 0) return BBP_OK;
    std::vector<u32> wk(8 * (size_t)W, 0), wid(8 * (size_t)W, 0);
    std::copy(S.keys.begin(), S.keys.end(), wk.begin());
    std::copy(S.ids.begin(), S.ids.end(), wid.begin());
    std::copy(keys, keys + 8 * (size_t)B, wk.begin() + 8 * (size_t)K);
    std::copy(ids, ids + 8 * (size_t)B, wid.begin() + 8 * (size_t)K);
    const u32 log2 = table_log2 ? table_log2 : best_table_log2(W), mask = (1u << log2) - 1;
    std::vector<u32> table((size_t)mask + 1, BEST_EMPTY), held, live;
    u32 flag = 0;
    for (u32 e = 0; e < n0; e++) best_table_insert(table.data(), mask, wid.data(), wk.data(), 8, e, W, &flag), held.push_back(e);
    auto before = [&](u32 a, u32 b) { return best_before_at(wk.data(), 8, a, b); };
    u32 sfloor[8];
    stand_screen_floor(S.floor, n0 == K, n0 == K ? &wk[8 * (size_t)(K - 1)] : S.floor, sfloor);
    for (u32 j = 0; j < B; j++) {
        const int32_t s = best_screen_key(keys + 8 * (size_t)j, sfloor);
        status[j] = s == BBP_ERR_FORMAT ? (int32_t)BBP_ERR_FORMAT : (int32_t)BBP_ROW_SKIPPED;
        if (s == BBP_OK) live.push_back(K + j);
    }
    std::sort(live.begin(), live.end(), before);
    const u32 nc = (u32)live.size(), T0 = best_tranche0(K, tranche, nc);
    u32 examined = 0, dups = 0;
    auto leave = [&] {
        std::vector<u32> keep;
        for (u32 i : live) {
            if (held.size() == K && !before(i, held[K - 1])) continue;  // (stays BBP_ROW_SKIPPED)
            const u32 h = best_table_find(table.data(), mask, wid.data(), &wid[8 * (size_t)i], &flag);
            if (h != BEST_EMPTY && before(h, i))
                status[i - K] = BBP_ROW_DUPLICATE, dups++;
            else
                keep.push_back(i);
        }
        live.swap(keep);
    };
    leave();
    for (u32 t = 0; !live.empty(); t++) {
        const u32 n = best_tranche_rows(T0, t, (u32)live.size());
        std::vector<u32> next = held;
        for (u32 j = 0; j < n; j++) {
            const u32 i = live[j];
            status[i - K] = verdicts[i - K];
            if (verdicts[i - K] != BBP_OK) continue;
            best_table_insert(table.data(), mask, wid.data(), wk.data(), 8, i, W, &flag);
            next.push_back(i);
        }
        live.erase(live.begin(), live.begin() + n);
        examined += n;
        held.clear();  // the merge: whoever holds its identity, in rank order, the first K
        for (u32 i : next)
            if (best_table_find(table.data(), mask, wid.data(), &wid[8 * (size_t)i], &flag) == i) held.push_back(i);
        std::sort(held.begin(), held.end(), before);
        if (held.size() > K) held.resize(K);
        leave();
        if (ran) *ran = t + 1;
    }
    if (flag) return BBP_ERR_INTERNAL;
    StandingState N = S;
    N.keys.clear(), N.ids.clear(), N.serials.clear();
    u32 ne = 0;
    for (u32 i : held) {
        N.keys.insert(N.keys.end(), &wk[8 * (size_t)i], &wk[8 * (size_t)i] + 8);
        N.ids.insert(N.ids.end(), &wid[8 * (size_t)i], &wid[8 * (size_t)i] + 8);
        N.serials.push_back(i < K ? S.serials[i] : S.offered + (i - K));
        if (i >= K) {
            if (ne < cap) entered_out[ne] = i - K;
            ne++;
        }
    }
    N.offered = S.offered + B;
    S = N;
    *n_entered = ne, *n_candidates = nc, *n_examined = examined, *n_duplicates = dups;
    return BBP_OK;
}

// k_stand_merge's workgroup; standings.h's merge has the same
constexpr u32 STAND_MERGE_T = 256;
#if defined(__HIPCC__) && defined(BBP_ROUND_BEST_KERNELS)  // the kernels: compiled by the one unit that launches them (capi.h)
// One lane per entry slot e < K.  st_*: the standing's own allocation (read only).  An entry's working index is its slot; it enters the
// table through the standing's own arrays (stride 8, the same indices), so no lane reads what another lane of this launch writes.
// Entries have distinct identities: every insert claims an empty slot.
__global__ void __launch_bounds__(BEST_T) k_stand_seed(u32 K, const u32* __restrict__ st_hdr, const u32* __restrict__ st_keys, const u32* __restrict__ st_ids,
                                                       const u32* __restrict__ st_serials, u32* __restrict__ recs, u32* __restrict__ win, u32* __restrict__ ids,
                                                       int32_t* __restrict__ status, u32* table, u32 mask, u32* __restrict__ whdr, u32* __restrict__ wserial,
                                                       u32* __restrict__ order, u32* dctr) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 count = st_hdr[STAND_H_COUNT] < K ? st_hdr[STAND_H_COUNT] : K;
    if (e == 0)
        for (u32 w = 0; w < STAND_H_WORDS; w++) whdr[w] = st_hdr[w];
    if (e >= K) return;
    const bool held = e < count;
    u32 *r = recs + (size_t)RS_WORDS * e, *v = win + (size_t)RS_WORDS * e;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const u32 k = held ? st_keys[8 * (size_t)e + w] : 0;
        r[RS_Q + w] = k, v[RS_Q + w] = k;
        ids[8 * (size_t)e + w] = held ? st_ids[8 * (size_t)e + w] : 0;
    }
    r[RS_STATUS] = BEST_OUT, r[RS_TOGGLE] = 0;
    v[RS_STATUS] = held ? (u32)BBP_OK : BEST_OUT, v[RS_TOGGLE] = 0;
    status[e] = BBP_ROW_SKIPPED;
    wserial[2 * (size_t)e] = held ? st_serials[2 * (size_t)e] : 0, wserial[2 * (size_t)e + 1] = held ? st_serials[2 * (size_t)e + 1] : 0;
    order[e] = e;
    if (held) best_table_insert(table, mask, st_ids, st_keys, 8, e, K, &dctr[BEST_D_FLAG]);
}

// Behind k_best_holders, one lane per entry slot: an entry whose identity a row of the tranche now holds is no winner any more.  (A row
// of the OFFER is never displaced: rows of later tranches come after it in rank order.)
__global__ void __launch_bounds__(BEST_T) k_stand_displace(u32 K, const u32* __restrict__ ids, const u32* __restrict__ table, u32 mask, u32* __restrict__ win,
                                                           u32* dctr) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K || win[(size_t)RS_WORDS * e + RS_STATUS] != (u32)BBP_OK) return;
    if (best_table_find(table, mask, ids, ids + 8 * (size_t)e, &dctr[BEST_D_FLAG]) != e) win[(size_t)RS_WORDS * e + RS_STATUS] = BEST_OUT;
}

// ONE workgroup, behind the selection over the winner records with the call's K: sel holds the at most K winners that stay, in ascending
// index.  Their keys go to LDS; every winner counts the winners that come before it in rank order (key descending, index ascending: a
// total order, so the counts are a permutation) and writes its index there.  At most K^2 / STAND_MERGE_T comparisons per lane.
__global__ void __launch_bounds__(STAND_MERGE_T) k_stand_merge(u32 K, const u32* __restrict__ sel, const u32* __restrict__ counts, const u32* __restrict__ win,
                                                               u32* __restrict__ whdr, u32* __restrict__ order, u32 trip, u32* dctr) {
    __shared__ u32 key[8 * BBP_STANDING_MAX_K];
    const u32 n = counts[0] < K ? counts[0] : K, tid = threadIdx.x;
    if (K > BBP_STANDING_MAX_K) return;
    for (u32 x = tid; x < 8 * n; x += STAND_MERGE_T) key[x] = win[(size_t)RS_WORDS * sel[x >> 3] + RS_Q + (x & 7)];
    __syncthreads();
    for (u32 j = tid; j < n; j += STAND_MERGE_T) {
        u32 rank = 0;
        for (u32 m = 0; m < n; m++) {
            const int c = rs_cmp_top(key + 8 * m, key + 8 * j, 32);
            rank += c > 0 || (c == 0 && m < j);  // (sel ascends: position order is index order)
        }
        order[rank] = sel[j];
        if (n == K && rank == K - 1) {
            whdr[STAND_H_LAST] = sel[j];
            for (int w = 0; w < 8; w++) whdr[STAND_H_BAR + w] = key[8 * j + w];
        }
    }
    if (tid == 0) {
        whdr[STAND_H_COUNT] = n;
        if (trip) atomicOr(&dctr[BEST_D_FLAG], BEST_FLAG_TRIP);
    }
}

// The leave pass, one lane per working row; recs: the candidate records, whose keys order every working row.
__global__ void __launch_bounds__(BEST_T) k_stand_leave(u32 W, u32 K, u32* __restrict__ recs, const u32* __restrict__ ids, const u32* __restrict__ table, u32 mask,
                                                        const u32* __restrict__ whdr, int32_t* __restrict__ status, u32* dctr) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool left = false, dup = false;
    if (i < W && recs[(size_t)RS_WORDS * i + RS_STATUS] == (u32)BBP_OK) {
        const u32 last = whdr[STAND_H_LAST];
        if (whdr[STAND_H_COUNT] >= K && last < W && !best_before_at(recs + RS_Q, RS_WORDS, i, last))
            left = true;
        else {
            const u32 h = best_table_find(table, mask, ids, ids + 8 * (size_t)i, &dctr[BEST_D_FLAG]);
            dup = h != BEST_EMPTY && best_before_at(recs + RS_Q, RS_WORDS, h, i);
        }
        if (left || dup) recs[(size_t)RS_WORDS * i + RS_STATUS] = BEST_OUT;
        if (dup) status[i] = BBP_ROW_DUPLICATE;
    }
    const unsigned long long bl = __ballot(left), bd = __ballot(dup);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicAdd(&dctr[STAND_D_LEFT], (u32)__popcll(bl));
        if (bd) atomicAdd(&dctr[BEST_D_DUPLICATES], (u32)__popcll(bd));
    }
}

// One lane per entry slot: entry e of the new standing is working row order[e] -- key and id from the working arrays, the serial an
// entry's own or, for row j of the offer, offered + j.  Everything read is the call's scratch; only the standing's allocation is written.
__global__ void __launch_bounds__(BEST_T) k_stand_commit(u32 K, u32 B, const u32* __restrict__ whdr, const u32* __restrict__ order, const u32* __restrict__ win,
                                                         const u32* __restrict__ ids, const u32* __restrict__ wserial, u32* __restrict__ st_hdr,
                                                         u32* __restrict__ st_keys, u32* __restrict__ st_ids, u32* __restrict__ st_serials) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 count = whdr[STAND_H_COUNT] < K ? whdr[STAND_H_COUNT] : K;
    const unsigned long long offered = ((unsigned long long)whdr[STAND_H_OFFERED + 1] << 32) | whdr[STAND_H_OFFERED];
    if (e == 0) {
        const unsigned long long now = offered + B;
        st_hdr[STAND_H_COUNT] = count, st_hdr[STAND_H_LAST] = count == K ? K - 1 : 0;
        st_hdr[STAND_H_OFFERED] = (u32)now, st_hdr[STAND_H_OFFERED + 1] = (u32)(now >> 32);
        for (int w = 0; w < 8; w++) st_hdr[STAND_H_BAR + w] = whdr[STAND_H_BAR + w];
    }
    if (e >= count) return;
    const u32 i = order[e];
    if (i >= K + B) return;
    for (int w = 0; w < 8; w++) st_keys[8 * (size_t)e + w] = win[(size_t)RS_WORDS * i + RS_Q + w], st_ids[8 * (size_t)e + w] = ids[8 * (size_t)i + w];
    const unsigned long long serial = i < K ? ((unsigned long long)wserial[2 * (size_t)i + 1] << 32) | wserial[2 * (size_t)i] : offered + (i - K);
    st_serials[2 * (size_t)e] = (u32)serial, st_serials[2 * (size_t)e + 1] = (u32)(serial >> 32);
}
#endif

}  // namespace bbp
