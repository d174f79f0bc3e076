// Best valid proofs of a round (bbp_verify_round_best, bbp_verify_round_best_dev, bbp_debug_round_best): sort a round's candidate proofs
// by their claimed score, verify from the top in tranches that double, stop at the K-th proof that holds.  The rules (include/bbp.h
// "Best valid proofs of a round") are stated once, in plain C++, by round_best_host; the kernels at the bottom are held to it
// (tests/round_best_check.cpp on the host, tests/test_gpu_round_best.py on the device):
//   k_best_keys     one lane per row: the 32 score bytes, screened against l and the floor -> a candidate record (RS_WORDS words, the
//                   record round_select.h's selection takes), a winner record that is not a member yet, the row's initial status
//   k_best_gather   the _dev form: row sel[j] and its entropy row -> packed row j, one workgroup per row, any source alignment
//   k_best_mark     a tranche's statuses scattered to status[sel[j]]; the row leaves the candidate records, an OK row enters the winners'
//   k_best_pairs    (key, index) of the selected winners, for the host to put in rank order
// The selection itself is round_select.h's, unchanged: over the candidate records with K = the tranche size, then once over the
// winners' records with the call's K.
// One per bidder (bbp_verify_round_best_distinct, its _dev form, bbp_debug_round_best_distinct): the same calls with at most one winner
// per z_img.  Rules: round_best_distinct_host (tests/round_best_distinct_check.cpp, tests/test_gpu_round_best_distinct.py); on top of
// the kernels above:
//   k_best_ids      one lane per row: the 32 z_img bytes -> id[i], 8 words
//   k_best_settle   a tranche's OK rows enter the identity table; per identity the first row in candidate order stays
//   k_best_holders  the winner record of a tranche's OK row is open only when the row holds its identity
//   k_best_drop     live candidates of a settled identity leave with BBP_ROW_DUPLICATE, unverified
#pragma once
#include <algorithm>
#include <vector>

#include "round_select.h"

namespace bbp {

// RS_STATUS of a record that is not (or no longer) a member of its array: rs_qualifies is false for it
constexpr u32 BEST_OUT = 0xffffffffu;
// what the host ranks: key (8 words), row index
constexpr u32 BEST_PAIR_WORDS = 9;

// Screening of one row by its key, in the header's order: BBP_ERR_FORMAT (key >= l: never verified), BBP_ROW_SKIPPED (below the
// floor), BBP_OK (a candidate).
BBP_HD int32_t best_screen_key(const u32* key, const u32* floor) {
    if (!sc_is_canonical(key)) return BBP_ERR_FORMAT;
    if (!rs_ge256(key, floor)) return BBP_ROW_SKIPPED;
    return BBP_OK;
}

// T_0 = max(tranche, K); tranche == 0: the default; K == 0: one tranche of every candidate
BBP_HD u32 best_tranche0(u32 K, u32 tranche, u32 n_candidates) {
    if (K == 0) return n_candidates;
    const u32 t = tranche ? tranche : BBP_BEST_TRANCHE_DEFAULT;
    return t > K ? t : K;
}
// tranche t: min(T_0 2^t, left) rows
BBP_HD u32 best_tranche_rows(u32 T0, u32 t, u32 left) {
    const unsigned long long T = t < 31 ? (unsigned long long)T0 << t : ~0ull;
    return T < left ? (u32)T : left;
}
// the most tranches a call runs: the least t with T_0 (2^t - 1) >= n_candidates, i.e. ceil(log2(n_candidates / T_0 + 1))
BBP_HD u32 best_max_tranches(u32 n_candidates, u32 T0) {
    u32 t = 0;
    for (unsigned long long seen = 0; seen < n_candidates; t++) seen += best_tranche_rows(T0, t, 0xffffffffu);
    return t;
}

// a comes before b in the candidate order: key descending, index ascending (keys: B x 8 words)
inline bool best_before(const u32* keys, u32 a, u32 b) {
    const int c = rs_cmp_top(keys + 8 * (size_t)a, keys + 8 * (size_t)b, 32);
    return c ? c > 0 : a < b;
}

// The rules.  keys: B x 8 words; verdicts: what verification says of row i (read for examined rows only); floor: 8 words; best_out:
// room for cap entries; status: B entries.
inline void round_best_host(u32 B, const u32* keys, const int32_t* verdicts, const u32* floor, u32 K, u32 tranche, u32 cap, u32* best_out, u32* n_best,
                            u32* n_candidates, u32* n_examined, int32_t* status) {
    std::vector<u32> cand, ok;
    for (u32 i = 0; i < B; i++) {
        const int32_t s = best_screen_key(keys + 8 * (size_t)i, floor);
        status[i] = s == BBP_ERR_FORMAT ? (int32_t)BBP_ERR_FORMAT : (int32_t)BBP_ROW_SKIPPED;
        if (s == BBP_OK) cand.push_back(i);
    }
    std::sort(cand.begin(), cand.end(), [&](u32 a, u32 b) { return best_before(keys, a, b); });
    const u32 nc = (u32)cand.size(), T0 = best_tranche0(K, tranche, nc);
    u32 at = 0;
    for (u32 t = 0; at < nc; t++) {
        const u32 n = best_tranche_rows(T0, t, nc - at);
        for (u32 j = at; j < at + n; j++) {
            status[cand[j]] = verdicts[cand[j]];
            if (verdicts[cand[j]] == BBP_OK) ok.push_back(cand[j]);
        }
        at += n;
        if (K && ok.size() >= K) break;
    }
    const u32 nb = K && ok.size() > K ? K : (u32)ok.size();
    for (u32 j = 0; j < nb && j < cap; j++) best_out[j] = ok[j];
    *n_best = nb, *n_candidates = nc, *n_examined = at;
}

// n (key, index) pairs in any order -> the first min(n, cap) indices in rank order
inline void best_rank_pairs(u32 n, const u32* pairs, u32 cap, u32* best_out) {
    std::vector<u32> order(n);
    for (u32 j = 0; j < n; j++) order[j] = j;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) {
        const u32 *pa = pairs + (size_t)BEST_PAIR_WORDS * a, *pb = pairs + (size_t)BEST_PAIR_WORDS * b;
        const int c = rs_cmp_top(pa, pb, 32);
        return c ? c > 0 : pa[8] < pb[8];
    });
    for (u32 j = 0; j < n && j < cap; j++) best_out[j] = pairs[(size_t)BEST_PAIR_WORDS * order[j] + 8];
}

// Where a call keeps its state: byte offsets (256-aligned) into the context's best_dev, and into its pinned mirror best_h.
//   device   ctr (examined, valid), counts (the selection's n_sel, n_qualified) with sel right behind it -- one copy fetches both --
//            the selection's state, keys (the host forms: the staged key bytes), candidate records, winner records, statuses, one
//            tranche's verdicts, the ranked pairs
//   pinned   keys going up, a tranche's verdicts going up, then what comes down: counts || sel, or at the end ctr, counts, pairs, statuses
struct BestLayout {
    size_t ctr, counts, sel, state, keys, recs, win, status, tstat, pairs, bytes;
    size_t h_keys, h_tstat, h_ctr, h_counts, h_sel, h_pairs, h_status, h_bytes;
    BestLayout(u32 B, bool host_keys) {
        const size_t b = B;
        ctr = 0;
        counts = 256;
        sel = 512;
        state = sel + align256(4 * b);
        keys = state + RS_STATE_BYTES;
        recs = keys + (host_keys ? align256(32 * b) : 0);
        win = recs + align256(4 * (size_t)RS_WORDS * b);
        status = win + align256(4 * (size_t)RS_WORDS * b);
        tstat = status + align256(4 * b);
        pairs = tstat + align256(4 * b);
        bytes = pairs + align256(4 * (size_t)BEST_PAIR_WORDS * b);
        h_keys = 0;
        h_tstat = host_keys ? align256(32 * b) : 0;
        h_ctr = h_tstat + align256(4 * b);
        h_counts = h_ctr + 256;
        h_sel = h_counts + 256;  // (counts || sel arrive in one copy: the same distance as on the device)
        h_pairs = h_sel + align256(4 * b);
        h_status = h_pairs + align256(4 * (size_t)BEST_PAIR_WORDS * b);
        h_bytes = h_status + align256(4 * b);
    }
};
// the _dev form's best_rows for a tranche of n rows of list length N: the packed rows, then their entropy rows
struct BestRows {
    size_t rows, ent, bytes;
    BestRows(u32 n, u32 N) {
        rows = 0;
        ent = align256(round_row_bytes(N) * (size_t)n);
        bytes = ent + align256(32 * (size_t)n);
    }
};

// ---- one per bidder (bbp_verify_round_best_distinct, its _dev form, bbp_debug_round_best_distinct; include/bbp.h "Best proofs of a
// round, one per bidder") --------------------------------------------------------------------------------------------------------------
// id[i] is the 32 raw z_img bytes of row i as 8 little-endian words; identities are compared as BYTES.  That is exact for every row that
// can settle an identity: the verifier refuses a row whose z_img is not canonical with BBP_ERR_FORMAT (k_vparse, verifier_mixed.inc: the
// parse of the row's scalars sets the format bit for any of them >= l) and so never reports BBP_OK for it; among canonical encodings
// equal values are equal bytes.  tests/test_gpu_round_best_distinct.py holds it end to end (a row carrying z_img + l).
//
// The identity table: open addressing over row indices, 2^s slots, empty = BEST_EMPTY, linear probing that wraps.  A slot, once claimed,
// keeps its identity for the rest of the call and holds the identity's holder so far: the first OK row in candidate order among those
// inserted.  Hash, probe step, compare, insert and lookup are BBP_HD, so the host runs what the kernels run; only the compare-and-swap
// differs (best_cas).  Every loop is bounded; a bound that is reached raises a bit of the flag word and the call ends BBP_ERR_INTERNAL.
constexpr u32 BEST_EMPTY = 0xffffffffu;
constexpr u32 BEST_TABLE_LOG2_MAX = 21;  // 2^21 slots >= 2 BBP_SELECT_MAX_BIDS: 8 MB
enum : u32 { BEST_FLAG_PROBE = 1, BEST_FLAG_REPLACE = 2 };
// the extra counters of a call, one word each (word 3 is round_standing.h's: zero in every other call)
enum : u32 { BEST_D_SETTLED = 0, BEST_D_DUPLICATES = 1, BEST_D_FLAG = 2, BEST_D_WORDS = 4 };

// the least s with 2^s >= 2 B: sized from B alone
BBP_HD u32 best_table_log2(u32 B) {
    u32 s = 1;
    while (s < BEST_TABLE_LOG2_MAX && (1ull << s) < 2ull * B) s++;
    return s;
}
// all eight words decide the slot (FNV-1a over the words, then a finaliser that brings the high bits down: the slot is the low bits)
BBP_HD u32 best_id_hash(const u32 id[8]) {
    u32 h = 0x811c9dc5u;
    for (int w = 0; w < 8; w++) h = (h ^ id[w]) * 0x01000193u;
    h ^= h >> 15, h *= 0x2c1b3c6du, h ^= h >> 12, h *= 0x297a2d39u, h ^= h >> 15;
    return h;
}
BBP_HD u32 best_probe_next(u32 p, u32 mask) { return (p + 1) & mask; }
BBP_HD bool best_id_equal(const u32* a, const u32* b) {
    u32 d = 0;
    for (int w = 0; w < 8; w++) d |= a[w] ^ b[w];
    return d == 0;
}
// a before b in the candidate order, keys at any stride (B x 8 words: stride 8; the selection's records: RS_WORDS, from RS_Q)
BBP_HD bool best_before_at(const u32* keys, u32 stride, u32 a, u32 b) {
    const int c = rs_cmp_top(keys + (size_t)stride * a, keys + (size_t)stride * b, 32);
    return c ? c > 0 : a < b;
}
// *p == expect ? (*p = v, expect) : *p -- atomic on the device, plain on the host (which runs its rows one after the other)
BBP_HD u32 best_cas(u32* p, u32 expect, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const u32 old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
BBP_HD void best_flag_raise(u32* flag, u32 bit) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(flag, bit);
#else
    *flag |= bit;
#endif
}

// Row i (OK) enters the table.  Returns 1 when it claimed an empty slot (a new identity is settled), else 0.  At a slot of its own identity
// the row that comes first in candidate order stays: the holder is a minimum under a total order, whichever insert ran first.  At most
// `slots` probe steps and `max_replace` exchanges (each failed exchange means another row of the identity, earlier in the order, got in).
BBP_HD u32 best_table_insert(u32* table, u32 mask, const u32* ids, const u32* keys, u32 kstride, u32 i, u32 max_replace, u32* flag) {
    const u32* id = ids + 8 * (size_t)i;
    u32 p = best_id_hash(id) & mask;
    for (u32 step = 0; step <= mask; step++, p = best_probe_next(p, mask)) {
        u32 cur = best_cas(&table[p], BEST_EMPTY, i);
        if (cur == BEST_EMPTY) return 1;
        if (!best_id_equal(ids + 8 * (size_t)cur, id)) continue;
        for (u32 r = 0; r <= max_replace; r++) {
            if (!best_before_at(keys, kstride, i, cur)) return 0;
            const u32 old = best_cas(&table[p], cur, i);
            if (old == cur) return 0;
            cur = old;  // (a slot keeps its identity: still a row of this one)
        }
        best_flag_raise(flag, BEST_FLAG_REPLACE);
        return 0;
    }
    best_flag_raise(flag, BEST_FLAG_PROBE);
    return 0;
}
// the holder of identity `id`, or BEST_EMPTY: the walk ends at the first empty slot, after `slots` steps at the latest
BBP_HD u32 best_table_find(const u32* table, u32 mask, const u32* ids, const u32* id, u32* flag) {
    u32 p = best_id_hash(id) & mask;
    for (u32 step = 0; step <= mask; step++, p = best_probe_next(p, mask)) {
        const u32 cur = table[p];
        if (cur == BEST_EMPTY) return BEST_EMPTY;
        if (best_id_equal(ids + 8 * (size_t)cur, id)) return cur;
    }
    best_flag_raise(flag, BEST_FLAG_PROBE);
    return BEST_EMPTY;
}

// The rules, one per bidder.  As round_best_host, plus ids (B x 8 words) and n_duplicates.  An identity is settled once a row carrying it
// has verified OK; its holder is the first such row in candidate order.  Tranche t is the next min(T_t, live) live candidates; all are
// verified and keep their true status.  Stop after the first tranche that leaves >= K identities settled (K > 0) or when no live
// candidate is left; otherwise every live candidate of a settled identity becomes BBP_ROW_DUPLICATE and leaves, before the next tranche.
// n_tranches (may be null): the tranches that ran, counted.
inline void round_best_distinct_host(u32 B, const u32* keys, const u32* ids, const int32_t* verdicts, const u32* floor, u32 K, u32 tranche, u32 cap,
                                     u32* best_out, u32* n_best, u32* n_candidates, u32* n_examined, u32* n_duplicates, int32_t* status,
                                     u32* n_tranches = nullptr) {
    std::vector<u32> live, holders;
    for (u32 i = 0; i < B; i++) {
        const int32_t s = best_screen_key(keys + 8 * (size_t)i, floor);
        status[i] = s == BBP_ERR_FORMAT ? (int32_t)BBP_ERR_FORMAT : (int32_t)BBP_ROW_SKIPPED;
        if (s == BBP_OK) live.push_back(i);
    }
    std::sort(live.begin(), live.end(), [&](u32 a, u32 b) { return best_before(keys, a, b); });
    auto settled = [&](u32 i) {
        for (u32 h : holders)
            if (best_id_equal(ids + 8 * (size_t)h, ids + 8 * (size_t)i)) return true;
        return false;
    };
    const u32 nc = (u32)live.size(), T0 = best_tranche0(K, tranche, nc);
    u32 examined = 0, dups = 0, ran = 0;
    for (u32 t = 0; !live.empty(); t++) {
        const u32 n = best_tranche_rows(T0, t, (u32)live.size());
        ran = t + 1;
        for (u32 j = 0; j < n; j++) {
            const u32 i = live[j];
            status[i] = verdicts[i];
            if (verdicts[i] == BBP_OK && !settled(i)) holders.push_back(i);  // (candidate order: the first OK row of an identity)
        }
        live.erase(live.begin(), live.begin() + n);
        examined += n;
        if (K && holders.size() >= K) break;
        std::vector<u32> keep;
        for (u32 i : live) {
            if (settled(i))
                status[i] = BBP_ROW_DUPLICATE, dups++;
            else
                keep.push_back(i);
        }
        live.swap(keep);
    }
    const u32 nb = K && holders.size() > K ? K : (u32)holders.size();
    for (u32 j = 0; j < nb && j < cap; j++) best_out[j] = holders[j];
    *n_best = nb, *n_candidates = nc, *n_examined = examined, *n_duplicates = dups;
    if (n_tranches) *n_tranches = ran;
}

// The extra state of a one-per-bidder call, behind the state BestLayout(B, false) describes (same allocations: the context's best_dev and
// its pinned mirror): the three counters, the ids, the table, and -- the host forms -- the staged score || z_img bytes, 64 per row.
struct BestDistinctLayout {
    u32 log2, slots;
    size_t dctr, ids, table, kid, bytes;
    size_t h_dctr, h_kid, h_bytes;
    BestDistinctLayout(const BestLayout& L, u32 B, u32 table_log2, bool host_rows) {
        const size_t b = B;
        log2 = table_log2 ? table_log2 : best_table_log2(B);
        slots = 1u << log2;
        dctr = L.bytes;
        ids = dctr + 256;
        table = ids + align256(32 * b);
        kid = table + align256(4 * (size_t)slots);
        bytes = kid + (host_rows ? align256(64 * b) : 0);
        h_dctr = L.h_bytes;
        h_kid = h_dctr + 256;
        h_bytes = h_kid + (host_rows ? align256(64 * b) : 0);
    }
};

constexpr u32 BEST_T = 64, BEST_GATHER_T = 256;  // workgroup sizes: the per-row kernels (rounds_best.h's too), the two gathers

#if defined(__HIPCC__) && defined(BBP_ROUND_BEST_KERNELS)  // the kernels: compiled by the one unit that launches them (capi.h)
// One lane per row, 64-lane workgroups.  The key is read byte by byte at base + i stride + off: the _dev form's stride 1313 + 32 N is
// odd, so every alignment occurs (the host forms: stride 32, offset 0).  Writes the candidate record (BBP_OK for a candidate), the
// winner record (not a member yet) and the row's initial status: BBP_ERR_FORMAT for a key >= l, BBP_ROW_SKIPPED for every other row.
__global__ void __launch_bounds__(BEST_T) k_best_keys(u32 B, const u8* __restrict__ base, size_t stride, size_t off, RsFloor floor, u32* __restrict__ recs,
                                                      u32* __restrict__ win, int32_t* __restrict__ status) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const u8* p = base + stride * (size_t)i + off;
    u32 k[8];
#pragma unroll
    for (int w = 0; w < 8; w++) k[w] = rb_le32(p + 4 * w);
    const int32_t s = best_screen_key(k, floor.w);
    u32 *r = recs + (size_t)RS_WORDS * i, *v = win + (size_t)RS_WORDS * i;
#pragma unroll
    for (int w = 0; w < 8; w++) r[RS_Q + w] = k[w], v[RS_Q + w] = k[w];
    r[RS_STATUS] = s == BBP_OK ? (u32)BBP_OK : BEST_OUT, r[RS_TOGGLE] = 0;
    v[RS_STATUS] = BEST_OUT, v[RS_TOGGLE] = 0;
    status[i] = s == BBP_ERR_FORMAT ? (int32_t)BBP_ERR_FORMAT : (int32_t)BBP_ROW_SKIPPED;
}

// One workgroup per row of a tranche, or of the part of it that starts at row `first` (a tranche is verified in engine calls of at
// most BBP_HOST_CHUNK_VERIFY rows, as a host-pointer call is): row sel[first + j] of `rows` (rb bytes each, any alignment) -> packed row
// j of out_rows, its 32 entropy bytes -> row j of out_ent.  Aligned 32-bit stores; a stored word is put together from the two aligned source words that hold
// it, or -- where those would reach outside the source row -- from its four bytes, so nothing outside [row, row + rb) is read.
// Workgroups at or beyond the device-side count leave at once.
__global__ void __launch_bounds__(BEST_GATHER_T) k_best_gather(u32 rb, u32 first, const u32* __restrict__ sel, const u32* __restrict__ counts,
                                                               const u8* __restrict__ rows, const u8* __restrict__ ent, u8* __restrict__ out_rows,
                                                               u8* __restrict__ out_ent) {
    const u32 j = blockIdx.x, tid = threadIdx.x;  // packed row j is row first + j of the tranche
    if (first + j >= counts[0]) return;
    const u32 i = sel[first + j];
    const u8* s = rows + (size_t)rb * i;
    u8* d = out_rows + (size_t)rb * j;
    if (tid < 32) out_ent[32 * (size_t)j + tid] = ent[32 * (size_t)i + tid];
    u32 head = (u32)(-(uintptr_t)d & 3);  // bytes in front of the first aligned word of the destination
    head = head < rb ? head : rb;
    if (tid < head) d[tid] = s[tid];
    const u32 nd = (rb - head) / 4, sh = (u32)((uintptr_t)(s + head) & 3);
    const u32* sw = (const u32*)(s + head - sh);  // aligned: words k and k + 1 hold source bytes [4k - sh, 4k - sh + 8) of the body
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

// One lane per row of the tranche (n: the launch's size, counts[0]: the rows it holds).  status[sel[j]] = tstat[j]; the row leaves the
// candidate records; an OK row enters the winners'; ctr += (rows examined, rows OK), one addition per wave.
__global__ void __launch_bounds__(BEST_T) k_best_mark(u32 n, const u32* __restrict__ sel, const u32* __restrict__ counts, const int32_t* __restrict__ tstat,
                                                      int32_t* __restrict__ status, u32* __restrict__ recs, u32* __restrict__ win, u32* __restrict__ ctr) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < n && j < counts[0];
    bool ok = false;
    if (live) {
        const u32 i = sel[j];
        const int32_t st = tstat[j];
        status[i] = st;
        recs[(size_t)RS_WORDS * i + RS_STATUS] = BEST_OUT;
        ok = st == BBP_OK;
        if (ok) win[(size_t)RS_WORDS * i + RS_STATUS] = (u32)BBP_OK;
    }
    const unsigned long long bl = __ballot(live), bo = __ballot(ok);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicAdd(&ctr[0], (u32)__popcll(bl));
        if (bo) atomicAdd(&ctr[1], (u32)__popcll(bo));
    }
}

// pair j < min(counts[0], cap): the key and the index of winner sel[j]
__global__ void __launch_bounds__(BEST_T) k_best_pairs(u32 cap, const u32* __restrict__ sel, const u32* __restrict__ counts, const u32* __restrict__ win,
                                                       u32* __restrict__ pairs) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cap || j >= counts[0]) return;
    const u32 i = sel[j];
    const u32* v = win + (size_t)RS_WORDS * i;
    u32* p = pairs + (size_t)BEST_PAIR_WORDS * j;
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = v[RS_Q + w];
    p[8] = i;
}

// ---- one per bidder ------------------------------------------------------------------------------------------------------------------
// k_best_keys' sibling, launched beside it: id[i], the 32 bytes at base + i stride + off read byte by byte (any alignment), as 8 words.
__global__ void __launch_bounds__(BEST_T) k_best_ids(u32 B, const u8* __restrict__ base, size_t stride, size_t off, u32* __restrict__ ids) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const u8* p = base + stride * (size_t)i + off;
    u32* d = ids + 8 * (size_t)i;
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = rb_le32(p + 4 * w);
}

// After a tranche's mark, one lane per row of the tranche: an OK row enters the identity table (best_table_insert: no lane waits for
// another; the loops are bounded by the table's size and by the tranche's).  dctr[BEST_D_SETTLED] += the slots claimed from empty, one
// addition per wave.  recs: the candidate records, whose keys order the rows.
__global__ void __launch_bounds__(BEST_T) k_best_settle(u32 n, const u32* __restrict__ sel, const u32* __restrict__ counts, const int32_t* __restrict__ tstat,
                                                        const u32* __restrict__ recs, const u32* __restrict__ ids, u32* table, u32 mask, u32* dctr) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (j < n && j < counts[0] && tstat[j] == BBP_OK)
        claimed = best_table_insert(table, mask, ids, recs + RS_Q, RS_WORDS, sel[j], n, &dctr[BEST_D_FLAG]) != 0;
    const unsigned long long bc = __ballot(claimed);
    if ((threadIdx.x & 63) == 0 && bc) atomicAdd(&dctr[BEST_D_SETTLED], (u32)__popcll(bc));
}

// A launch of its own behind k_best_settle (the table is final for this tranche), one lane per row of the tranche: the winner record of
// an OK row is open exactly when the row is its identity's holder.  Only the current tranche needs it: a later row never displaces a
// holder, because rows of a settled identity leave (k_best_drop) before the next selection.
__global__ void __launch_bounds__(BEST_T) k_best_holders(u32 n, const u32* __restrict__ sel, const u32* __restrict__ counts, const int32_t* __restrict__ tstat,
                                                         const u32* __restrict__ ids, const u32* __restrict__ table, u32 mask, u32* __restrict__ win, u32* dctr) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || j >= counts[0] || tstat[j] != BBP_OK) return;
    const u32 i = sel[j];
    const bool holder = best_table_find(table, mask, ids, ids + 8 * (size_t)i, &dctr[BEST_D_FLAG]) == i;
    win[(size_t)RS_WORDS * i + RS_STATUS] = holder ? (u32)BBP_OK : BEST_OUT;
}

// Before each further selection, one lane per row: a candidate record that is still a member and whose identity is settled leaves with
// BBP_ROW_DUPLICATE; dctr[BEST_D_DUPLICATES] += those rows, one addition per wave.  Enqueued behind k_best_holders, before the host has
// read the count of settled identities: when the call stops here (K > 0 identities settled -- written by an earlier launch, every lane
// reads the same) the launch does nothing, so no drop pass runs after the last tranche.
__global__ void __launch_bounds__(BEST_T) k_best_drop(u32 B, u32 K, u32* __restrict__ recs, const u32* __restrict__ ids, const u32* __restrict__ table, u32 mask,
                                                      int32_t* __restrict__ status, u32* dctr) {
    if (K && dctr[BEST_D_SETTLED] >= K) return;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool dup = false;
    if (i < B && recs[(size_t)RS_WORDS * i + RS_STATUS] == (u32)BBP_OK) {
        dup = best_table_find(table, mask, ids, ids + 8 * (size_t)i, &dctr[BEST_D_FLAG]) != BEST_EMPTY;
        if (dup) status[i] = BBP_ROW_DUPLICATE, recs[(size_t)RS_WORDS * i + RS_STATUS] = BEST_OUT;
    }
    const unsigned long long bd = __ballot(dup);
    if ((threadIdx.x & 63) == 0 && bd) atomicAdd(&dctr[BEST_D_DUPLICATES], (u32)__popcll(bd));
}
#endif

}  // namespace bbp
