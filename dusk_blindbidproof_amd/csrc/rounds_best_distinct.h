// Best proofs of many rounds, one per bidder (bbp_verify_rounds_best_distinct, its _dev form, bbp_debug_rounds_best_distinct): the
// one-per-bidder rules of round_best.h kept per round while every running round shares one step, as rounds_best.h keeps the plain
// rules.  The rules (include/bbp.h "Best proofs of many rounds, one per bidder") are stated once, in plain C++, by
// rounds_best_distinct_host -- round_best_distinct_host per round, indices mapped back, steps counted; the kernels at the bottom are held
// to it (tests/rounds_best_distinct_check.cpp on the host, tests/test_gpu_rounds_best_distinct.py on the device).  Segments, scan,
// select, gather, mark and pairs are rounds_best.h's and round_best.h's, unchanged; on top of them:
//   k_bests_ids      one lane per row: the 32 z_img bytes at any alignment -> id[i], 8 words
//   k_bests_settle   behind k_bests_mark: a step's OK rows enter the identity table; settled[round] counts the slots claimed from empty
//   k_bests_holders  a launch of its own behind it: the winner record of a step's OK row is open only when the row holds its identity
//   k_bests_drop     one lane per row: a live candidate whose identity is settled in ITS round leaves with BBP_ROW_DUPLICATE, unless
//                    its round has stopped; dups[round] counts it
//   k_bests_plan_distinct   one lane per round: take[r] from live = ncand - examined - dups, nothing once settled[r] >= K
// An identity is (round, 32 bytes): the round enters the hash and the equality test, so one z_img resent in every round is R
// identities on R probe chains.  ONE table per call, sized from B alone.
#pragma once
#include "rounds_best.h"

namespace bbp {

// (round, id) decides the slot: best_id_hash's FNV-1a with the round in front of the eight words, the same finaliser
BBP_HD u32 bests_id_hash(u32 round, const u32 id[8]) {
    u32 h = (0x811c9dc5u ^ round) * 0x01000193u;
    for (int w = 0; w < 8; w++) h = (h ^ id[w]) * 0x01000193u;
    h ^= h >> 15, h *= 0x2c1b3c6du, h ^= h >> 12, h *= 0x297a2d39u, h ^= h >> 15;
    return h;
}
// rows a and b carry one identity: the same round and the same 32 bytes
BBP_HD bool bests_id_equal(const u32* ids, const u32* round_of, u32 a, u32 round_b, const u32* id_b) {
    return round_of[a] == round_b && best_id_equal(ids + 8 * (size_t)a, id_b);
}
// best_table_insert with identities that belong to a round (round_of: one entry per row).  The holder order is best_before_at on the
// call's indices: within a round, ascending global index is ascending local index.  The same bounds: at most `slots` probe steps and
// `max_replace` exchanges; a bound that is reached raises its bit of *flag.
BBP_HD u32 bests_table_insert(u32* table, u32 mask, const u32* ids, const u32* round_of, const u32* keys, u32 kstride, u32 i, u32 max_replace, u32* flag) {
    const u32* id = ids + 8 * (size_t)i;
    const u32 rd = round_of[i];
    u32 p = bests_id_hash(rd, id) & mask;
    for (u32 step = 0; step <= mask; step++, p = best_probe_next(p, mask)) {
        u32 cur = best_cas(&table[p], BEST_EMPTY, i);
        if (cur == BEST_EMPTY) return 1;
        if (!bests_id_equal(ids, round_of, cur, rd, id)) continue;
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
// the holder of identity (round, id), or BEST_EMPTY: the walk ends at the first empty slot, after `slots` steps at the latest
BBP_HD u32 bests_table_find(const u32* table, u32 mask, const u32* ids, const u32* round_of, u32 round, const u32* id, u32* flag) {
    u32 p = bests_id_hash(round, id) & mask;
    for (u32 step = 0; step <= mask; step++, p = best_probe_next(p, mask)) {
        const u32 cur = table[p];
        if (cur == BEST_EMPTY) return BEST_EMPTY;
        if (bests_id_equal(ids, round_of, cur, round, id)) return cur;
    }
    best_flag_raise(flag, BEST_FLAG_PROBE);
    return BEST_EMPTY;
}

// the rows round r contributes to step t: nothing once it has stopped (K identities settled, or no live candidate left), else tranche
// t of its live candidates.  A round that runs has run every step so far, so the step is its tranche number.
BBP_HD u32 bests_take_distinct(u32 K, u32 tranche, u32 t, u32 n_candidates, u32 examined, u32 dups, u32 settled) {
    const unsigned long long gone = (unsigned long long)examined + dups;
    if (gone >= n_candidates || (K && settled >= K)) return 0;
    return best_tranche_rows(best_tranche0(K, tranche, n_candidates), t, n_candidates - (u32)gone);
}

// The rules.  As rounds_best_host, plus ids (B x 8 words) and n_duplicates (R entries).  Round r: round_best_distinct_host over its rows
// in ascending index -- identities never meet across rounds; n_steps (may be null): the most tranches any round ran.
inline void rounds_best_distinct_host(u32 R, u32 B, const u32* round_of, const u32* keys, const u32* ids, const int32_t* verdicts, const u32* floors, u32 K,
                                      u32 tranche, u32 cap, u32* best_out, u32* n_best, u32* n_candidates, u32* n_examined, u32* n_duplicates, u32* n_steps,
                                      int32_t* status) {
    std::vector<std::vector<u32>> rows(R);
    for (u32 i = 0; i < B; i++) rows[round_of ? round_of[i] : 0].push_back(i);
    u32 steps = 0;
    for (u32 r = 0; r < R; r++) {
        const u32 n = (u32)rows[r].size();
        std::vector<u32> k(8 * (size_t)n + 8), id(8 * (size_t)n + 8), best(cap);
        std::vector<int32_t> v(n), st(n);
        for (u32 j = 0; j < n; j++) {
            memcpy(&k[8 * (size_t)j], keys + 8 * (size_t)rows[r][j], 32);
            memcpy(&id[8 * (size_t)j], ids + 8 * (size_t)rows[r][j], 32);
            v[j] = verdicts[rows[r][j]];
        }
        u32 ran = 0;
        round_best_distinct_host(n, k.data(), id.data(), v.data(), floors + 8 * (size_t)r, K, tranche, cap, best.data(), &n_best[r], &n_candidates[r],
                                 &n_examined[r], &n_duplicates[r], st.data(), &ran);
        for (u32 j = 0; j < n; j++) status[rows[r][j]] = st[j];
        for (u32 j = 0; j < n_best[r] && j < cap; j++) best_out[(size_t)r * cap + j] = rows[r][best[j]];
        steps = ran > steps ? ran : steps;
    }
    if (n_steps) *n_steps = steps;
}

// The extra state of a many-rounds one-per-bidder call, behind the state BestsLayout(B, R, false) describes (same allocations: the
// context's best_dev and its pinned mirror).  dctr: 2 R + 1 words that one copy fetches -- per round settled and dups (word offsets
// d_*), then the flag word; the ids (8 words per row); the table; and -- the host forms -- the staged score || z_img bytes, 64 per row.
struct BestsDistinctLayout {
    u32 log2, slots;
    u32 d_settled, d_dups, d_flag, d_words;
    size_t dctr, ids, table, kid, bytes;
    size_t h_dctr, h_kid, h_bytes;
    BestsDistinctLayout(const BestsLayout& L, u32 B, u32 R, u32 table_log2, bool host_rows) {
        const size_t b = B;
        log2 = table_log2 ? table_log2 : best_table_log2(B);
        slots = 1u << log2;
        d_settled = 0, d_dups = R, d_flag = 2 * R, d_words = 2 * R + 1;
        dctr = L.bytes;
        ids = dctr + align256(4 * (size_t)d_words);
        table = ids + align256(32 * b);
        kid = table + align256(4 * (size_t)slots);
        bytes = kid + (host_rows ? align256(64 * b) : 0);
        h_dctr = L.h_bytes;
        h_kid = h_dctr + align256(4 * (size_t)d_words);
        h_bytes = h_kid + (host_rows ? align256(64 * b) : 0);
    }
};

#ifdef __HIPCC__
// ctr[rd] += the lanes of this wave that count.  A step's rows are grouped by round, so a wave mostly holds one round: where its
// lanes in range agree on the round (lane 0 is in range whenever any lane is: the lanes in range are a prefix) one addition per
// wave, else one per lane.  Every lane of the wave calls it.
__device__ inline void bests_wave_add(u32* ctr, u32 rd, bool in_range, bool counts) {
    const u32 rd0 = __shfl(rd, 0);
    const bool agree = __ballot(in_range && rd != rd0) == 0;
    const unsigned long long bc = __ballot(counts);
    if (agree) {
        if ((threadIdx.x & 63) == 0 && bc) atomicAdd(&ctr[rd0], (u32)__popcll(bc));
    } else if (counts)
        atomicAdd(&ctr[rd], 1u);
}

// k_bests_keys' sibling, launched in front of it.  id[i]: the 32 bytes behind the score, read byte by byte -- at base + rowoff[i] +
// rb[round] - 32 (the _dev form: z_img is a row's last field), or, rowoff null, at base + 64 i + 32 (the staged score || z_img rows).
// staged_off (the host forms; else null): staged_off[i] = 64 i, where the staged row of i starts -- with a row size of 64 for every
// round, k_bests_keys then reads the score of the same staged row, and no offsets are uploaded.
__global__ void __launch_bounds__(BEST_T) k_bests_ids(u32 B, const u8* __restrict__ base, const unsigned long long* __restrict__ rowoff,
                                                      const u32* __restrict__ rb, const u32* __restrict__ round_of, u32* __restrict__ ids,
                                                      unsigned long long* __restrict__ staged_off) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const u8* p = rowoff ? base + rowoff[i] + rb[round_of[i]] - 32 : base + 64 * (size_t)i + 32;
    u32* d = ids + 8 * (size_t)i;
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = rb_le32(p + 4 * w);
    if (staged_off) staged_off[i] = 64ull * i;
}

// Behind k_bests_mark, one lane per row of the step (n rows, grouped by round): an OK row enters the identity table
// (bests_table_insert: no lane waits for another; the loops are bounded by the table's size and by the step's).  settled[round] += the
// slots claimed from empty.  recs: the candidate records, whose keys order the rows.  A sel entry that is no row is passed over.
__global__ void __launch_bounds__(BEST_T) k_bests_settle(u32 n, u32 B, const u32* __restrict__ sel, const int32_t* __restrict__ tstat,
                                                         const u32* __restrict__ recs, const u32* __restrict__ ids, const u32* __restrict__ round_of, u32* table,
                                                         u32 mask, u32* settled, u32* flag) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 i = j < n ? sel[j] : B;
    const bool in_range = i < B;
    const u32 rd = in_range ? round_of[i] : 0;
    bool claimed = false;
    if (in_range && tstat[j] == BBP_OK) claimed = bests_table_insert(table, mask, ids, round_of, recs + RS_Q, RS_WORDS, i, n, flag) != 0;
    bests_wave_add(settled, rd, in_range, claimed);
}

// A launch of its own behind k_bests_settle (the table is final for this step), one lane per row of the step: the winner record of an
// OK row is open exactly when the row is its identity's holder.  Only the current step needs it: a later row never displaces a holder,
// because rows of a settled identity leave (k_bests_drop) before their round's next selection, and a stopped round selects no more.
__global__ void __launch_bounds__(BEST_T) k_bests_holders(u32 n, u32 B, const u32* __restrict__ sel, const int32_t* __restrict__ tstat,
                                                          const u32* __restrict__ ids, const u32* __restrict__ round_of, const u32* __restrict__ table,
                                                          u32 mask, u32* __restrict__ win, u32* flag) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || tstat[j] != BBP_OK) return;
    const u32 i = sel[j];
    if (i >= B) return;
    const bool holder = bests_table_find(table, mask, ids, round_of, round_of[i], ids + 8 * (size_t)i, flag) == i;
    win[(size_t)RS_WORDS * i + RS_STATUS] = holder ? (u32)BBP_OK : BEST_OUT;
}

// Behind k_bests_holders, one lane per row of the call.  A lane whose round has stopped (K > 0 identities settled in it -- written by an
// earlier launch) does nothing: no drop pass runs after a round's last tranche, whatever the other rounds do.  Otherwise a candidate
// record that is still a member and whose identity is settled in its round leaves with BBP_ROW_DUPLICATE; dups[round] counts it.
__global__ void __launch_bounds__(BEST_T) k_bests_drop(u32 B, u32 K, u32* __restrict__ recs, const u32* __restrict__ ids, const u32* __restrict__ round_of,
                                                       const u32* __restrict__ table, u32 mask, int32_t* __restrict__ status, const u32* __restrict__ settled,
                                                       u32* dups, u32* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = i < B;
    const u32 rd = in_range ? round_of[i] : 0;
    bool dup = false;
    if (in_range && !(K && settled[rd] >= K) && recs[(size_t)RS_WORDS * i + RS_STATUS] == (u32)BBP_OK) {
        dup = bests_table_find(table, mask, ids, round_of, rd, ids + 8 * (size_t)i, flag) != BEST_EMPTY;
        if (dup) status[i] = BBP_ROW_DUPLICATE, recs[(size_t)RS_WORDS * i + RS_STATUS] = BEST_OUT;
    }
    bests_wave_add(dups, rd, in_range, dup);
}

// k_bests_plan for the one-per-bidder calls, one lane per round.  finish == 0: take[r] = the rows round r contributes to step t
// (bests_take_distinct), and tranches[r] = t + 1 when it contributes; finish != 0: take[r] = the winners it reports, min(K, settled[r])
// or all of them.
__global__ void __launch_bounds__(BEST_T) k_bests_plan_distinct(u32 R, u32 t, u32 K, u32 tranche, u32 finish, const u32* __restrict__ ncand,
                                                                const u32* __restrict__ examined, const u32* __restrict__ dups,
                                                                const u32* __restrict__ settled, u32* __restrict__ take, u32* __restrict__ tranches) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (finish) {
        take[r] = bests_winners(K, settled[r]);
        return;
    }
    const u32 n = bests_take_distinct(K, tranche, t, ncand[r], examined[r], dups[r], settled[r]);
    take[r] = n;
    if (n) tranches[r] = t + 1;
}
#endif

}  // namespace bbp
