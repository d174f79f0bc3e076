// C-ABI, best proofs of ONE round: the plain and the one-per-bidder calls with their hooks and _dev forms, and standings -- see
// include/bbp.h.  What the many-rounds calls (capi_bests.hip) run of this unit is declared in capi.h.
#define BBP_ROUND_BEST_KERNELS  // the kernels of round_best.h are compiled here, round_standing.h's with them (capi.h)
#include <string.h>

#include <algorithm>
#include <optional>

#include "capi.h"
#include "round_best.h"
#include "round_standing.h"

using namespace bbp;

// ---- best valid proofs of a round (include/bbp.h; rules and kernels: round_best.h) ----------------------------------------------------
// The launch sequence of one call, on ONE device's context and one stream (context lock held by every step).  [..]: what the
// one-per-bidder calls add -- the same calls, plus an identity table (BestDistinctLayout behind BestLayout(B, false), same allocations):
//   open      the state reserved, ctr [and dctr] zeroed [the table emptied]
//   keys      k_best_keys: records, winners' records, initial statuses [k_best_ids]
//   per tranche   select (the candidates' records, K = the tranche's size; 0: all) -> counts, sel;  [the rows verified];  mark
//                 [k_best_settle, k_best_holders, k_best_drop (which does nothing once the call stops), then ctr and dctr into the
//                 mirror: settled identities and dropped rows decide the next tranche]
//   finish    select (the winners' records, the call's K), k_best_pairs, then ctr, counts and pairs [and dctr] into the pinned mirror
struct BestCall {
    bbp_ctx* ctx;
    u32 B, K;
    hipStream_t s;
    BestLayout L;
    std::optional<BestDistinctLayout> D;  // one per bidder only
    struct StandCall* stand = nullptr;    // an offer to a standing only (below): B is K + the offer's rows, the working rows
    u8 *d = nullptr, *h = nullptr;
    // host_rows: a host form, which stages bytes of every row -- the 32 key bytes (in L), one per bidder score || z_img (in D)
    BestCall(bbp_ctx* c, u32 B_, u32 K_, hipStream_t s_, bool host_rows, bool distinct, u32 table_log2 = 0)
        : ctx(c), B(B_), K(K_), s(s_), L(B_, host_rows && !distinct) {
        if (distinct) D.emplace(L, B_, table_log2, host_rows);
    }
    u32* at(size_t off) const { return (u32*)(d + off); }
    u32 mask() const { return D->slots - 1; }
    size_t bytes() const;
    size_t h_bytes() const;
    u32 first() const;  // the working rows in front of the call's own: a standing's K entry slots, otherwise none
    size_t staged_row() const { return D ? 64 : 32; }
    size_t staged() const { return D ? D->kid : L.keys; }
    size_t h_staged() const { return D ? D->h_kid : L.h_keys; }
    std::string family() const { return stand ? "standing of a round: " : D ? "best proofs, one per bidder: " : "best valid proofs: "; }
};
// What an offer to a standing adds to a one-per-bidder call (round_standing.h): the standing's own allocation and the host's record of
// it, the scratch behind the call's, and the launches between the family's.
struct StandCall {
    bbp_ctx::Standing* meta;
    u8* st;        // the standing's allocation
    u32 K, rows;   // rows: the offer's
    StandingLayout SL;
    StandingWork W;
    u32 merges = 0;
    StandCall(bbp_ctx::Standing* m, u8* st_, u32 rows_, const BestDistinctLayout& D) : meta(m), st(st_), K(m->K), rows(rows_), SL(m->K), W(D, m->K) {}
};
size_t BestCall::bytes() const { return stand ? stand->W.bytes : D ? D->bytes : L.bytes; }
size_t BestCall::h_bytes() const { return stand ? stand->W.h_bytes : D ? D->h_bytes : L.h_bytes; }
u32 BestCall::first() const { return stand ? stand->K : 0; }
static const RsFloor BEST_NO_FLOOR = {};  // k_best_keys has applied the floor: a record is a member by its status alone

static int32_t best_open(BestCall& c) {
    bbp_ctx* ctx = c.ctx;
    int32_t rc;
    if ((rc = dev_reserve(ctx, ctx->best_dev, c.bytes())) || (rc = pinned_reserve(ctx, ctx->best_h, ctx->best_h_cap, c.h_bytes()))) return rc;
    if (!ctx->ev_best) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_best, hipEventDisableTiming));
    c.d = (u8*)ctx->best_dev.p, c.h = (u8*)ctx->best_h;
    BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + c.L.ctr, 0, 16, c.s));
    if (c.D) {
        BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + c.D->dctr, 0, 16, c.s));
        BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + c.D->table, 0xff, 4 * (size_t)c.D->slots, c.s));
    }
    return BBP_OK;
}

// keys at base + i stride + off (device memory) [ids 32 bytes behind them: score || z_img are adjacent in a row], status: B x int32
// (device memory)
static int32_t best_keys_enqueue(const BestCall& c, const u8* base, size_t stride, size_t off, const uint8_t* floor32, int32_t* status) {
    const u32 f = c.first(), n = c.B - f;  // (an offer to a standing: base is the offer's row 0, which is working row f)
    const dim3 grid((n + BEST_T - 1) / BEST_T), block(BEST_T);
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_best_keys, grid, block, 0, c.s, n, base, stride, off, rs_floor_load(floor32), c.at(c.L.recs) + (size_t)RS_WORDS * f,
                           c.at(c.L.win) + (size_t)RS_WORDS * f, status + f);
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (!c.D) return BBP_OK;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_best_ids, grid, block, 0, c.s, n, base, stride, off + 32, c.at(c.D->ids) + 8 * (size_t)f);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// the next `rows` candidates in the candidate order (0: every one that is left) -> counts, sel
static int32_t best_select_enqueue(const BestCall& c, u32 rows) {
    return select_kernels_enqueue(c.ctx, c.B, c.at(c.L.recs), BEST_NO_FLOOR, rows, rows ? rows : c.B, c.at(c.L.sel), c.at(c.L.counts), c.d + c.L.state, c.s);
}

// the tranche in sel (n rows) has the statuses at tstat (device memory)
static int32_t best_mark_enqueue(const BestCall& c, u32 n, const int32_t* tstat, int32_t* status) {
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_best_mark, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, n, (const u32*)c.at(c.L.sel), (const u32*)c.at(c.L.counts), tstat, status,
                       c.at(c.L.recs), c.at(c.L.win), c.at(c.L.ctr));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// An offer to a standing, on c.s.  Seed: behind best_open, before the keys.  Leave: the leave pass.  Merge: behind a tranche's holders --
// displaced entries closed, the selection over the winner records with the call's K, the merge, then the leave pass unless no live
// candidate is left.  Finish: everything the host reads into the mirror.  Commit: a submission of its own, after the host's checks.
static int32_t stand_seed_enqueue(const BestCall& c, int32_t* status) {
    const StandCall& S = *c.stand;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stand_seed, dim3((S.K + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.K, (const u32*)(S.st + S.SL.hdr), (const u32*)(S.st + S.SL.keys),
                       (const u32*)(S.st + S.SL.ids), (const u32*)(S.st + S.SL.serials), c.at(c.L.recs), c.at(c.L.win), c.at(c.D->ids), status,
                       c.at(c.D->table), c.mask(), c.at(S.W.whdr), c.at(S.W.wserial), c.at(S.W.order), c.at(c.D->dctr));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t stand_leave_enqueue(const BestCall& c, int32_t* status) {
    const StandCall& S = *c.stand;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stand_leave, dim3((c.B + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.B, S.K, c.at(c.L.recs), (const u32*)c.at(c.D->ids),
                       (const u32*)c.at(c.D->table), c.mask(), (const u32*)c.at(S.W.whdr), status, c.at(c.D->dctr));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t stand_merge_enqueue(const BestCall& c, int32_t* status, bool leave) {
    StandCall& S = *c.stand;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_stand_displace, dim3((S.K + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.K, (const u32*)c.at(c.D->ids),
                           (const u32*)c.at(c.D->table), c.mask(), c.at(c.L.win), c.at(c.D->dctr));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (int32_t rc = select_kernels_enqueue(c.ctx, c.B, c.at(c.L.win), BEST_NO_FLOOR, S.K, S.K, c.at(c.L.sel), c.at(c.L.counts), c.d + c.L.state, c.s)) return rc;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        const u32 trip = S.meta->trip && S.meta->trip == ++S.merges;  // (bbp_debug_standing_trip: once)
        if (trip) S.meta->trip = 0;
        hipLaunchKernelGGL(k_stand_merge, dim3(1), dim3(STAND_MERGE_T), 0, c.s, S.K, (const u32*)c.at(c.L.sel), (const u32*)c.at(c.L.counts),
                           (const u32*)c.at(c.L.win), c.at(S.W.whdr), c.at(S.W.order), trip, c.at(c.D->dctr));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    return leave ? stand_leave_enqueue(c, status) : (int32_t)BBP_OK;
}
static int32_t stand_finish_enqueue(const BestCall& c, const int32_t* status) {
    bbp_ctx* ctx = c.ctx;
    const StandCall& S = *c.stand;
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_ctr, c.d + c.L.ctr, 8, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * BEST_D_WORDS, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + S.W.h_whdr, c.d + S.W.whdr, 4 * STAND_H_WORDS, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + S.W.h_order, c.d + S.W.order, 4 * (size_t)S.K, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_status, status + S.K, 4 * (size_t)S.rows, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}
static int32_t stand_commit_enqueue(const BestCall& c) {
    const StandCall& S = *c.stand;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stand_commit, dim3((S.K + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.K, S.rows, (const u32*)c.at(S.W.whdr),
                       (const u32*)c.at(S.W.order), (const u32*)c.at(c.L.win), (const u32*)c.at(c.D->ids), (const u32*)c.at(S.W.wserial),
                       (u32*)(S.st + S.SL.hdr), (u32*)(S.st + S.SL.keys), (u32*)(S.st + S.SL.ids), (u32*)(S.st + S.SL.serials));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// Behind the mark of a tranche of n rows, for a caller that decides from the device's counters whether another tranche runs: ctr into
// the mirror.  [Before that: identities settled, holders' winner records opened, duplicates dropped unless the call stops here (`drop`:
// false when the host knows that no live candidate is left); dctr into the mirror as well.]
static int32_t best_counters_enqueue(const BestCall& c, u32 n, const int32_t* tstat, int32_t* status, bool drop) {
    bbp_ctx* ctx = c.ctx;
    if (c.D) {
        const u32 *sel = c.at(c.L.sel), *counts = c.at(c.L.counts), *ids = c.at(c.D->ids);
        u32 *table = c.at(c.D->table), *dctr = c.at(c.D->dctr);
        ScopedEvent ev(ctx, TAG_SELECT, c.s);
        const dim3 grid((n + BEST_T - 1) / BEST_T), block(BEST_T);
        hipLaunchKernelGGL(k_best_settle, grid, block, 0, c.s, n, sel, counts, tstat, (const u32*)c.at(c.L.recs), ids, table, c.mask(), dctr);
        BBP_HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_best_holders, grid, block, 0, c.s, n, sel, counts, tstat, ids, (const u32*)table, c.mask(), c.at(c.L.win), dctr);
        BBP_HIP_TRY(ctx, hipGetLastError());
        if (c.stand) {  // (an offer to a standing: the merge, and the leave pass in the drop pass's place)
            if (int32_t rc = stand_merge_enqueue(c, status, drop)) return rc;
        } else if (drop) {
            hipLaunchKernelGGL(k_best_drop, dim3((c.B + BEST_T - 1) / BEST_T), block, 0, c.s, c.B, c.K, c.at(c.L.recs), ids, (const u32*)table, c.mask(), status,
                               dctr);
            BBP_HIP_TRY(ctx, hipGetLastError());
        }
    }
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_ctr, c.d + c.L.ctr, 8, hipMemcpyDeviceToHost, c.s));
    if (c.D) BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * BEST_D_WORDS, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}

// What a call knows between tranches, and the checks that hold it to the device's counters.  reached: the rows found valid [the
// identities settled]; dups: [the rows dropped as duplicates] 0.
struct BestTally {
    u32 T0 = 0, nc = 0, examined = 0, reached = 0, dups = 0, left = 0;  // left: an offer to a standing -- candidates that left by the bar
    u32 live() const { return nc - examined - dups - left; }
    // an offer to a standing, before tranche 0: the leave pass that ran in front of the first selection (the candidate count follows)
    bool pre(const BestCall& c, std::string* why) {
        u32 d[BEST_D_WORDS];
        memcpy(d, c.h + c.D->h_dctr, sizeof d);
        if (d[BEST_D_FLAG]) return *why = c.family() + "a bounded loop of the identity table ran out (flag " + std::to_string(d[BEST_D_FLAG]) + ")", false;
        dups = d[BEST_D_DUPLICATES], left = d[STAND_D_LEFT];
        return true;
    }
    bool stop(u32 K) const { return live() == 0 || (K && reached >= K); }
    // the counters that arrived behind a tranche's mark, or with the finish: false (with *why) when they are not what the call counted
    bool take(const BestCall& c, std::string* why) {
        u32 ctr[2], d[BEST_D_WORDS] = {};
        memcpy(ctr, c.h + c.L.h_ctr, 8);
        if (c.D)
            memcpy(d, c.h + c.D->h_dctr, sizeof d);
        else
            d[BEST_D_SETTLED] = ctr[1];  // every valid row counts
        if (d[BEST_D_FLAG]) return *why = c.family() + "a bounded loop of the identity table ran out (flag " + std::to_string(d[BEST_D_FLAG]) + ")", false;
        if (ctr[0] != examined || d[BEST_D_SETTLED] < reached || d[BEST_D_SETTLED] > ctr[1] || d[BEST_D_DUPLICATES] < dups || d[STAND_D_LEFT] < left ||
            (unsigned long long)examined + d[BEST_D_DUPLICATES] + d[STAND_D_LEFT] > nc)
            return *why = c.family() + "the device counted " + std::to_string(ctr[0]) + " rows examined, " + std::to_string(ctr[1]) + " valid, " +
                          std::to_string(d[BEST_D_SETTLED]) + " reached and " + std::to_string(d[BEST_D_DUPLICATES]) + " rows dropped; the call examined " +
                          std::to_string(examined) + " of " + std::to_string(nc) + " candidates and had reached " + std::to_string(reached),
                   false;
        reached = d[BEST_D_SETTLED], dups = d[BEST_D_DUPLICATES], left = d[STAND_D_LEFT];
        return true;
    }
};
// the rows to ask tranche t's selection for.  Tranche 0: its size needs the candidate count, which that selection delivers (0: every
// candidate); a later one: the host knows it
static u32 best_tranche_ask(u32 K, u32 tranche, u32 B, const BestTally& ty, u32 t) {
    return t == 0 ? (K ? std::min(best_tranche0(K, tranche, 0), B) : 0u) : best_tranche_rows(ty.T0, t, ty.live());
}
// counts = {n, live} of the selection of tranche t against the call's tally
static bool best_tranche_ok(const u32* counts, u32 t, u32 K, u32 tranche, BestTally& ty) {
    if (t == 0) ty.nc = counts[1] + ty.dups + ty.left, ty.T0 = best_tranche0(K, tranche, ty.nc);
    return counts[1] == ty.live() && counts[0] == best_tranche_rows(ty.T0, t, counts[1]);
}

int32_t bbp::best_pairs_enqueue(bbp_ctx* ctx, u32 n, const u32* sel, const u32* counts, const u32* win, u32* pairs, hipStream_t s) {
    ScopedEvent ev(ctx, TAG_SELECT, s);
    hipLaunchKernelGGL(k_best_pairs, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, s, n, sel, counts, win, pairs);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

// the K best winners (K == 0: all): selection, pairs, and everything the host reads into the mirror.  *room: pairs fetched at most.
static int32_t best_finish_enqueue(const BestCall& c, const int32_t* status_to_fetch, u32* room) {
    bbp_ctx* ctx = c.ctx;
    const u32 n = c.K && c.K < c.B ? c.K : c.B;
    *room = n;
    if (int32_t rc = select_kernels_enqueue(ctx, c.B, c.at(c.L.win), BEST_NO_FLOOR, c.K, n, c.at(c.L.sel), c.at(c.L.counts), c.d + c.L.state, c.s)) return rc;
    if (int32_t rc = best_pairs_enqueue(ctx, n, c.at(c.L.sel), c.at(c.L.counts), c.at(c.L.win), c.at(c.L.pairs), c.s)) return rc;
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_ctr, c.d + c.L.ctr, 8, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_counts, c.d + c.L.counts, 8, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_pairs, c.d + c.L.pairs, 4 * (size_t)BEST_PAIR_WORDS * n, hipMemcpyDeviceToHost, c.s));
    if (status_to_fetch) BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_status, status_to_fetch, 4 * (size_t)c.B, hipMemcpyDeviceToHost, c.s));
    if (c.D) BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * BEST_D_WORDS, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}

// after the finish has arrived: the call's tally against the device's counters, which the finish must not have moved [and against the
// winners' records the last selection counted], then the outputs
static int32_t best_deliver(const BestCall& c, u32 room, BestTally& t, const BestOut& o, std::string* why) {
    const u32 reached = t.reached, dups = t.dups;
    if (!t.take(c, why)) return BBP_ERR_INTERNAL;
    u32 counts[2];
    memcpy(counts, c.h + c.L.h_counts, 8);
    bool ok = t.reached == reached && t.dups == dups && counts[0] <= room;
    if (c.D) ok = ok && counts[1] == reached && counts[0] == (c.K && c.K < reached ? c.K : reached);
    if (!ok) {
        *why = c.family() + std::to_string(counts[1]) + " winner records are open and " + std::to_string(counts[0]) + " selected (room for " +
               std::to_string(room) + "); the device counted " + std::to_string(t.reached) + " reached and " + std::to_string(t.dups) +
               " rows dropped, the call " + std::to_string(reached) + " and " + std::to_string(dups);
        return BBP_ERR_INTERNAL;
    }
    best_rank_pairs(counts[0], (const u32*)(c.h + c.L.h_pairs), o.cap, o.best);
    *o.n_best = counts[0], *o.n_candidates = t.nc, *o.n_examined = t.examined;
    if (o.n_duplicates) *o.n_duplicates = t.dups;
    return BBP_OK;
}

// An offer to a standing, after its finish has arrived: the tally against the device's counters, the working standing against the call
// (no live candidate left, at most K entries, every one a working row), then the outputs: the offer's rows among the entries, in rank order.
static int32_t stand_deliver(const BestCall& c, BestTally& t, const BestOut& o, std::string* why) {
    const StandCall& S = *c.stand;
    const u32 dups = t.dups, left = t.left;
    if (!t.take(c, why)) return BBP_ERR_INTERNAL;
    const u32 *whdr = (const u32*)(c.h + S.W.h_whdr), *order = (const u32*)(c.h + S.W.h_order), count = whdr[STAND_H_COUNT];
    bool ok = t.dups == dups && t.left == left && t.live() == 0 && count <= S.K;
    for (u32 e = 0; ok && e < count; e++) ok = order[e] < c.B;
    if (!ok) {
        *why = c.family() + "the working standing holds " + std::to_string(count) + " entries; the device counted " + std::to_string(t.dups) +
               " duplicates and " + std::to_string(t.left) + " rows below the bar, the call " + std::to_string(dups) + " and " + std::to_string(left) + "; " +
               std::to_string(t.live()) + " candidates are live";
        return BBP_ERR_INTERNAL;
    }
    u32 ne = 0;
    for (u32 e = 0; e < count; e++)
        if (order[e] >= S.K) {
            if (ne < o.cap) o.best[ne] = order[e] - S.K;
            ne++;
        }
    *o.n_best = ne, *o.n_candidates = t.nc, *o.n_examined = t.examined, *o.n_duplicates = t.dups;
    return BBP_OK;
}
// ... and after its commit has run: what the host keeps of the header
void bbp::stand_record_commit(bbp_ctx::Standing& m, const u32* whdr, u32 rows) {
    m.count = whdr[STAND_H_COUNT];
    memcpy(m.bar, whdr + STAND_H_BAR, 32);
    m.offered += rows;
    m.trip = 0;
}
static void stand_committed(const BestCall& c) {
    const StandCall& S = *c.stand;
    stand_record_commit(*S.meta, (const u32*)(c.h + S.W.h_whdr), S.rows);
}

// The host forms on ONE device's context (c.ctx).  fill(dst): the B x c.staged_row() bytes into the pinned staging area; verdicts(n, sel,
// st): the statuses of the tranche's rows sel[0..n) -- called with no lock of the device held (the host form verifies through the
// caller's handle).  Every submission is enqueued under the context lock and waited for with the lock released: one per tranche and one
// for the finish [two per tranche: for the selection, and for the counters behind the settle].
template <class Fill, class Verdicts>
static int32_t best_run_host(BestCall& c, Fill&& fill, Verdicts&& verdicts, const uint8_t* floor32, u32 tranche, const BestOut& out, int32_t* status) {
    bbp_ctx* const dev = c.ctx;
    std::lock_guard<std::mutex> call(dev->best_mu);
    const u32 B = c.B, K = c.K, first = c.first(), stop_K = c.stand ? 0 : K;  // (an offer to a standing stops when nothing is live)
    BestTally ty;
    std::vector<int32_t> st;
    u32 pending = 0, room = 0, tranches = 0;
    uint8_t stand_floor[32];
    if (c.stand) {  // the floor an offer screens by, from the standing as the last commit left it
        const bbp_ctx::Standing& m = *c.stand->meta;
        u32 f[8];
        stand_screen_floor(m.floor, m.count == m.K, m.bar, f);
        for (int b = 0; b < 32; b++) stand_floor[b] = (uint8_t)(f[b >> 2] >> (8 * (b & 3)));
        floor32 = stand_floor;
    }
    auto fail = [&](const std::string& why, int32_t rc) {
        api_guard(dev, [&]() -> int32_t { return dev->err = why, rc; });
        return rc;
    };
    auto submit = [&](auto&& enqueue) -> int32_t {
        int32_t rc = api_guard(dev, [&]() -> int32_t {
            BBP_HIP_TRY(dev, hipSetDevice(dev->device));
            if (int32_t r = enqueue()) return r;
            BBP_HIP_TRY(dev, hipEventRecord(dev->ev_best, c.s));
            return BBP_OK;
        });
        if (rc) return rc;
        const hipError_t e = wait_event_polling(dev->ev_best);
        return e == hipSuccess ? (int32_t)BBP_OK : fail(c.family() + hipGetErrorString(e), BBP_ERR_DEVICE);
    };
    auto dstatus = [&] { return (int32_t*)c.at(c.L.status); };  // (the state's base is known once it is open)
    auto tstat = [&] { return (const int32_t*)c.at(c.L.tstat); };
    auto mark = [&](u32 n) -> int32_t {  // the statuses of the tranche just verified up, its rows marked
        memcpy(c.h + c.L.h_tstat, st.data(), 4 * (size_t)n);
        BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + c.L.tstat, c.h + c.L.h_tstat, 4 * (size_t)n, hipMemcpyHostToDevice, c.s));
        return best_mark_enqueue(c, n, tstat(), dstatus());
    };
    bool finish = false;
    for (u32 t = 0;; t++) {
        const u32 rows = best_tranche_ask(K, tranche, B, ty, t), room_sel = rows ? rows : B;
        int32_t rc = submit([&]() -> int32_t {
            int32_t r;
            if (t == 0) {
                if ((r = best_open(c))) return r;
                if (c.stand && (r = stand_seed_enqueue(c, dstatus()))) return r;
                const size_t skip = c.staged_row() * first;  // (the entry slots of a standing are not staged: the seed wrote them)
                fill(c.h + c.h_staged() + skip);
                BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + c.staged() + skip, c.h + c.h_staged() + skip, c.staged_row() * (B - first), hipMemcpyHostToDevice, c.s));
                if ((r = best_keys_enqueue(c, c.d + c.staged() + skip, c.staged_row(), 0, floor32, dstatus()))) return r;
                if (c.stand) {  // the leave pass in front of tranche 0; its counts come down with the selection's
                    if ((r = stand_leave_enqueue(c, dstatus()))) return r;
                    BBP_HIP_TRY(dev, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * BEST_D_WORDS, hipMemcpyDeviceToHost, c.s));
                }
            }
            if (pending && (r = mark(pending))) return r;
            if (finish) return c.stand ? stand_finish_enqueue(c, dstatus()) : best_finish_enqueue(c, dstatus(), &room);
            if ((r = best_select_enqueue(c, rows))) return r;
            BBP_HIP_TRY(dev, hipMemcpyAsync(c.h + c.L.h_counts, c.d + c.L.counts, 256 + 4 * (size_t)room_sel, hipMemcpyDeviceToHost, c.s));
            return BBP_OK;
        });
        if (rc) return rc;
        if (finish) break;
        u32 counts[2];
        memcpy(counts, c.h + c.L.h_counts, 8);
        if (c.stand && t == 0) {
            std::string why;
            if (!ty.pre(c, &why)) return fail(why, BBP_ERR_INTERNAL);
        }
        if (!best_tranche_ok(counts, t, K, tranche, ty)) return fail(c.family() + "a tranche of unexpected size", BBP_ERR_INTERNAL);
        const u32 n = counts[0];
        pending = 0;
        if (n) {
            tranches++;
            st.assign(n, BBP_ERR_INTERNAL);
            if ((rc = verdicts(n, (const u32*)(c.h + c.L.h_sel), st.data()))) return rc;
            ty.examined += n;
            if (c.D) {  // the stop rule needs the device's counters: statuses, mark and settle at once, and a wait of their own
                const bool drop = ty.live() > 0;
                rc = submit([&]() -> int32_t {
                    if (int32_t r = mark(n)) return r;
                    return best_counters_enqueue(c, n, tstat(), dstatus(), drop);
                });
                if (rc) return rc;
                std::string why;
                if (!ty.take(c, &why)) return fail(why, BBP_ERR_INTERNAL);
            } else {  // the host can count: the mark travels with the next submission
                pending = n;
                for (u32 j = 0; j < n; j++) ty.reached += st[j] == BBP_OK;
            }
        }
        finish = n == 0 || ty.stop(stop_K);
    }
    std::string why;
    if (c.stand) {  // the host's checks first, then the one commit, then the host's record of what was committed
        if (int32_t rc = stand_deliver(c, ty, out, &why)) return fail(why, rc);
        if (int32_t rc = submit([&]() -> int32_t { return stand_commit_enqueue(c); })) return rc;
        stand_committed(c);
    } else if (int32_t rc = best_deliver(c, room, ty, out, &why))
        return fail(why, rc);
    memcpy(status, c.h + c.L.h_status, 4 * (size_t)(B - first));
    if (out.n_tranches) *out.n_tranches = tranches;
    return BBP_OK;
}

// screening shared by every form's numbers: N, then B (round_select.h round_select_screen: the same checks in the same order)
static int32_t best_screen(bbp_ctx* ctx, const char* what, u32 N, u32 B, bool* done) {
    const int32_t screened = round_select_screen(N, B, done);
    if (!screened) return BBP_OK;
    return api_guard(ctx, [&]() -> int32_t {
        if (int32_t rc = check_n(ctx, N)) return rc;  // (names the list length)
        ctx->err = std::string(what) + ": more than BBP_SELECT_MAX_BIDS rows";
        return screened;
    });
}

// The public host forms.  Staged: the score of every row [score || z_img: adjacent in a row, one gather per row]; a tranche comes from
// the CALLER's memory, through the rounds verifier's own path.  On a pool, keys [identities], selection and marks are member 0's.
int32_t bbp::best_public_host(bbp_ctx* ctx, u32 N, const uint8_t* round, u32 B, const uint8_t* rows, const uint8_t* floor32, u32 K, u32 tranche,
                              bool distinct, const BestOut& out, int32_t* status) {
    return no_throw_ctx(ctx, [&]() -> int32_t {
        bbp_ctx* const dev = is_pool(ctx) ? ctx->members[0] : ctx;
        BestCall c(dev, B, K, dev->stream, true, distinct);
        const size_t rb = round_row_bytes(N), key_off = proof_record_bytes(N), w = c.staged_row();
        std::vector<uint8_t> picked;
        auto fill = [&](u8* dst) {
            for (u32 i = 0; i < B; i++) memcpy(dst + w * i, rows + rb * i + key_off, w);
        };
        auto verdicts = [&](u32 n, const u32* sel, int32_t* st) -> int32_t {
            picked.resize(rb * n);
            for (u32 j = 0; j < n; j++) memcpy(&picked[rb * j], rows + rb * sel[j], rb);
            return verify_host(ctx, VerifyRows::of_rounds(n, 1, &N, round, nullptr), picked.data(), st, BBP_AGG_GROUP_DEFAULT, nullptr);
        };
        const int32_t rc = best_run_host(c, fill, verdicts, floor32, tranche, out, status);
        if (rc && dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
        return rc;
    });
}

// The test hooks: B, then the verdicts (*n_ok: how many are BBP_OK); a tranche's statuses are read from the caller's verdicts.
int32_t bbp::best_hook_refuse(bbp_ctx* ctx, const std::string& why) {
    return api_guard(ctx, [&]() -> int32_t { return ctx->err = why, BBP_ERR_BAD_ARG; });
}
int32_t bbp::best_hook_screen(bbp_ctx* ctx, const char* what, u32 B, const int32_t* verdicts, u32* n_ok) {
    if (B == 0 || B > BBP_SELECT_MAX_BIDS) return best_hook_refuse(ctx, std::string(what) + ": B is 0 or above BBP_SELECT_MAX_BIDS");
    *n_ok = 0;
    for (u32 i = 0; i < B; i++) {
        if (verdicts[i] != BBP_OK && verdicts[i] != BBP_ERR_VERIFY && verdicts[i] != BBP_ERR_FORMAT)
            return best_hook_refuse(ctx, std::string(what) + ": a verdict is none of BBP_OK, BBP_ERR_VERIFY, BBP_ERR_FORMAT");
        *n_ok += verdicts[i] == BBP_OK;
    }
    return BBP_OK;
}
static auto best_hook_read(const int32_t* verdicts) {
    return [verdicts](u32 n, const u32* sel, int32_t* st) -> int32_t {
        for (u32 j = 0; j < n; j++) st[j] = verdicts[sel[j]];
        return BBP_OK;
    };
}
// ... and the call behind the screening: the host driver on caller-made keys, ids (null: the plain call) and verdicts
int32_t bbp::best_hook_host(bbp_ctx* ctx, u32 B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts, const uint8_t* floor32, u32 K, u32 tranche,
                            u32 table_log2, const BestOut& out, int32_t* status) {
    const size_t w = ids ? 64 : 32;
    auto fill = [&](u8* dst) {
        for (u32 i = 0; i < B; i++) {
            memcpy(dst + w * i, keys + 32 * (size_t)i, 32);
            if (ids) memcpy(dst + w * i + 32, ids + 32 * (size_t)i, 32);
        }
    };
    BestCall c(ctx, B, K, ctx->stream, true, ids != nullptr, table_log2);
    return best_run_host(c, fill, best_hook_read(verdicts), floor32, tranche, out, status);
}

// One tranche of n rows (in sel) on the device: the rows and their entropy rows packed, verified through the aggregated rounds path in
// engine calls of at most BBP_HOST_CHUNK_VERIFY rows, as a host-pointer call's are (the packed rows of a part are read before the next
// part's are written: one stream) -> tstat
static int32_t best_verify_enqueue(const BestCall& c, u32 N, const u8* round_dev, const u8* rows_dev, const u8* entropy_dev, u32 n, int32_t* tstat) {
    bbp_ctx* ctx = c.ctx;
    const u32 rb = (u32)round_row_bytes(N), part = std::min(n, host_chunk_verify());
    const BestRows R(part, N);
    if (int32_t rc = dev_reserve(ctx, ctx->best_rows, R.bytes)) return rc;
    u8* g = (u8*)ctx->best_rows.p;
    for (u32 first = 0; first < n; first += part) {
        const u32 m = std::min(part, n - first);
        {
            ScopedEvent ev(ctx, TAG_SELECT, c.s);
            hipLaunchKernelGGL(k_best_gather, dim3(m), dim3(BEST_GATHER_T), 0, c.s, rb, first, (const u32*)c.at(c.L.sel), (const u32*)c.at(c.L.counts),
                               rows_dev, entropy_dev, g + R.rows, g + R.ent);
            BBP_HIP_TRY(ctx, hipGetLastError());
        }
        if (int32_t rc = verify_batch_agg_dev(ctx, VerifyRows::of_rounds(m, 1, &N, round_dev, nullptr), BBP_AGG_GROUP_DEFAULT, g + R.rows, g + R.ent,
                                              tstat + first, c.s, nullptr))
            return rc;
    }
    return BBP_OK;
}

// The device forms, everything on c.s.  They synchronise c.s after the first selection (the candidate count), once per tranche (the
// counters behind the mark [and the settle], which decide whether another tranche runs and size it) and once to deliver the results;
// the context lock is held throughout, as by a _dev call that delivers n_fallback.
static int32_t best_run_dev(BestCall& c, u32 N, const u8* round_dev, const u8* rows_dev, const u8* entropy_dev, const uint8_t* floor32, u32 tranche,
                            const BestOut& out, int32_t* status) {
    bbp_ctx* const ctx = c.ctx;
    std::lock_guard<std::mutex> call(ctx->best_mu);
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = best_open(c)) || (rc = best_keys_enqueue(c, rows_dev, round_row_bytes(N), proof_record_bytes(N), floor32, status))) return rc;
        BestTally ty;
        std::string why;
        u32 room = 0, tranches = 0;
        for (u32 t = 0;; t++) {
            u32 n = best_tranche_ask(c.K, tranche, c.B, ty, t);
            if ((rc = best_select_enqueue(c, n))) return rc;
            if (t == 0) {
                BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_counts, c.d + c.L.counts, 8, hipMemcpyDeviceToHost, c.s));
                BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));
                u32 counts[2];
                memcpy(counts, c.h + c.L.h_counts, 8);
                if (!best_tranche_ok(counts, 0, c.K, tranche, ty)) return ctx->err = c.family() + "a tranche of unexpected size", BBP_ERR_INTERNAL;
                n = counts[0];
            }
            if (n == 0) break;
            tranches++;
            int32_t* tstat = (int32_t*)c.at(c.L.tstat);
            if ((rc = best_verify_enqueue(c, N, round_dev, rows_dev, entropy_dev, n, tstat))) return rc;
            ty.examined += n;
            if ((rc = best_mark_enqueue(c, n, tstat, status)) || (rc = best_counters_enqueue(c, n, tstat, status, ty.live() > 0))) return rc;
            BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));  // rows examined and OK [identities settled, rows dropped]
            if (!ty.take(c, &why)) return ctx->err = why, BBP_ERR_INTERNAL;
            if (ty.stop(c.K)) break;
        }
        if ((rc = best_finish_enqueue(c, nullptr, &room))) return rc;
        BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));
        if ((rc = best_deliver(c, room, ty, out, &why))) ctx->err = why;
        if (!rc && out.n_tranches) *out.n_tranches = tranches;
        return rc;
    });
}
// ... and the call of the _dev forms behind their screening (the caller keeps exceptions on this side of the boundary)
int32_t bbp::best_public_dev(bbp_ctx* ctx, u32 N, const void* round_dev, u32 B, const void* rows_dev, const void* entropy_dev, const uint8_t* floor32, u32 K,
                             u32 tranche, bool distinct, const BestOut& out, void* status_dev, void* stream) {
    BestCall c(ctx, B, K, pick_stream(ctx, stream), false, distinct);
    return best_run_dev(c, N, (const u8*)round_dev, (const u8*)rows_dev, (const u8*)entropy_dev, floor32, tranche, out, (int32_t*)status_dev);
}

extern "C" int32_t bbp_verify_round_best(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* rows, const uint8_t floor32[32], uint32_t K,
                                         uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                                         int32_t* status) {
    if (!ctx || !round || !rows || !floor32 || !n_best || !n_candidates || !n_examined || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    *n_best = *n_candidates = *n_examined = 0;
    bool done;
    if (int32_t rc = best_screen(ctx, "bbp_verify_round_best", N, B, &done)) return rc;
    if (done) return BBP_OK;
    return best_public_host(ctx, N, round, B, rows, floor32, K, tranche, false, BestOut{cap, best_out, n_best, n_candidates, n_examined, nullptr}, status);
}

// Test hook: the shipped key, selection, mark and ranking kernels on caller-made keys and verdicts.  Synchronises.
extern "C" int32_t bbp_debug_round_best(bbp_ctx* ctx, uint32_t B, const uint8_t* keys, const int32_t* verdicts, const uint8_t floor32[32], uint32_t K,
                                        uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                                        int32_t* status) {
    if (!ctx || !keys || !verdicts || !floor32 || !n_best || !n_candidates || !n_examined || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_round_best");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        u32 n_ok;
        if (int32_t rc = best_hook_screen(ctx, "bbp_debug_round_best", B, verdicts, &n_ok)) return rc;
        return best_hook_host(ctx, B, keys, nullptr, verdicts, floor32, K, tranche, 0, BestOut{cap, best_out, n_best, n_candidates, n_examined, nullptr}, status);
    });
}

extern "C" int32_t bbp_verify_round_best_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* rows_dev, const void* entropy_dev,
                                             const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                             uint32_t* n_candidates, uint32_t* n_examined, void* status_dev, void* stream) {
    if (!ctx || !round_dev || !rows_dev || !entropy_dev || !floor32 || !n_best || !n_candidates || !n_examined || !status_dev || (cap && !best_out))
        return BBP_ERR_BAD_ARG;
    *n_best = *n_candidates = *n_examined = 0;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_verify_round_best_dev");
    bool done;
    if (int32_t rc = best_screen(ctx, "bbp_verify_round_best_dev", N, B, &done)) return rc;
    if (done) return BBP_OK;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        return best_public_dev(ctx, N, round_dev, B, rows_dev, entropy_dev, floor32, K, tranche, false,
                               BestOut{cap, best_out, n_best, n_candidates, n_examined, nullptr}, status_dev, stream);
    });
}

// ---- best proofs of a round, one per bidder (include/bbp.h; rules and kernels: round_best.h) ------------------------------------------
// The calls above with an identity table: the same drivers over a BestCall that has one.
extern "C" int32_t bbp_verify_round_best_distinct(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* rows, const uint8_t floor32[32],
                                                  uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates,
                                                  uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status) {
    if (!ctx || !round || !rows || !floor32 || !n_best || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    *n_best = *n_candidates = *n_examined = *n_duplicates = 0;
    bool done;
    if (int32_t rc = best_screen(ctx, "bbp_verify_round_best_distinct", N, B, &done)) return rc;
    if (done) return BBP_OK;
    return best_public_host(ctx, N, round, B, rows, floor32, K, tranche, true, BestOut{cap, best_out, n_best, n_candidates, n_examined, n_duplicates}, status);
}

// Test hook: the shipped key, identity, selection, mark, settle, holder, drop and ranking kernels on caller-made keys, ids and verdicts.
extern "C" int32_t bbp_debug_round_best_distinct(bbp_ctx* ctx, uint32_t B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts,
                                                 const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t table_log2, uint32_t* best_out,
                                                 uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status) {
    if (!ctx || !keys || !ids || !verdicts || !floor32 || !n_best || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !best_out))
        return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_round_best_distinct");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        u32 n_ok;
        if (int32_t rc = best_hook_screen(ctx, "bbp_debug_round_best_distinct", B, verdicts, &n_ok)) return rc;
        if (table_log2 > BEST_TABLE_LOG2_MAX || (table_log2 && (1u << table_log2) <= n_ok))
            return best_hook_refuse(ctx, "bbp_debug_round_best_distinct: table_log2 is above 21, or the table has no slot more than there are BBP_OK verdicts");
        return best_hook_host(ctx, B, keys, ids, verdicts, floor32, K, tranche, table_log2,
                              BestOut{cap, best_out, n_best, n_candidates, n_examined, n_duplicates}, status);
    });
}

extern "C" int32_t bbp_verify_round_best_distinct_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* rows_dev, const void* entropy_dev,
                                                      const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                                      uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, void* status_dev, void* stream) {
    if (!ctx || !round_dev || !rows_dev || !entropy_dev || !floor32 || !n_best || !n_candidates || !n_examined || !n_duplicates || !status_dev ||
        (cap && !best_out))
        return BBP_ERR_BAD_ARG;
    *n_best = *n_candidates = *n_examined = *n_duplicates = 0;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_verify_round_best_distinct_dev");
    bool done;
    if (int32_t rc = best_screen(ctx, "bbp_verify_round_best_distinct_dev", N, B, &done)) return rc;
    if (done) return BBP_OK;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        return best_public_dev(ctx, N, round_dev, B, rows_dev, entropy_dev, floor32, K, tranche, true,
                               BestOut{cap, best_out, n_best, n_candidates, n_examined, n_duplicates}, status_dev, stream);
    });
}

// ---- standing of a round (include/bbp.h; rules and kernels: round_standing.h) ---------------------------------------------------------
// An offer is a one-per-bidder host call over K + B working rows with a StandCall: the same driver.  The standings of a handle live on
// ONE device's context (a pool: member 0), found and changed under its best_mu.
bbp_ctx* bbp::stand_dev(bbp_ctx* ctx) { return is_pool(ctx) ? ctx->members[0] : ctx; }
int32_t bbp::stand_refuse(bbp_ctx* ctx, const std::string& why) {
    return api_guard(ctx, [&]() -> int32_t { return ctx->err = why, BBP_ERR_BAD_ARG; });
}
// the open standing behind a handle, or null (caller holds dev->best_mu)
bbp_ctx::Standing* bbp::stand_find(bbp_ctx* dev, u32 handle) {
    return dev->stand_handles.is_open(handle) ? &dev->stand_meta[handle] : nullptr;
}

extern "C" int32_t bbp_standing_open(bbp_ctx* ctx, uint32_t N, const uint8_t* round, const uint8_t floor32[32], uint32_t K, uint32_t* standing) {
    if (!ctx || !round || !floor32 || !standing) return BBP_ERR_BAD_ARG;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        if (N == 0 || N > BBP_MAX_ITEMS) return api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
        if (K == 0 || K > BBP_STANDING_MAX_K) return stand_refuse(ctx, "bbp_standing_open: K is 0 or above BBP_STANDING_MAX_K");
        bbp_ctx* const dev = stand_dev(ctx);
        std::lock_guard<std::mutex> call(dev->best_mu);
        const u32 h = dev->stand_handles.take();
        if (h == BBP_STANDING_MAX_OPEN) return stand_refuse(ctx, "bbp_standing_open: BBP_STANDING_MAX_OPEN standings are open on this handle");
        bbp_ctx::Standing m;
        m.N = N, m.K = K;
        const RsFloor f = rs_floor_load(floor32);
        memcpy(m.floor, f.w, 32);
        m.round.assign(round, round + round_table_bytes(N));
        const int32_t rc = api_guard(dev, [&]() -> int32_t {
            BBP_HIP_TRY(dev, hipSetDevice(dev->device));
            const StandingLayout SL(K);
            if (int32_t r = dev_reserve(dev, dev->stand[h], SL.bytes)) return r;
            BBP_HIP_TRY(dev, hipMemsetAsync(dev->stand[h].p, 0, SL.bytes, dev->stream));  // count 0, offered 0
            BBP_HIP_TRY(dev, hipStreamSynchronize(dev->stream));
            return BBP_OK;
        });
        if (rc) {
            dev->stand_handles.release(h);
            if (dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
            return rc;
        }
        dev->stand_meta[h] = std::move(m);
        *standing = h;
        return BBP_OK;
    });
}

extern "C" int32_t bbp_standing_close(bbp_ctx* ctx, uint32_t standing) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        bbp_ctx* const dev = stand_dev(ctx);
        std::lock_guard<std::mutex> call(dev->best_mu);
        if (!dev->stand_handles.release(standing)) return stand_refuse(ctx, "bbp_standing_close: no open standing has this handle");
        dev->stand_meta[standing] = bbp_ctx::Standing{};
        return api_guard(dev, [&]() -> int32_t {
            DevBuf& b = dev->stand[standing];
            BBP_HIP_TRY(dev, hipSetDevice(dev->device));
            if (b.p) {
                BBP_HIP_TRY(dev, hipFree(b.p));  // (waits for the device: no offer is in flight, best_mu is held)
                dev->scratch_bytes -= b.cap;
            }
            b = DevBuf{};
            return BBP_OK;
        });
    });
}

extern "C" int32_t bbp_standing_read(bbp_ctx* ctx, uint32_t standing, uint32_t cap, uint64_t* serials_out, uint8_t* scores_out, uint8_t* z_imgs_out,
                                     uint32_t* n_entries, uint64_t* n_offered) {
    if (!ctx || !n_entries) return BBP_ERR_BAD_ARG;
    *n_entries = 0;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        bbp_ctx* const dev = stand_dev(ctx);
        std::lock_guard<std::mutex> call(dev->best_mu);
        const bbp_ctx::Standing* m = stand_find(dev, standing);
        if (!m) return stand_refuse(ctx, "bbp_standing_read: no open standing has this handle");
        const int32_t rc = api_guard(dev, [&]() -> int32_t {
            BBP_HIP_TRY(dev, hipSetDevice(dev->device));
            const StandingLayout SL(m->K);
            const u8* st = (const u8*)dev->stand[standing].p;
            u32 hdr[STAND_H_WORDS];
            BBP_HIP_TRY(dev, hipMemcpy(hdr, st + SL.hdr, sizeof hdr, hipMemcpyDeviceToHost));  // (the device's own record, not the host's shadow)
            const u32 count = hdr[STAND_H_COUNT];
            if (count > m->K) return dev->err = "standing of a round: the state holds more than K entries", BBP_ERR_INTERNAL;
            const u32 n = count < cap ? count : cap;
            std::vector<u32> w(8 * (size_t)n);
            auto words_out = [&](size_t off, uint8_t* out) -> int32_t {  // n x 8 words -> n x 32 little-endian bytes
                if (!out || !n) return BBP_OK;
                BBP_HIP_TRY(dev, hipMemcpy(w.data(), st + off, 32 * (size_t)n, hipMemcpyDeviceToHost));
                for (size_t b = 0; b < 32 * (size_t)n; b++) out[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
                return BBP_OK;
            };
            if (int32_t r = words_out(SL.keys, scores_out)) return r;
            if (int32_t r = words_out(SL.ids, z_imgs_out)) return r;
            if (serials_out && n) {
                BBP_HIP_TRY(dev, hipMemcpy(w.data(), st + SL.serials, 8 * (size_t)n, hipMemcpyDeviceToHost));
                for (u32 e = 0; e < n; e++) serials_out[e] = ((uint64_t)w[2 * (size_t)e + 1] << 32) | w[2 * (size_t)e];
            }
            *n_entries = count;
            if (n_offered) *n_offered = ((uint64_t)hdr[STAND_H_OFFERED + 1] << 32) | hdr[STAND_H_OFFERED];
            return BBP_OK;
        });
        if (rc && dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
        return rc;
    });
}

// Both forms of an offer behind their screening: the standing looked up, the one-per-bidder call over K + B working rows built, run by
// the host driver.  run(c, m): the form's fill and verdicts for the standing m, handed to best_run_host with the call c.
template <class Run>
static int32_t stand_offer(bbp_ctx* ctx, const char* what, u32 standing, u32 B, Run&& run) {
    bbp_ctx* const dev = stand_dev(ctx);
    bbp_ctx::Standing* m;
    {
        std::lock_guard<std::mutex> call(dev->best_mu);
        m = stand_find(dev, standing);
    }
    if (!m) return stand_refuse(ctx, std::string(what) + ": no open standing has this handle");
    BestCall c(dev, m->K + B, m->K, dev->stream, true, true);
    StandCall S(m, (u8*)dev->stand[standing].p, B, *c.D);
    c.stand = &S;
    const int32_t rc = run(c, *m);
    if (rc && dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
    return rc;
}

extern "C" int32_t bbp_standing_offer(bbp_ctx* ctx, uint32_t standing, uint32_t B, const uint8_t* rows, uint32_t tranche, uint32_t cap, uint32_t* entered_out,
                                      uint32_t* n_entered, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        {
            bbp_ctx* const dev = stand_dev(ctx);
            std::lock_guard<std::mutex> call(dev->best_mu);
            if (!stand_find(dev, standing)) return stand_refuse(ctx, "bbp_standing_offer: no open standing has this handle");
        }
        if (!rows || !n_entered || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !entered_out))
            return stand_refuse(ctx, "bbp_standing_offer: a NULL pointer");
        *n_entered = *n_candidates = *n_examined = *n_duplicates = 0;
        if (B > BBP_SELECT_MAX_BIDS) return stand_refuse(ctx, "bbp_standing_offer: more than BBP_SELECT_MAX_BIDS rows");
        if (B == 0) return BBP_OK;
        return stand_public_host(ctx, "bbp_standing_offer", standing, B, rows, tranche,
                                 BestOut{cap, entered_out, n_entered, n_candidates, n_examined, n_duplicates}, status);
    });
}
// ... and behind that screening (the many-standings call with one standing runs it too; out.n_tranches: the tranches that ran)
int32_t bbp::stand_public_host(bbp_ctx* ctx, const char* what, u32 standing, u32 B, const uint8_t* rows, u32 tranche, const BestOut& out, int32_t* status) {
    return stand_offer(ctx, what, standing, B,
                       [&](BestCall& c, const bbp_ctx::Standing& m) -> int32_t {
                           const u32 N = m.N, K = m.K;
                           const size_t rb = round_row_bytes(N), key_off = proof_record_bytes(N);
                           std::vector<uint8_t> picked;
                           auto fill = [&](u8* dst) {
                               for (u32 i = 0; i < B; i++) memcpy(dst + 64 * (size_t)i, rows + rb * i + key_off, 64);
                           };
                           auto verdicts = [&](u32 n, const u32* sel, int32_t* st) -> int32_t {  // (sel: working rows; row sel[j] - K of the offer)
                               picked.resize(rb * n);
                               for (u32 j = 0; j < n; j++) memcpy(&picked[rb * j], rows + rb * (sel[j] - K), rb);
                               return verify_host(ctx, VerifyRows::of_rounds(n, 1, &N, m.round.data(), nullptr), picked.data(), st, BBP_AGG_GROUP_DEFAULT,
                                                  nullptr);
                           };
                           return best_run_host(c, fill, verdicts, nullptr, tranche, out, status);
                       });
}

// Test hook: an offer of caller-made keys, ids and verdicts through the shipped kernels against the standing's state.
extern "C" int32_t bbp_debug_standing_offer(bbp_ctx* ctx, uint32_t standing, uint32_t B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts,
                                            uint32_t tranche, uint32_t cap, uint32_t* entered_out, uint32_t* n_entered, uint32_t* n_candidates,
                                            uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_standing_offer");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        {
            std::lock_guard<std::mutex> call(ctx->best_mu);
            if (!stand_find(ctx, standing)) return stand_refuse(ctx, "bbp_debug_standing_offer: no open standing has this handle");
        }
        if (!keys || !ids || !verdicts || !n_entered || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !entered_out))
            return stand_refuse(ctx, "bbp_debug_standing_offer: a NULL pointer");
        *n_entered = *n_candidates = *n_examined = *n_duplicates = 0;
        if (B == 0) return BBP_OK;  // (as the offer itself: zero counts, the standing unchanged)
        u32 n_ok;
        if (int32_t rc = best_hook_screen(ctx, "bbp_debug_standing_offer", B, verdicts, &n_ok)) return rc;
        return stand_hook_host(ctx, "bbp_debug_standing_offer", standing, B, keys, ids, verdicts, tranche,
                               BestOut{cap, entered_out, n_entered, n_candidates, n_examined, n_duplicates}, status);
    });
}
int32_t bbp::stand_hook_host(bbp_ctx* ctx, const char* what, u32 standing, u32 B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts, u32 tranche,
                             const BestOut& out, int32_t* status) {
    return stand_offer(ctx, what, standing, B,
                       [&](BestCall& c, const bbp_ctx::Standing& m) -> int32_t {
                           const u32 K = m.K;
                           auto fill = [&](u8* dst) {
                               for (u32 i = 0; i < B; i++)
                                   memcpy(dst + 64 * (size_t)i, keys + 32 * (size_t)i, 32), memcpy(dst + 64 * (size_t)i + 32, ids + 32 * (size_t)i, 32);
                           };
                           auto read = [&](u32 n, const u32* sel, int32_t* st) -> int32_t {
                               for (u32 j = 0; j < n; j++) st[j] = verdicts[sel[j] - K];
                               return BBP_OK;
                           };
                           return best_run_host(c, fill, read, nullptr, tranche, out, status);
                       });
}

extern "C" int32_t bbp_debug_standing_trip(bbp_ctx* ctx, uint32_t standing, uint32_t after) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_standing_trip");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        std::lock_guard<std::mutex> call(ctx->best_mu);
        bbp_ctx::Standing* m = stand_find(ctx, standing);
        if (!m || after == 0) return stand_refuse(ctx, "bbp_debug_standing_trip: no open standing has this handle, or after is 0");
        m->trip = after;
        return BBP_OK;
    });
}
