// C-ABI, best proofs of MANY rounds, plain and one per bidder, with their hooks and _dev forms, and an offer to MANY standings -- see
// include/bbp.h.  A call with one round, or one standing, runs the single-round calls of capi_best.hip (capi.h).
#include <string.h>

#include <algorithm>
#include <optional>

#include "capi.h"
#include "rounds_best.h"
#include "rounds_best_distinct.h"
#include "standings.h"

using namespace bbp;

// ---- best valid proofs of many rounds (include/bbp.h; rules and kernels: rounds_best.h) ---------------------------------------------
// The launch sequence of one call with R > 1, on ONE device's context and one stream.  {..}: what the one-per-bidder calls add -- the
// same calls, plus an identity table (BestsDistinctLayout behind BestsLayout(B, R, false), same allocations):
//   open      the state reserved, the counters and sel zeroed {settled, dups and the flag zeroed, the table emptied}; floors, round_of
//             [the _dev form: row offsets and row sizes; the host forms: the keys {the staged score || z_img rows, 64 bytes each}] up
//   segment   {k_bests_ids,} k_bests_keys, k_bests_scan (ncand -> seg), k_bests_place
//   per step  k_bests_plan {k_bests_plan_distinct} (take), k_bests_scan (take -> off), k_bests_select over the candidate records -> sel;
//             [the rows verified];  k_bests_mark {k_bests_settle, k_bests_holders, k_bests_drop (which does nothing for a round that has
//             stopped)}
//   finish    k_bests_plan {k_bests_plan_distinct} (winners {the settled identities}), k_bests_scan, k_bests_select over the winner
//             records, k_best_pairs; ctr, pairs [statuses] down
// <..>: an offer to many standings (standings.h), a one-per-bidder host call over the working rows with the standings as its rounds:
//   open      <sctr zeroed, the parameter table and the local indices up, k_stands_seed>
//   segment   the ids and keys of the OFFER rows; <k_stands_plan: the segment sizes;> scan, place <k_stands_enter, k_stands_leave>
//   per step  <k_stands_plan in k_bests_plan_distinct's place>; behind settle and holders, in k_bests_drop's place: <k_stands_displace,
//             k_stands_plan (the winners to keep), scan, k_bests_select over the winner records, k_stands_merge, k_stands_leave>
//   finish    <no selection: the working headers, order and statuses down; after the host's checks k_stands_commit, a submission of its own>
struct BestsCall {
    bbp_ctx* ctx;
    u32 R, B, K, tranche;
    hipStream_t s;
    BestsLayout L;
    std::optional<BestsDistinctLayout> D;  // one per bidder only (rounds_best_distinct.h)
    struct StandsCall* stands = nullptr;   // an offer to many standings only (below): B is the working rows, R the standings
    u8 *d = nullptr, *h = nullptr;
    // host_rows: a host form, which stages bytes of every row -- the 32 key bytes (in L), one per bidder score || z_img (in D)
    BestsCall(bbp_ctx* c, u32 R_, u32 B_, u32 K_, u32 tranche_, hipStream_t s_, bool host_rows, bool distinct = false, u32 table_log2 = 0)
        : ctx(c), R(R_), B(B_), K(K_), tranche(tranche_), s(s_), L(B_, R_, host_rows && !distinct) {
        if (distinct) D.emplace(L, B_, R_, table_log2, host_rows);
    }
    u32* at(size_t off) const { return (u32*)(d + off); }
    u32* ctr(u32 word) const { return (u32*)(d + L.ctr) + word; }
    const u32* mirror(u32 word) const { return (const u32*)(h + L.h_ctr) + word; }
    u32* dctr(u32 word) const { return (u32*)(d + D->dctr) + word; }
    const u32* dmirror(u32 word) const { return (const u32*)(h + D->h_dctr) + word; }
    size_t bytes() const;
    size_t h_bytes() const;
    u32 first() const;  // the working rows in front of the call's own: the standings' entry slots, otherwise none
    size_t staged_row() const { return D ? 64 : 32; }
    size_t staged() const { return D ? D->kid : L.keys; }
    size_t h_staged() const { return D ? D->h_kid : L.h_keys; }
    const char* family() const {
        return stands ? "standings of many rounds: " : D ? "best proofs of many rounds, one per bidder: " : "best valid proofs of many rounds: ";
    }
    unsigned long long* offb() const { return (unsigned long long*)(d + L.offb); }
};
// What an offer to many standings adds (standings.h): the standings' own allocations and the host's records of them, the scratch behind
// the call's, and what the host counts between the steps.
struct StandsCall {
    u32 S, sumK = 0, rows;  // rows: the call's
    std::vector<bbp_ctx::Standing*> meta;
    std::vector<u8*> st;
    std::vector<u32> K, E, n_rows, merges, local;
    std::optional<StandingsLayout> W;
    StandsCall(bbp_ctx* dev, u32 S_, const u32* handles, u32 B, const u32* standing_of) : S(S_), rows(B), meta(S_), st(S_), K(S_), E(S_), n_rows(S_, 0), merges(S_, 0), local(B) {
        for (u32 s = 0; s < S; s++) {
            meta[s] = &dev->stand_meta[handles[s]], st[s] = (u8*)dev->stand[handles[s]].p;
            K[s] = meta[s]->K, E[s] = sumK, sumK += K[s];
        }
        for (u32 i = 0; i < B; i++) local[i] = n_rows[standing_of[i]]++;
    }
    // the standings whose merge behind a step with these rows is the one bbp_debug_standing_trip asked for (once)
    unsigned long long trips(const u32* take) {
        unsigned long long mask = 0;
        for (u32 s = 0; s < S; s++)
            if (take[s] && meta[s]->trip && meta[s]->trip == ++merges[s]) mask |= 1ull << s, meta[s]->trip = 0;
        return mask;
    }
};
size_t BestsCall::bytes() const { return stands ? stands->W->bytes : D ? D->bytes : L.bytes; }
size_t BestsCall::h_bytes() const { return stands ? stands->W->h_bytes : D ? D->h_bytes : L.h_bytes; }
u32 BestsCall::first() const { return stands ? stands->sumK : 0; }
// where a call's results go: R x cap, R, R, R entries; n_steps may be null
struct BestsOut {
    u32 cap;
    u32 *best, *n_best, *n_candidates, *n_examined, *n_steps;
    u32* n_duplicates = nullptr;  // the one-per-bidder calls: R entries
    // the same places as one round's call fills them (R == 1: the single-round drivers run it)
    BestOut one_round() const { return BestOut{cap, best, n_best, n_candidates, n_examined, n_duplicates, n_steps}; }
};

// open: floors32 (R x 32 bytes or null), round_of (B, host), [rowoff (B u64) and rb (R): the _dev form] go up through the mirror
static int32_t bests_open(BestsCall& c, const uint8_t* floors, const u32* round_of, const unsigned long long* rowoff, const u32* rb) {
    bbp_ctx* ctx = c.ctx;
    const BestsLayout& L = c.L;
    int32_t rc;
    if ((rc = dev_reserve(ctx, ctx->best_dev, c.bytes())) || (rc = pinned_reserve(ctx, ctx->best_h, ctx->best_h_cap, c.h_bytes()))) return rc;
    if (!ctx->ev_best) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_best, hipEventDisableTiming));
    c.d = (u8*)ctx->best_dev.p, c.h = (u8*)ctx->best_h;
    BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + L.ctr, 0, 4 * (size_t)L.c_words, c.s));
    if (c.D) {  // [settled, dups and the flag zeroed, the table emptied]
        BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + c.D->dctr, 0, 4 * (size_t)c.D->d_words, c.s));
        BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + c.D->table, 0xff, 4 * (size_t)c.D->slots, c.s));
    }
    BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + L.sel, 0, 4 * (size_t)c.B, c.s));
    if (floors) {
        memcpy(c.h + L.h_floors, floors, 32 * (size_t)c.R);
        BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + L.floors, c.h + L.h_floors, 32 * (size_t)c.R, hipMemcpyHostToDevice, c.s));
    } else
        BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + L.floors, 0, 32 * (size_t)c.R, c.s));
    memcpy(c.h + L.h_round_of, round_of, 4 * (size_t)c.B);
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + L.round_of, c.h + L.h_round_of, 4 * (size_t)c.B, hipMemcpyHostToDevice, c.s));
    if (rowoff) {
        memcpy(c.h + L.h_rowoff, rowoff, 8 * (size_t)c.B);
        memcpy(c.h + L.h_rb, rb, 4 * (size_t)c.R);
        BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + L.rowoff, c.h + L.h_rowoff, 8 * (size_t)c.B, hipMemcpyHostToDevice, c.s));
        BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + L.rb, c.h + L.h_rb, 4 * (size_t)c.R, hipMemcpyHostToDevice, c.s));
    }
    return BBP_OK;
}

static int32_t bests_scan_enqueue(const BestsCall& c, u32 in_word, u32 out_word, bool bytes) {
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_scan, dim3(1), dim3(BESTS_T), 0, c.s, c.R, (const u32*)c.ctr(in_word), bytes ? (const u32*)c.at(c.L.rb) : (const u32*)nullptr,
                       c.ctr(out_word), bytes ? c.offb() : (unsigned long long*)nullptr);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// {one per bidder, in front of the segment pass} ids [the staged rows: where each starts, so that k_bests_keys reads the score of the
// same staged row]
static int32_t bests_ids_enqueue(const BestsCall& c, const u8* base, bool dev_rows) {
    const BestsLayout& L = c.L;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    if (!dev_rows) BBP_HIP_TRY(c.ctx, hipMemsetD32Async((hipDeviceptr_t)c.at(L.rb), 64, c.R, c.s));  // a staged row: 64 bytes in every round
    auto* rowoff = (unsigned long long*)(c.d + L.rowoff);
    const u32 f = c.first(), n = c.B - f;  // <base is the staged row of the offer's row 0, which is working row f>
    hipLaunchKernelGGL(k_bests_ids, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, n, base, dev_rows ? (const unsigned long long*)rowoff : nullptr,
                       (const u32*)c.at(L.rb), (const u32*)c.at(L.round_of) + f, c.at(c.D->ids) + 8 * (size_t)f, dev_rows ? nullptr : rowoff);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// <an offer to many standings, on c.s>  Seed: behind bests_open, before the keys.  Plan: k_stands_plan in one of its modes, into take.
// Enter: behind the segment starts -- the entry slots into their segments and the identity table -- then the leave pass in front of
// step 0.  Merge: behind a step's holders.  Finish: everything the host reads.  Commit: a submission of its own, after the host's checks.
static int32_t stands_seed_enqueue(const BestsCall& c, int32_t* status) {
    bbp_ctx* ctx = c.ctx;
    const StandsCall& S = *c.stands;
    const StandingsLayout& W = *S.W;
    u32* par = (u32*)(c.h + W.h_par);
    for (u32 s = 0; s < S.S; s++) {
        const StandingLayout SL(S.K[s]);
        u32* p = par + (size_t)STANDS_P_WORDS * s;
        const unsigned long long ptr = (unsigned long long)(uintptr_t)S.st[s];
        p[STANDS_P_PTR] = (u32)ptr, p[STANDS_P_PTR + 1] = (u32)(ptr >> 32), p[STANDS_P_K] = S.K[s], p[STANDS_P_E] = S.E[s], p[STANDS_P_ROWS] = S.n_rows[s];
        p[STANDS_P_KEYS] = (u32)SL.keys, p[STANDS_P_IDS] = (u32)SL.ids, p[STANDS_P_SERIALS] = (u32)SL.serials;
    }
    memcpy(c.h + W.h_local, S.local.data(), 4 * (size_t)S.rows);
    BBP_HIP_TRY(ctx, hipMemsetAsync(c.d + W.sctr, 0, 4 * (size_t)S.S, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + W.par, c.h + W.h_par, 4 * (size_t)STANDS_P_WORDS * S.S, hipMemcpyHostToDevice, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.d + W.local, c.h + W.h_local, 4 * (size_t)S.rows, hipMemcpyHostToDevice, c.s));
    ScopedEvent ev(ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stands_seed, dim3((S.sumK + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.S, S.sumK, (const u32*)c.at(W.par), c.at(c.L.recs), c.at(c.L.win),
                       c.at(c.D->ids), status, c.at(W.whdr), c.at(W.wserial), c.at(W.order));
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t stands_plan_enqueue(const BestsCall& c, u32 mode, u32 t) {
    const BestsLayout& L = c.L;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stands_plan, dim3((c.R + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.R, mode, t, c.tranche, (const u32*)c.at(c.stands->W->par),
                       (const u32*)c.ctr(L.c_ncand), (const u32*)c.ctr(L.c_examined), (const u32*)c.dctr(c.D->d_dups), (const u32*)c.at(c.stands->W->sctr),
                       c.ctr(L.c_take), c.ctr(L.c_tranches));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t stands_leave_enqueue(const BestsCall& c, int32_t* status) {
    const StandingsLayout& W = *c.stands->W;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stands_leave, dim3((c.B + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.B, (const u32*)c.at(W.par), c.at(c.L.recs),
                       (const u32*)c.at(c.D->ids), (const u32*)c.at(c.L.round_of), (const u32*)c.at(c.D->table), c.D->slots - 1, (const u32*)c.at(W.whdr), status,
                       c.at(W.sctr), c.dctr(c.D->d_dups), c.dctr(c.D->d_flag));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t stands_enter_enqueue(const BestsCall& c, int32_t* status) {
    const StandsCall& S = *c.stands;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_stands_enter, dim3((S.sumK + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.S, S.sumK, (const u32*)c.at(S.W->par), (const u32*)c.at(c.L.win),
                           (const u32*)c.at(c.D->ids), (const u32*)c.at(c.L.round_of), (const u32*)c.ctr(c.L.c_ncand), (const u32*)c.ctr(c.L.c_seg), c.at(c.L.cand),
                           c.at(c.D->table), c.D->slots - 1, c.dctr(c.D->d_flag));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    return stands_leave_enqueue(c, status);
}
static int32_t bests_select_enqueue(const BestsCall& c, bool finish);
static int32_t bests_scan_enqueue(const BestsCall& c, u32 in_word, u32 out_word, bool bytes);
// behind the holders of step t, whose rows were take[s] of standing s
static int32_t stands_merge_enqueue(const BestsCall& c, u32 t, const u32* take, int32_t* status) {
    StandsCall& S = *c.stands;
    const BestsLayout& L = c.L;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_stands_displace, dim3((S.sumK + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.sumK, (const u32*)c.at(c.D->ids), (const u32*)c.at(L.round_of),
                           (const u32*)c.at(c.D->table), c.D->slots - 1, c.at(L.win), c.at(L.sel), c.dctr(c.D->d_flag));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    int32_t rc;
    if ((rc = stands_plan_enqueue(c, STANDS_PLAN_WINNERS, t)) || (rc = bests_scan_enqueue(c, L.c_take, L.c_off, false)) || (rc = bests_select_enqueue(c, true))) return rc;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_stands_merge, dim3(S.S), dim3(STAND_MERGE_T), 0, c.s, c.B, (const u32*)c.at(S.W->par), (const u32*)c.ctr(L.c_take), (const u32*)c.ctr(L.c_off),
                           (const u32*)c.at(L.sel), (const u32*)c.at(L.win), c.at(S.W->whdr), c.at(S.W->order), S.trips(take), c.dctr(c.D->d_flag));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    return stands_leave_enqueue(c, status);
}
static int32_t stands_counters_fetch(const BestsCall& c) {
    const StandingsLayout& W = *c.stands->W;
    BBP_HIP_TRY(c.ctx, hipMemcpyAsync(c.h + W.h_sctr, c.d + W.sctr, 4 * (size_t)c.R, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}
static int32_t stands_finish_enqueue(const BestsCall& c, const int32_t* status) {
    bbp_ctx* ctx = c.ctx;
    const StandsCall& S = *c.stands;
    const StandingsLayout& W = *S.W;
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_ctr, c.d + c.L.ctr, 4 * (size_t)c.L.c_words, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * (size_t)c.D->d_words, hipMemcpyDeviceToHost, c.s));
    if (int32_t rc = stands_counters_fetch(c)) return rc;
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + W.h_whdr, c.d + W.whdr, 4 * (size_t)STANDS_H_STRIDE * S.S, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + W.h_order, c.d + W.order, 4 * (size_t)S.sumK, hipMemcpyDeviceToHost, c.s));
    BBP_HIP_TRY(ctx, hipMemcpyAsync(c.h + c.L.h_status, status + S.sumK, 4 * (size_t)S.rows, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}
static int32_t stands_commit_enqueue(const BestsCall& c) {
    const StandsCall& S = *c.stands;
    const StandingsLayout& W = *S.W;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_stands_commit, dim3((S.sumK + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, S.S, S.sumK, c.B, (const u32*)c.at(W.par), (const u32*)c.at(W.whdr),
                       (const u32*)c.at(W.order), (const u32*)c.at(c.L.win), (const u32*)c.at(c.D->ids), (const u32*)c.at(W.wserial), (const u32*)c.at(W.local));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// keys at base (the _dev form: the rows; else the staged keys {rows}) -> records, statuses, candidate counts, segments
static int32_t bests_segment_enqueue(const BestsCall& c, const u8* base, bool dev_rows, int32_t* status) {
    const BestsLayout& L = c.L;
    const u32 f = c.first(), n = c.B - f;  // <the keys of the offer's rows: the seed wrote the entry slots>
    const dim3 grid((c.B + BEST_T - 1) / BEST_T), block(BEST_T);
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_bests_keys, dim3((n + BEST_T - 1) / BEST_T), block, 0, c.s, n, base, dev_rows ? (const unsigned long long*)(c.d + L.rowoff) : nullptr,
                           (const u32*)c.at(L.rb), (const u32*)c.at(L.round_of) + f, (const u32*)c.at(L.floors), c.at(L.recs) + (size_t)RS_WORDS * f,
                           c.at(L.win) + (size_t)RS_WORDS * f, status + f, c.ctr(L.c_ncand));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (c.stands) {  // <a segment holds the candidates and the entry slots: its size into take, which the first plan overwrites>
        if (int32_t rc = stands_plan_enqueue(c, STANDS_PLAN_SEGMENTS, 0)) return rc;
    }
    if (int32_t rc = bests_scan_enqueue(c, c.stands ? L.c_take : L.c_ncand, L.c_seg, false)) return rc;
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_bests_place, grid, block, 0, c.s, c.B, (const u32*)c.at(L.recs), (const u32*)c.ctr(L.c_seg), c.ctr(L.c_fill), c.at(L.cand));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    return c.stands ? stands_enter_enqueue(c, status) : (int32_t)BBP_OK;
}

// the rows that take and off plan, out of the candidate records (finish: the winner records) -> sel
static int32_t bests_select_enqueue(const BestsCall& c, bool finish) {
    const BestsLayout& L = c.L;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_select, dim3(c.R), dim3(BESTS_T), 0, c.s, (const u32*)c.at(finish ? L.win : L.recs), (const u32*)c.at(L.cand),
                       (const u32*)c.ctr(L.c_seg), (const u32*)c.ctr(L.c_take), (const u32*)c.ctr(L.c_off), c.at(L.sel));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// take and off of step t (finish: of the winners), [the selection -> sel], the counters into the mirror
static int32_t bests_plan_enqueue(const BestsCall& c, u32 t, bool finish, bool bytes, bool select) {
    const BestsLayout& L = c.L;
    if (c.stands) {
        if (int32_t rc = stands_plan_enqueue(c, STANDS_PLAN_STEP, t)) return rc;
    } else {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        if (c.D)
            hipLaunchKernelGGL(k_bests_plan_distinct, dim3((c.R + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.R, t, c.K, c.tranche, finish ? 1u : 0u,
                               (const u32*)c.ctr(L.c_ncand), (const u32*)c.ctr(L.c_examined), (const u32*)c.dctr(c.D->d_dups),
                               (const u32*)c.dctr(c.D->d_settled), c.ctr(L.c_take), c.ctr(L.c_tranches));
        else
            hipLaunchKernelGGL(k_bests_plan, dim3((c.R + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.R, t, c.K, c.tranche, finish ? 1u : 0u,
                               (const u32*)c.ctr(L.c_ncand), (const u32*)c.ctr(L.c_examined), (const u32*)c.ctr(L.c_ok), c.ctr(L.c_take), c.ctr(L.c_tranches));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (int32_t rc = bests_scan_enqueue(c, L.c_take, L.c_off, bytes)) return rc;
    if (select)
        if (int32_t rc = bests_select_enqueue(c, finish)) return rc;
    BBP_HIP_TRY(c.ctx, hipMemcpyAsync(c.h + L.h_ctr, c.d + L.ctr, 4 * (size_t)L.c_words, hipMemcpyDeviceToHost, c.s));
    if (c.D) BBP_HIP_TRY(c.ctx, hipMemcpyAsync(c.h + c.D->h_dctr, c.d + c.D->dctr, 4 * (size_t)c.D->d_words, hipMemcpyDeviceToHost, c.s));
    return c.stands ? stands_counters_fetch(c) : (int32_t)BBP_OK;
}

static int32_t bests_mark_enqueue(const BestsCall& c, u32 n, const int32_t* tstat, int32_t* status) {
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_mark, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, n, (const u32*)c.at(c.L.sel), tstat, status, c.at(c.L.recs),
                       c.at(c.L.win), c.ctr(c.L.c_examined), c.ctr(c.L.c_ok));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// {one per bidder} behind the mark of a step of n rows: identities settled, holders' winner records opened, duplicates of running
// rounds dropped <the merge and the leave pass in the drop pass's place; t: the step, take: its rows per standing>
static int32_t bests_settle_enqueue(const BestsCall& c, u32 n, const int32_t* tstat, int32_t* status, u32 t = 0, const u32* take = nullptr) {
    const BestsLayout& L = c.L;
    const BestsDistinctLayout& D = *c.D;
    const u32 *sel = c.at(L.sel), *ids = c.at(D.ids), *round_of = c.at(L.round_of), mask = D.slots - 1;
    u32 *table = c.at(D.table), *flag = c.dctr(D.d_flag);
    const dim3 grid((n + BEST_T - 1) / BEST_T), block(BEST_T);
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
            hipLaunchKernelGGL(k_bests_settle, grid, block, 0, c.s, n, c.B, sel, tstat, (const u32*)c.at(L.recs), ids, round_of, table, mask, c.dctr(D.d_settled), flag);
        BBP_HIP_TRY(c.ctx, hipGetLastError());
        hipLaunchKernelGGL(k_bests_holders, grid, block, 0, c.s, n, c.B, sel, tstat, ids, round_of, (const u32*)table, mask, c.at(L.win), flag);
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (c.stands) return stands_merge_enqueue(c, t, take, status);
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_drop, dim3((c.B + BEST_T - 1) / BEST_T), block, 0, c.s, c.B, c.K, c.at(L.recs), ids, round_of, (const u32*)table, mask, status,
                       (const u32*)c.dctr(D.d_settled), c.dctr(D.d_dups), flag);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// the winners' pairs (nw of them, grouped by round as off says) and everything the host reads, into the mirror
static int32_t bests_pairs_enqueue(const BestsCall& c, u32 nw, const int32_t* status_to_fetch) {
    const BestsLayout& L = c.L;
    if (nw) {
        if (int32_t rc = best_pairs_enqueue(c.ctx, nw, c.at(L.sel), c.ctr(L.c_off + c.R), c.at(L.win), c.at(L.pairs), c.s)) return rc;
        BBP_HIP_TRY(c.ctx, hipMemcpyAsync(c.h + L.h_pairs, c.d + L.pairs, 4 * (size_t)BEST_PAIR_WORDS * nw, hipMemcpyDeviceToHost, c.s));
    }
    if (status_to_fetch) BBP_HIP_TRY(c.ctx, hipMemcpyAsync(c.h + L.h_status, status_to_fetch, 4 * (size_t)c.B, hipMemcpyDeviceToHost, c.s));
    return BBP_OK;
}

// What a call knows of every round between steps, held against the device's counters each time they arrive.  {One per bidder: the
// host cannot recount identities, so settled and dups are the device's, held to what the host can know -- settled[r] is at most the
// valid rows of r and never shrinks, dups never shrinks, examined + dups stays within the candidates.}
struct BestsTally {
    u32 R, K, tranche;
    bool distinct;
    std::vector<u32> nc, examined, ok, take, settled, dups;  // (settled, dups, running: the one-per-bidder calls only, otherwise empty)
    std::vector<u32> Ks, left;  // <an offer to many standings only: every standing's K, and the candidates that left by the bar>
    std::vector<char> running;  // round r contributed to the step planned last (all of them before step 0); a round that stopped stays stopped
    u32 n = 0;                  // the rows of the step planned last
    explicit BestsTally(const BestsCall& c)
        : R(c.R), K(c.K), tranche(c.tranche), distinct(c.D.has_value()), nc(R), examined(R), ok(R), take(R), settled(distinct ? R : 0),
          dups(settled.size()), running(settled.size(), 1) {
        if (c.stands) Ks = c.stands->K, left.assign(R, 0);
    }
    bool stands() const { return !Ks.empty(); }
    // the rows round r contributes to step t (finish: the winners it reports), from what the call holds of the device's counters
    u32 rows_of(u32 r, u32 t, bool finish) const {
        if (stands()) return finish ? 0 : stands_take(Ks[r], tranche, t, nc[r], examined[r], dups[r], left[r]);  // <no stop at K, no winners' selection>
        if (distinct) return finish ? bests_winners(K, settled[r]) : bests_take_distinct(K, tranche, t, nc[r], examined[r], dups[r], settled[r]);
        return finish ? bests_winners(K, ok[r]) : bests_take(K, tranche, t, nc[r], examined[r], ok[r]);
    }
    // the first counters: the candidate counts are the device's; B bounds them
    bool adopt_candidates(const BestsCall& c, std::string* why) {
        unsigned long long total = 0;
        for (u32 r = 0; r < R; r++) total += nc[r] = c.mirror(c.L.c_ncand)[r];
        if (total <= c.B - c.first() && c.mirror(c.L.c_seg)[R] == total + c.first()) return true;  // <a segment holds the entry slots too>
        return *why = std::string(c.family()) + "the device counted " + std::to_string(total) + " candidates among " + std::to_string(c.B) + " rows", false;
    }
    // The most rows step t can hold, from what a host form knows before the device has planned it.  It has counted the valid rows, so
    // this is the step's size.  {A bound only, before the device has counted the last step's identities: a valid row settles at least
    // one identity, the mirrored dups are a lower bound.  0: every round has stopped for sure.}
    u32 bound(u32 t) const {
        unsigned long long sum = 0;
        for (u32 r = 0; r < R; r++) {
            if (!distinct || stands())  // <dups and left as mirrored are lower bounds>
                sum += !distinct || running[r] ? rows_of(r, t, false) : 0;
            else if (running[r] && !(K && std::max(settled[r], ok[r] ? 1u : 0u) >= K))
                sum += bests_take_distinct(K, tranche, t, nc[r], examined[r], dups[r], 0);
        }
        return (u32)std::min<unsigned long long>(sum, 0xffffffffu);
    }
    // the winners at most, from the valid rows {before the device has counted the settled identities among them}
    u32 winners_bound() const {
        u32 sum = 0;
        for (u32 r = 0; r < R; r++) sum += bests_winners(K, ok[r]);
        return sum;
    }
    // the winners, from the counters a _dev form took over with the last plan
    u32 winners() const {
        u32 sum = 0;
        for (u32 r = 0; r < R; r++) sum += rows_of(r, 0, true);
        return sum;
    }
    // the counters that arrived with step t's plan (or the finish's) -> take, n.  ok_known: the host has counted the valid rows itself
    // (the host forms); otherwise the device's count is taken over where it can be true, and the plan is made from it.
    bool check(const BestsCall& c, u32 t, bool finish, bool ok_known, std::string* why) {
        const BestsLayout& L = c.L;
        if (c.D)
            if (const u32 flag = c.dmirror(c.D->d_flag)[0])
                return *why = std::string(c.family()) + "a bounded loop of the identity table ran out (flag " + std::to_string(flag) + ")", false;
        bool good = true;
        for (u32 r = 0; r < R && good; r++) {
            const u32 dok = c.mirror(L.c_ok)[r];
            good = c.mirror(L.c_ncand)[r] == nc[r] && c.mirror(L.c_examined)[r] == examined[r] && (ok_known ? dok == ok[r] : dok >= ok[r] && dok <= examined[r]);
            if (good && c.D) {
                const u32 ds = c.dmirror(c.D->d_settled)[r], dd = c.dmirror(c.D->d_dups)[r];
                good = ds >= settled[r] && ds <= dok && dd >= dups[r] && (unsigned long long)examined[r] + dd <= nc[r];
                if (good && stands()) {
                    const u32 dl = ((const u32*)(c.h + c.stands->W->h_sctr))[r];
                    good = dl >= left[r] && (unsigned long long)examined[r] + dd + dl <= nc[r];
                    if (good) left[r] = dl;
                }
                if (good) settled[r] = ds, dups[r] = dd;
            }
            if (good) ok[r] = dok;
        }
        if (good && stands() && finish) {  // <nothing was planned: every standing has stopped, no candidate is live>
            n = 0;
            for (u32 r = 0; r < R && good; r++) good = rows_of(r, 0, false) == 0, take[r] = 0;
        } else if (good) {
            n = 0;
            unsigned long long at = 0;
            for (u32 r = 0; r < R && good; r++) {
                take[r] = rows_of(r, t, finish);
                good = c.mirror(L.c_take)[r] == take[r] && c.mirror(L.c_off)[r] == at && (!c.D || finish || running[r] || take[r] == 0);
                at += take[r], n += take[r];
                if (c.D && !finish) running[r] = take[r] > 0;
            }
            good = good && c.mirror(L.c_off)[R] == n;
        }
        if (!good) *why = std::string(c.family()) + "the device's per-round counters at step " + std::to_string(t) + " are not what the call counted";
        return good;
    }
};

// after the finish has arrived (tally checked): every round's part of the pairs ranked, the counts delivered {the rows dropped}
static int32_t bests_deliver(const BestsCall& c, const BestsTally& ty, const u32* round_of, u32 steps, const BestsOut& o, std::string* why) {
    const u32* pairs = (const u32*)(c.h + c.L.h_pairs);
    u32 at = 0;
    for (u32 r = 0; r < c.R; r++) {
        const u32 nw = ty.take[r];
        for (u32 j = at; j < at + nw; j++) {
            const u32 i = pairs[(size_t)BEST_PAIR_WORDS * j + 8];
            if (i >= c.B || round_of[i] != r) return *why = std::string(c.family()) + "a winner of round " + std::to_string(r) + " is no row of it", BBP_ERR_INTERNAL;
        }
        best_rank_pairs(nw, pairs + (size_t)BEST_PAIR_WORDS * at, o.cap, o.best + (size_t)r * o.cap);
        o.n_best[r] = nw, o.n_candidates[r] = ty.nc[r], o.n_examined[r] = ty.examined[r];
        if (o.n_duplicates) o.n_duplicates[r] = ty.dups[r];
        at += nw;
    }
    if (o.n_steps) *o.n_steps = steps;
    return BBP_OK;
}
// <an offer to many standings, after its finish has arrived (tally checked): every working standing against the call -- at most K
// entries, every one a working row of that standing -- then the outputs: the call's rows among the entries, in rank order>
static int32_t stands_deliver(const BestsCall& c, const BestsTally& ty, const u32* round_of, u32 steps, const BestsOut& o, std::string* why) {
    const StandsCall& S = *c.stands;
    const u32 *whdr = (const u32*)(c.h + S.W->h_whdr), *order = (const u32*)(c.h + S.W->h_order);
    for (u32 s = 0; s < S.S; s++) {
        const u32 count = whdr[(size_t)STANDS_H_STRIDE * s + STAND_H_COUNT];
        bool ok = count <= S.K[s];
        for (u32 e = 0; ok && e < count; e++) {
            const u32 i = order[S.E[s] + e];
            ok = i < c.B && round_of[i] == s && (i >= S.sumK || (i >= S.E[s] && i - S.E[s] < S.K[s]));
        }
        if (!ok) return *why = std::string(c.family()) + "the working standing " + std::to_string(s) + " holds what is no row of it", BBP_ERR_INTERNAL;
        u32 ne = 0;
        for (u32 e = 0; e < count; e++) {
            const u32 i = order[S.E[s] + e];
            if (i < S.sumK) continue;
            if (ne < o.cap) o.best[(size_t)s * o.cap + ne] = i - S.sumK;
            ne++;
        }
        o.n_best[s] = ne, o.n_candidates[s] = ty.nc[s], o.n_examined[s] = ty.examined[s], o.n_duplicates[s] = ty.dups[s];
    }
    if (o.n_steps) *o.n_steps = steps;
    return BBP_OK;
}
// a step cannot run more often than a tranche can double
constexpr u32 BESTS_MAX_STEPS = 40;

// The host forms with R > 1 on ONE device's context (c.ctx).  fill(dst): the B x c.staged_row() bytes into the pinned staging area
// (the key {score || z_img} of every row); verdicts(n, sel, take, st): the statuses of the step's rows sel[0..n), grouped by round in
// ascending order, take[r] of round r -- called with no lock of the device held.  One submission in front reads the candidate counts;
// one per step carries the verdicts of the step before up, then mark {settle, holders, drop}, plan, scan and select, and brings the
// counters down with sel up to the room the host has for the step.  The host counts the valid rows itself, so it knows the step's
// size before the device has planned it, and the finish travels with the last marks.  {The device plans from its own counters: the host
// knows the verdicts, not the identities, so the room is a bound.  The finish travels with the last marks when the host knows that every
// round has stopped (always with K <= 1: a valid row settles an identity), and otherwise follows the submission whose plan held no row.}
template <class Fill, class Verdicts>
static int32_t bests_run_host(BestsCall& c, const u32* round_of, Fill&& fill, Verdicts&& verdicts, const uint8_t* floors, const BestsOut& out, int32_t* status) {
    bbp_ctx* const dev = c.ctx;
    std::lock_guard<std::mutex> call(dev->best_mu);
    const BestsLayout& L = c.L;
    BestsTally ty(c);
    std::vector<int32_t> st;
    std::string why;
    const u32 first = c.first();
    std::vector<uint8_t> stand_floors;
    if (c.stands) {  // <the floor every standing screens by, from the standing as its last commit left it>
        stand_floors.resize(32 * (size_t)c.R);
        for (u32 s = 0; s < c.R; s++) {
            const bbp_ctx::Standing& m = *c.stands->meta[s];
            u32 f[8];
            stand_screen_floor(m.floor, m.count == m.K, m.bar, f);
            for (int b = 0; b < 32; b++) stand_floors[32 * (size_t)s + b] = (uint8_t)(f[b >> 2] >> (8 * (b & 3)));
        }
        floors = stand_floors.data();
    }
    auto fail = [&](const std::string& w, int32_t rc) {
        api_guard(dev, [&]() -> int32_t { return dev->err = w, rc; });
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
        return e == hipSuccess ? (int32_t)BBP_OK : fail(std::string(c.family()) + hipGetErrorString(e), BBP_ERR_DEVICE);
    };
    int32_t rc = submit([&]() -> int32_t {
        int32_t r;
        if ((r = bests_open(c, floors, round_of, nullptr, nullptr))) return r;
        if (c.stands && (r = stands_seed_enqueue(c, (int32_t*)c.at(L.status)))) return r;
        const size_t skip = c.staged_row() * first;  // <the entry slots are not staged: the seed wrote them>
        fill(c.h + c.h_staged() + skip);
        BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + c.staged() + skip, c.h + c.h_staged() + skip, c.staged_row() * (c.B - first), hipMemcpyHostToDevice, c.s));
        if (c.D && (r = bests_ids_enqueue(c, c.d + c.staged() + skip, false))) return r;  // (which says where each staged row starts)
        if ((r = bests_segment_enqueue(c, c.d + c.staged() + skip, c.D.has_value(), (int32_t*)c.at(L.status)))) return r;  // <and the leave pass in front of step 0>
        BBP_HIP_TRY(dev, hipMemcpyAsync(c.h + L.h_ctr, c.d + L.ctr, 4 * (size_t)L.c_words, hipMemcpyDeviceToHost, c.s));
        return BBP_OK;
    });
    if (rc) return rc;
    if (!ty.adopt_candidates(c, &why)) return fail(why, BBP_ERR_INTERNAL);
    u32 pending = 0, steps = 0;
    bool finish = false;
    for (u32 t = 0;; t++) {
        const u32 room = std::min(ty.bound(t), c.B);
        finish = finish || room == 0 || t >= BESTS_MAX_STEPS;
        const u32 nw = finish && !c.stands ? std::min(ty.winners_bound(), c.B) : 0;
        rc = submit([&]() -> int32_t {
            int32_t r;
            if (pending) {
                const int32_t* tstat = (const int32_t*)c.at(L.tstat);
                memcpy(c.h + L.h_tstat, st.data(), 4 * (size_t)pending);
                BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + L.tstat, c.h + L.h_tstat, 4 * (size_t)pending, hipMemcpyHostToDevice, c.s));
                if ((r = bests_mark_enqueue(c, pending, tstat, (int32_t*)c.at(L.status)))) return r;
                if (c.D && (r = bests_settle_enqueue(c, pending, tstat, (int32_t*)c.at(L.status), t - 1, ty.take.data()))) return r;
            }
            if (c.stands && finish) return stands_finish_enqueue(c, (const int32_t*)c.at(L.status));
            if ((r = bests_plan_enqueue(c, t, finish, false, finish ? nw > 0 : true))) return r;
            if (finish) return bests_pairs_enqueue(c, nw, (const int32_t*)c.at(L.status));
            BBP_HIP_TRY(dev, hipMemcpyAsync(c.h + L.h_sel, c.d + L.sel, 4 * (size_t)room, hipMemcpyDeviceToHost, c.s));
            return BBP_OK;
        });
        if (rc) return rc;
        pending = 0;
        if (!ty.check(c, t, finish, true, &why)) return fail(why, BBP_ERR_INTERNAL);
        if (finish) {
            if (ty.n > nw) return fail(std::string(c.family()) + "more winners than valid rows", BBP_ERR_INTERNAL);
            break;
        }
        const u32 n = ty.n;
        if (n > room) return fail(std::string(c.family()) + "a step of " + std::to_string(n) + " rows, above the " + std::to_string(room) + " it can hold", BBP_ERR_INTERNAL);
        if (n == 0) {  // {every round has stopped, which only the device could know: the finish follows}
            finish = true;
            continue;
        }
        steps++;
        st.assign(n, BBP_ERR_INTERNAL);
        if ((rc = verdicts(n, (const u32*)(c.h + L.h_sel), ty.take.data(), st.data()))) return rc;
        u32 j = 0;
        for (u32 r = 0; r < c.R; r++)
            for (u32 e = j + ty.take[r]; j < e; j++) ty.examined[r]++, ty.ok[r] += st[j] == BBP_OK;
        pending = n;
    }
    if (c.stands) {  // <the host's checks first, then the one commit, then the host's records of what was committed>
        if ((rc = stands_deliver(c, ty, round_of, steps, out, &why))) return fail(why, rc);
        if ((rc = submit([&]() -> int32_t { return stands_commit_enqueue(c); }))) return rc;
        for (u32 s = 0; s < c.R; s++)
            stand_record_commit(*c.stands->meta[s], (const u32*)(c.h + c.stands->W->h_whdr) + (size_t)STANDS_H_STRIDE * s, c.stands->n_rows[s]);
    } else if ((rc = bests_deliver(c, ty, round_of, steps, out, &why)))
        return fail(why, rc);
    memcpy(status, c.h + L.h_status, 4 * (size_t)(c.B - first));
    return BBP_OK;
}

// byte offset of every row of a rounds call (rows packed back to back in request order), the total at [B]
static std::vector<unsigned long long> bests_row_offsets(const u32* round_Ns, u32 B, const u32* round_of) {
    std::vector<unsigned long long> off((size_t)B + 1);
    unsigned long long at = 0;
    for (u32 i = 0; i < B; i++) off[i] = at, at += round_row_bytes(round_Ns[round_of[i]]);
    off[B] = at;
    return off;
}
// round_of of a step's rows: grouped by round in ascending order, take[r] of round r
static void bests_step_rounds(u32 R, const u32* take, std::vector<u32>& step_round_of) {
    step_round_of.clear();
    for (u32 r = 0; r < R; r++) step_round_of.insert(step_round_of.end(), take[r], r);
}

// A step of a _dev form (n rows in sel, take[r] of round r; rb: the row size of every round): the rows packed by round on the device and
// verified, in engine calls of at most BBP_HOST_CHUNK_VERIFY rows -> tstat
static int32_t bests_step_verify_dev(const BestsCall& c, const u32* round_Ns, const u8* rounds_dev, const std::vector<u32>& rb, const u32* take, u32 n,
                                     const u8* rows_dev, const u8* entropy_dev, int32_t* tstat, std::vector<u32>& step_round_of) {
    bbp_ctx* const ctx = c.ctx;
    const BestsLayout& L = c.L;
    bests_step_rounds(c.R, take, step_round_of);
    std::vector<unsigned long long> at((size_t)n + 1, 0);
    for (u32 j = 0; j < n; j++) at[j + 1] = at[j] + rb[step_round_of[j]];
    const u32 part = std::min(n, host_chunk_verify());
    unsigned long long most = 0;
    for (u32 first = 0; first < n; first += part) most = std::max(most, at[std::min(n, first + part)] - at[first]);
    const size_t ent_off = align256((size_t)most + 4);
    if (int32_t rc = dev_reserve(ctx, ctx->best_rows, ent_off + align256(32 * (size_t)part))) return rc;
    u8* g = (u8*)ctx->best_rows.p;
    for (u32 first = 0; first < n; first += part) {
        const u32 m = std::min(part, n - first);
        {
            ScopedEvent ev(ctx, TAG_SELECT, c.s);
            hipLaunchKernelGGL(k_bests_gather, dim3(m), dim3(BEST_GATHER_T), 0, c.s, n, first, at[first], (const u32*)c.at(L.sel), (const u32*)c.at(L.round_of),
                               (const u32*)c.at(L.rb), (const u32*)c.ctr(L.c_off), (const unsigned long long*)c.offb(),
                               (const unsigned long long*)(c.d + L.rowoff), rows_dev, entropy_dev, g, g + ent_off);
            BBP_HIP_TRY(ctx, hipGetLastError());
        }
        if (int32_t rc = verify_batch_agg_dev(ctx, VerifyRows::of_rounds(m, c.R, round_Ns, rounds_dev, step_round_of.data() + first), BBP_AGG_GROUP_DEFAULT, g,
                                              g + ent_off, tstat + first, c.s, nullptr))
            return rc;
    }
    return BBP_OK;
}

// The _dev form with R > 1, everything on c.s, the context lock held throughout.  It synchronises c.s after the segments are built (the
// candidate counts, and step 0's plan), once per step (the counters behind the mark, and the next step's plan: the host needs
// take[] to build the step's round_of {behind settle, holders and drop}) and once to deliver.
static int32_t bests_run_dev(BestsCall& c, const u32* round_Ns, const u8* rounds_dev, const u32* round_of, const u8* rows_dev, const u8* entropy_dev,
                             const uint8_t* floors, const BestsOut& out, int32_t* status) {
    bbp_ctx* const ctx = c.ctx;
    std::lock_guard<std::mutex> call(ctx->best_mu);
    return api_guard(ctx, [&]() -> int32_t {
        const BestsLayout& L = c.L;
        int32_t rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const std::vector<unsigned long long> rowoff = bests_row_offsets(round_Ns, c.B, round_of);
        std::vector<u32> rb(c.R), step_round_of;
        for (u32 r = 0; r < c.R; r++) rb[r] = (u32)round_row_bytes(round_Ns[r]);
        if ((rc = bests_open(c, floors, round_of, rowoff.data(), rb.data())) || (c.D && (rc = bests_ids_enqueue(c, rows_dev, true))) ||
            (rc = bests_segment_enqueue(c, rows_dev, true, status)) || (rc = bests_plan_enqueue(c, 0, false, true, false)))
            return rc;
        BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));
        BestsTally ty(c);
        std::string why;
        if (!ty.adopt_candidates(c, &why)) return ctx->err = why, BBP_ERR_INTERNAL;
        u32 steps = 0;
        int32_t* tstat = (int32_t*)c.at(L.tstat);
        for (u32 t = 0; t < BESTS_MAX_STEPS; t++) {
            if (!ty.check(c, t, false, false, &why)) return ctx->err = why, BBP_ERR_INTERNAL;
            const u32 n = ty.n;
            if (n == 0) break;
            steps++;
            if ((rc = bests_select_enqueue(c, false))) return rc;
            if ((rc = bests_step_verify_dev(c, round_Ns, rounds_dev, rb, ty.take.data(), n, rows_dev, entropy_dev, tstat, step_round_of))) return rc;
            if ((rc = bests_mark_enqueue(c, n, tstat, status)) || (c.D && (rc = bests_settle_enqueue(c, n, tstat, status))) ||
                (rc = bests_plan_enqueue(c, t + 1, false, true, false)))
                return rc;
            BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));
            for (u32 r = 0; r < c.R; r++) ty.examined[r] += ty.take[r];
        }
        // the last plan that arrived held no row (or the step bound is reached, and the valid rows of the last step are the device's
        // count): the valid rows {the settled identities} are known, the winners can be planned
        if (!c.D)
            for (u32 r = 0; r < c.R; r++) ty.ok[r] = std::min(c.mirror(L.c_ok)[r], ty.examined[r]);
        const u32 nw = ty.winners();
        if ((rc = bests_plan_enqueue(c, 0, true, false, nw > 0)) || (rc = bests_pairs_enqueue(c, nw, nullptr))) return rc;
        BBP_HIP_TRY(ctx, hipStreamSynchronize(c.s));
        if (!ty.check(c, 0, true, true, &why)) return ctx->err = why, BBP_ERR_INTERNAL;
        if (c.D && ty.n != nw) return ctx->err = std::string(c.family()) + "the winners are not the settled identities", BBP_ERR_INTERNAL;
        if ((rc = bests_deliver(c, ty, round_of, steps, out, &why))) ctx->err = why;
        return rc;
    });
}

// screening of the numbers shared by the three forms (rounds_best.h rounds_best_screen: the same checks in the same order)
static int32_t bests_screen(bbp_ctx* ctx, const char* what, u32 R, const u32* round_Ns, u32 B, const u32* round_of, bool* done) {
    const int32_t screened = rounds_best_screen(R, round_Ns, B, round_of, done);
    if (!screened) return BBP_OK;
    return api_guard(ctx, [&]() -> int32_t {
        for (u32 r = 0; r < R && R <= BBP_BEST_MAX_ROUNDS; r++)
            if (round_Ns[r] == 0 || (screened == BBP_ERR_GENS_LEN && round_Ns[r] > BBP_MAX_ITEMS)) return check_n(ctx, round_Ns[r]);  // (names the list length)
        ctx->err = std::string(what) + ": R is 0 or above BBP_BEST_MAX_ROUNDS, more than BBP_SELECT_MAX_BIDS rows, or round_of names no round";
        return screened;
    });
}
static void bests_zero(u32 R, const BestsOut& o) {
    for (u32 r = 0; r < R && R <= BBP_BEST_MAX_ROUNDS; r++) {
        o.n_best[r] = o.n_candidates[r] = o.n_examined[r] = 0;
        if (o.n_duplicates) o.n_duplicates[r] = 0;
    }
    if (o.n_steps) *o.n_steps = 0;
}
static const uint8_t BESTS_ZERO_FLOOR[32] = {};

// A step of a public host form: the rows sel[0..n), grouped by round in ascending order (take[r] of round r), gathered from the CALLER's
// memory and verified in one rounds call through bbp_verify_rounds_aggregated's own path -> st
struct BestsHostRows {
    bbp_ctx* ctx;
    const char* family;
    u32 R, B;
    const u32 *round_Ns, *round_of;
    const uint8_t *rounds, *rows;
    std::vector<unsigned long long> rowoff;
    std::vector<uint8_t> picked;
    std::vector<u32> step_round_of;
    u32 first = 0;  // <sel holds working rows: row sel[j] - first of the call>
    int32_t verify(u32 n, const u32* sel, const u32* take, int32_t* st) {
        bests_step_rounds(R, take, step_round_of);
        picked.clear();
        for (u32 j = 0; j < n; j++) {
            const u32 i = sel[j] - first;
            if (sel[j] < first || i >= B || round_of[i] != step_round_of[j])
                return api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string(family) + "a selected row is no row of its round", BBP_ERR_INTERNAL; });
            picked.insert(picked.end(), rows + rowoff[i], rows + rowoff[i + 1]);
        }
        return verify_host(ctx, VerifyRows::of_rounds(n, R, round_Ns, rounds, step_round_of.data()), picked.data(), st, BBP_AGG_GROUP_DEFAULT, nullptr);
    }
};

// The public host forms behind their screening.  Staged: the score of every row {score || z_img: adjacent, a row's last 64 bytes}; a
// step comes from the CALLER's memory.  On a pool, everything but the verification is member 0's.  One round: the single-round driver.
static int32_t bests_public_host(bbp_ctx* ctx, u32 R, const u32* round_Ns, const uint8_t* rounds, u32 B, const u32* round_of, const uint8_t* rows,
                                 const uint8_t* floors, u32 K, u32 tranche, bool distinct, const BestsOut& out, int32_t* status) {
    if (R == 1) return best_public_host(ctx, round_Ns[0], rounds, B, rows, floors ? floors : BESTS_ZERO_FLOOR, K, tranche, distinct, out.one_round(), status);
    return no_throw_ctx(ctx, [&]() -> int32_t {
        bbp_ctx* const dev = is_pool(ctx) ? ctx->members[0] : ctx;
        BestsCall c(dev, R, B, K, tranche, dev->stream, true, distinct);
        BestsHostRows hr{ctx, c.family(), R, B, round_Ns, round_of, rounds, rows, bests_row_offsets(round_Ns, B, round_of), {}, {}};
        const size_t w = c.staged_row();
        auto fill = [&](u8* dst) {
            for (u32 i = 0; i < B; i++) memcpy(dst + w * i, rows + hr.rowoff[i + 1] - 64, w);
        };
        auto verdicts = [&](u32 n, const u32* sel, const u32* take, int32_t* st) -> int32_t { return hr.verify(n, sel, take, st); };
        const int32_t rc = bests_run_host(c, round_of, fill, verdicts, floors, out, status);
        if (rc && dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
        return rc;
    });
}

// The test hooks behind their NULL checks: the shipped kernels on caller-made keys {ids} and verdicts.  ids == nullptr: the plain
// call; table_log2 is screened for the one-per-bidder call only.
static int32_t bests_hook(bbp_ctx* ctx, const char* what, u32 R, u32 B, const u32* round_of, const uint8_t* keys, const uint8_t* ids,
                          const int32_t* verdicts, const uint8_t* floors, u32 K, u32 tranche, u32 table_log2, const BestsOut& out, int32_t* status) {
    if (is_pool(ctx)) return pool_reject(ctx, what);
    return no_throw_ctx(ctx, [&]() -> int32_t {
        const std::string name(what);
        u32 n_ok;
        if (R == 0 || R > BBP_BEST_MAX_ROUNDS) return best_hook_refuse(ctx, name + ": R is 0 or above BBP_BEST_MAX_ROUNDS");
        if (int32_t rc = best_hook_screen(ctx, what, B, verdicts, &n_ok)) return rc;
        if (!round_of && R > 1) return best_hook_refuse(ctx, name + ": round_of may be NULL with one round only");
        for (u32 i = 0; round_of && i < B; i++)
            if (round_of[i] >= R) return best_hook_refuse(ctx, name + ": round_of names a round beyond R");
        if (ids && (table_log2 > BEST_TABLE_LOG2_MAX || (table_log2 && (1ull << table_log2) <= n_ok)))
            return best_hook_refuse(ctx, name + ": table_log2 is above 21, or the table has no slot more than there are BBP_OK verdicts");
        bests_zero(R, out);
        if (R == 1) return best_hook_host(ctx, B, keys, ids, verdicts, floors ? floors : BESTS_ZERO_FLOOR, K, tranche, table_log2, out.one_round(), status);
        const size_t w = ids ? 64 : 32;
        auto fill = [&](u8* dst) {
            for (u32 i = 0; i < B; i++) {
                memcpy(dst + w * i, keys + 32 * (size_t)i, 32);
                if (ids) memcpy(dst + w * i + 32, ids + 32 * (size_t)i, 32);
            }
        };
        BestsCall c(ctx, R, B, K, tranche, ctx->stream, true, ids != nullptr, table_log2);
        auto read = [&](u32 n, const u32* sel, const u32*, int32_t* st) -> int32_t {
            for (u32 j = 0; j < n; j++) st[j] = sel[j] < B ? verdicts[sel[j]] : (int32_t)BBP_ERR_INTERNAL;
            return BBP_OK;
        };
        return bests_run_host(c, round_of, fill, read, floors, out, status);
    });
}

// The _dev forms behind their screening.  One round: the single-round driver.
static int32_t bests_public_dev(bbp_ctx* ctx, u32 R, const u32* round_Ns, const void* rounds_dev, u32 B, const u32* round_of, const void* rows_dev,
                                const void* entropy_dev, const uint8_t* floors, u32 K, u32 tranche, bool distinct, const BestsOut& out, void* status_dev,
                                void* stream) {
    return no_throw_ctx(ctx, [&]() -> int32_t {
        if (R == 1)
            return best_public_dev(ctx, round_Ns[0], rounds_dev, B, rows_dev, entropy_dev, floors ? floors : BESTS_ZERO_FLOOR, K, tranche, distinct, out.one_round(),
                                   status_dev, stream);
        BestsCall c(ctx, R, B, K, tranche, pick_stream(ctx, stream), false, distinct);
        return bests_run_dev(c, round_Ns, (const u8*)rounds_dev, round_of, (const u8*)rows_dev, (const u8*)entropy_dev, floors, out, (int32_t*)status_dev);
    });
}

extern "C" int32_t bbp_verify_rounds_best(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                                          const uint8_t* rows, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out,
                                          uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_steps, int32_t* status) {
    if (!ctx || !round_Ns || !rounds || !rows || !n_best || !n_candidates || !n_examined || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    const BestsOut out{cap, best_out, n_best, n_candidates, n_examined, n_steps};
    bests_zero(R, out);
    bool done;
    if (int32_t rc = bests_screen(ctx, "bbp_verify_rounds_best", R, round_Ns, B, round_of, &done)) return rc;
    if (done) return BBP_OK;
    return bests_public_host(ctx, R, round_Ns, rounds, B, round_of, rows, floors, K, tranche, false, out, status);
}

// Test hook: the shipped kernels of rounds_best.h on caller-made keys and verdicts.  Synchronises.
extern "C" int32_t bbp_debug_rounds_best(bbp_ctx* ctx, uint32_t R, uint32_t B, const uint32_t* round_of, const uint8_t* keys, const int32_t* verdicts,
                                         const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                         uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_steps, int32_t* status) {
    if (!ctx || !keys || !verdicts || !n_best || !n_candidates || !n_examined || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    return bests_hook(ctx, "bbp_debug_rounds_best", R, B, round_of, keys, nullptr, verdicts, floors, K, tranche, 0,
                      BestsOut{cap, best_out, n_best, n_candidates, n_examined, n_steps}, status);
}

extern "C" int32_t bbp_verify_rounds_best_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B, const uint32_t* round_of,
                                              const void* rows_dev, const void* entropy_dev, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap,
                                              uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_steps,
                                              void* status_dev, void* stream) {
    if (!ctx || !round_Ns || !rounds_dev || !rows_dev || !entropy_dev || !n_best || !n_candidates || !n_examined || !status_dev || (cap && !best_out))
        return BBP_ERR_BAD_ARG;
    const BestsOut out{cap, best_out, n_best, n_candidates, n_examined, n_steps};
    bests_zero(R, out);
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_verify_rounds_best_dev");
    bool done;
    if (int32_t rc = bests_screen(ctx, "bbp_verify_rounds_best_dev", R, round_Ns, B, round_of, &done)) return rc;
    if (done) return BBP_OK;
    return bests_public_dev(ctx, R, round_Ns, rounds_dev, B, round_of, rows_dev, entropy_dev, floors, K, tranche, false, out, status_dev, stream);
}

// ---- best proofs of many rounds, one per bidder (include/bbp.h; rules and kernels: rounds_best_distinct.h) ---------------------------
// The calls above with an identity table: the same drivers over a BestsCall that has one.
extern "C" int32_t bbp_verify_rounds_best_distinct(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B,
                                                   const uint32_t* round_of, const uint8_t* rows, const uint8_t* floors, uint32_t K, uint32_t tranche,
                                                   uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                                                   uint32_t* n_duplicates, uint32_t* n_steps, int32_t* status) {
    if (!ctx || !round_Ns || !rounds || !rows || !n_best || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    const BestsOut out{cap, best_out, n_best, n_candidates, n_examined, n_steps, n_duplicates};
    bests_zero(R, out);
    bool done;
    if (int32_t rc = bests_screen(ctx, "bbp_verify_rounds_best_distinct", R, round_Ns, B, round_of, &done)) return rc;
    if (done) return BBP_OK;
    return bests_public_host(ctx, R, round_Ns, rounds, B, round_of, rows, floors, K, tranche, true, out, status);
}

// Test hook: the shipped kernels of rounds_best_distinct.h on caller-made keys, ids and verdicts.  Synchronises.
extern "C" int32_t bbp_debug_rounds_best_distinct(bbp_ctx* ctx, uint32_t R, uint32_t B, const uint32_t* round_of, const uint8_t* keys, const uint8_t* ids,
                                                  const int32_t* verdicts, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap,
                                                  uint32_t table_log2, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                                                  uint32_t* n_duplicates, uint32_t* n_steps, int32_t* status) {
    if (!ctx || !keys || !ids || !verdicts || !n_best || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !best_out)) return BBP_ERR_BAD_ARG;
    return bests_hook(ctx, "bbp_debug_rounds_best_distinct", R, B, round_of, keys, ids, verdicts, floors, K, tranche, table_log2,
                      BestsOut{cap, best_out, n_best, n_candidates, n_examined, n_steps, n_duplicates}, status);
}

extern "C" int32_t bbp_verify_rounds_best_distinct_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B,
                                                       const uint32_t* round_of, const void* rows_dev, const void* entropy_dev, const uint8_t* floors,
                                                       uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                                       uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, uint32_t* n_steps,
                                                       void* status_dev, void* stream) {
    if (!ctx || !round_Ns || !rounds_dev || !rows_dev || !entropy_dev || !n_best || !n_candidates || !n_examined || !n_duplicates || !status_dev ||
        (cap && !best_out))
        return BBP_ERR_BAD_ARG;
    const BestsOut out{cap, best_out, n_best, n_candidates, n_examined, n_steps, n_duplicates};
    bests_zero(R, out);
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_verify_rounds_best_distinct_dev");
    bool done;
    if (int32_t rc = bests_screen(ctx, "bbp_verify_rounds_best_distinct_dev", R, round_Ns, B, round_of, &done)) return rc;
    if (done) return BBP_OK;
    return bests_public_dev(ctx, R, round_Ns, rounds_dev, B, round_of, rows_dev, entropy_dev, floors, K, tranche, true, out, status_dev, stream);
}

// ---- standings of many rounds (include/bbp.h; rules and kernels: standings.h) -----------------------------------------------------------
// One offer to S open standings: the host driver above over the W = sum K + B working rows, the standings as its rounds.  The standings
// of a handle live on ONE device's context (a pool: member 0).  One standing: the single-standing driver of capi_best.hip.
static void stands_zero(u32 S, const BestsOut& o) {
    for (u32 s = 0; s < S && S <= BBP_STANDING_MAX_OPEN; s++) o.n_best[s] = o.n_candidates[s] = o.n_examined[s] = o.n_duplicates[s] = 0;
    if (o.n_steps) *o.n_steps = 0;
}
// the screening both forms share, in the header's order behind the NULL checks; *done: the call ends here with BBP_OK
static int32_t stands_screen(bbp_ctx* ctx, const char* what, u32 S, const u32* standings, u32 B, const u32* standing_of, bool* done) {
    const std::string name(what);
    *done = false;
    if (S == 0 || S > BBP_STANDING_MAX_OPEN) return stand_refuse(ctx, name + ": S is 0 or above BBP_STANDING_MAX_OPEN");
    {
        bbp_ctx* const dev = stand_dev(ctx);
        std::lock_guard<std::mutex> call(dev->best_mu);
        for (u32 s = 0; s < S; s++)
            if (!stand_find(dev, standings[s])) return stand_refuse(ctx, name + ": no open standing has the handle standings[" + std::to_string(s) + "]");
    }
    for (u32 s = 0; s < S; s++)
        for (u32 q = 0; q < s; q++)
            if (standings[q] == standings[s]) return stand_refuse(ctx, name + ": a standing is named twice");
    if (B > BBP_SELECT_MAX_BIDS) return stand_refuse(ctx, name + ": more than BBP_SELECT_MAX_BIDS rows");
    if (B == 0) return *done = true, BBP_OK;
    for (u32 i = 0; standing_of && i < B; i++)
        if (standing_of[i] >= S) return stand_refuse(ctx, name + ": standing_of names a standing beyond S");
    return BBP_OK;
}
// both forms behind their screening, S > 1: the call built and run.  run(c, S): the form's fill and verdicts, handed to bests_run_host.
template <class Run>
static int32_t stands_offer(bbp_ctx* ctx, u32 S, const u32* standings, u32 B, const u32* standing_of, u32 tranche, Run&& run) {
    bbp_ctx* const dev = stand_dev(ctx);
    StandsCall SC(dev, S, standings, B, standing_of);
    const u32 W = SC.sumK + B;
    BestsCall c(dev, S, W, 0, tranche, dev->stream, true, true);
    SC.W.emplace(*c.D, S, SC.sumK, B);
    c.stands = &SC;
    std::vector<u32> round_of(W);  // the working round_of
    for (u32 s = 0; s < S; s++) std::fill(round_of.begin() + SC.E[s], round_of.begin() + SC.E[s] + SC.K[s], s);
    std::copy(standing_of, standing_of + B, round_of.begin() + SC.sumK);
    const int32_t rc = run(c, SC, round_of.data());
    if (rc && dev != ctx) api_guard(ctx, [&]() -> int32_t { return ctx->err = tls_error(), rc; });
    return rc;
}

extern "C" int32_t bbp_standings_offer(bbp_ctx* ctx, uint32_t S, const uint32_t* standings, uint32_t B, const uint32_t* standing_of, const uint8_t* rows,
                                       uint32_t tranche, uint32_t cap, uint32_t* entered_out, uint32_t* n_entered, uint32_t* n_candidates, uint32_t* n_examined,
                                       uint32_t* n_duplicates, uint32_t* n_steps, int32_t* status) {
    if (!ctx || !standings || !rows || !n_entered || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !entered_out) || (!standing_of && S != 1))
        return BBP_ERR_BAD_ARG;
    return no_throw_ctx(ctx, [&]() -> int32_t {
        const BestsOut out{cap, entered_out, n_entered, n_candidates, n_examined, n_steps, n_duplicates};
        stands_zero(S, out);
        bool done;
        if (int32_t rc = stands_screen(ctx, "bbp_standings_offer", S, standings, B, standing_of, &done)) return rc;
        if (done) return BBP_OK;
        if (S == 1) return stand_public_host(ctx, "bbp_standings_offer", standings[0], B, rows, tranche, out.one_round(), status);
        return stands_offer(ctx, S, standings, B, standing_of, tranche, [&](BestsCall& c, StandsCall& SC, const u32* round_of) -> int32_t {
            std::vector<u32> Ns(S);
            std::vector<uint8_t> rounds;
            for (u32 s = 0; s < S; s++) Ns[s] = SC.meta[s]->N, rounds.insert(rounds.end(), SC.meta[s]->round.begin(), SC.meta[s]->round.end());
            BestsHostRows hr{ctx, c.family(), S, B, Ns.data(), standing_of, rounds.data(), rows, bests_row_offsets(Ns.data(), B, standing_of), {}, {}, SC.sumK};
            auto fill = [&](u8* dst) {
                for (u32 i = 0; i < B; i++) memcpy(dst + 64 * (size_t)i, rows + hr.rowoff[i + 1] - 64, 64);
            };
            auto verdicts = [&](u32 n, const u32* sel, const u32* take, int32_t* st) -> int32_t { return hr.verify(n, sel, take, st); };
            return bests_run_host(c, round_of, fill, verdicts, nullptr, out, status);
        });
    });
}

// Test hook: an offer of caller-made keys, ids and verdicts through the shipped kernels against the standings' states.  Synchronises.
extern "C" int32_t bbp_debug_standings_offer(bbp_ctx* ctx, uint32_t S, const uint32_t* standings, uint32_t B, const uint32_t* standing_of, const uint8_t* keys,
                                             const uint8_t* ids, const int32_t* verdicts, uint32_t tranche, uint32_t cap, uint32_t* entered_out,
                                             uint32_t* n_entered, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, uint32_t* n_steps,
                                             int32_t* status) {
    if (!ctx || !standings || !keys || !ids || !verdicts || !n_entered || !n_candidates || !n_examined || !n_duplicates || !status || (cap && !entered_out) ||
        (!standing_of && S != 1))
        return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_standings_offer");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        const BestsOut out{cap, entered_out, n_entered, n_candidates, n_examined, n_steps, n_duplicates};
        stands_zero(S, out);
        bool done;
        if (int32_t rc = stands_screen(ctx, "bbp_debug_standings_offer", S, standings, B, standing_of, &done)) return rc;
        if (done) return BBP_OK;
        u32 n_ok;
        if (int32_t rc = best_hook_screen(ctx, "bbp_debug_standings_offer", B, verdicts, &n_ok)) return rc;
        if (S == 1) return stand_hook_host(ctx, "bbp_debug_standings_offer", standings[0], B, keys, ids, verdicts, tranche, out.one_round(), status);
        return stands_offer(ctx, S, standings, B, standing_of, tranche, [&](BestsCall& c, StandsCall& SC, const u32* round_of) -> int32_t {
            auto fill = [&](u8* dst) {
                for (u32 i = 0; i < B; i++) memcpy(dst + 64 * (size_t)i, keys + 32 * (size_t)i, 32), memcpy(dst + 64 * (size_t)i + 32, ids + 32 * (size_t)i, 32);
            };
            auto read = [&](u32 n, const u32* sel, const u32*, int32_t* st) -> int32_t {
                for (u32 j = 0; j < n; j++) st[j] = sel[j] >= SC.sumK && sel[j] - SC.sumK < B ? verdicts[sel[j] - SC.sumK] : (int32_t)BBP_ERR_INTERNAL;
                return BBP_OK;
            };
            return bests_run_host(c, round_of, fill, read, nullptr, out, status);
        });
    });
}
