// What the five C-API units share (DESIGN.md "C API units"); included by them and by nothing else:
//   capi_prove.hip   everything that proves: witness, entropy, checked proving, the host and device prove calls, rounds, selection
//   capi_best.hip    best proofs of one round, plain and one per bidder; standings
//   capi_bests.hip   best proofs of many rounds; one offer to many standings
//   capi_verify.hip  every verify entry point and the host verify path
//   capi_ctx.hip     error slots, sizes, bbp_reserve, settings, debug hooks, profiling
// Declarations only -- each function is defined once, in the unit named above it -- except the two exception barriers, SlotLease and
// one-line accessors.  A helper that one unit alone uses is a `static` of that unit and does not appear here.
// Kernels: every kernel is compiled by exactly one unit.  round_bids.h, round_select.h and round_best.h are also read by other units
// for their host-side rules (round_standing.h: with round_best.h's), so their kernels sit behind BBP_ROUND_BIDS_KERNELS / BBP_ROUND_SELECT_KERNELS / BBP_ROUND_BEST_KERNELS,
// which the owning unit defines before it includes anything.  A unit that needs another unit's launch calls a host function below.
#pragma once
#include <mutex>
#include <string>

#include "batch.h"
#include "chacha.h"
#include "round_select.h"
#include "submit.h"

namespace bbp {

// ---- the exception barriers -------------------------------------------------------------------------------------------------------
// entry points without a context to lock still keep every exception on this side of the boundary
template <class F>
static int32_t no_throw(F&& body, const void* ctx = nullptr) noexcept {
    try {
        return body();
    } catch (const std::invalid_argument& e) {
        try { set_tls_error(ctx, std::string("invalid argument: ") + e.what()); } catch (...) {}
        return BBP_ERR_BAD_ARG;
    } catch (const std::exception& e) {
        try { set_tls_error(ctx, std::string("internal error: ") + e.what()); } catch (...) {}
        return BBP_ERR_INTERNAL;
    } catch (...) {
        set_tls_error(ctx, "internal error: unknown exception");
        return BBP_ERR_INTERNAL;
    }
}
template <class F>
static int32_t no_throw_ctx(bbp_ctx* ctx, F&& body) noexcept {  // for bodies that lock in phases: same mapping as api_guard
    try {
        return body();
    } catch (const std::invalid_argument& e) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string("invalid argument: ") + e.what(), BBP_ERR_BAD_ARG; });
        return BBP_ERR_BAD_ARG;
    } catch (const std::bad_alloc&) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = "host allocation failed", BBP_ERR_INTERNAL; });
        return BBP_ERR_INTERNAL;
    } catch (const std::exception& e) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string("internal error: ") + e.what(), BBP_ERR_INTERNAL; });
        return BBP_ERR_INTERNAL;
    } catch (...) {
        return BBP_ERR_INTERNAL;
    }
}

// ---- host-pointer batch calls: three staging slots, lock held only while enqueueing (context.h IoSlot) ---------------------------
struct SlotLease {
    bbp_ctx* ctx;
    bbp_ctx::IoSlot* sl;
    explicit SlotLease(bbp_ctx* c, bool verify = false) : ctx(c) {
        std::unique_lock<std::mutex> lk(c->io_mu);
        // strict rotation keeps consecutive calls on different slots; prove and verify calls have their own
        const uint32_t want = verify ? bbp_ctx::IO_SLOTS + c->io_vnext++ % bbp_ctx::IO_VSLOTS : c->io_next++ % bbp_ctx::IO_SLOTS;
        c->io_cv.wait(lk, [&] { return !c->io[want].busy; });
        sl = &c->io[want];
        sl->busy = true;
    }
    ~SlotLease() {
        {
            std::lock_guard<std::mutex> lk(ctx->io_mu);
            sl->busy = false;
        }
        ctx->io_cv.notify_all();
    }
};
inline uint32_t host_chunk_verify() { return VerifyKnobs::host_chunk_now(); }  // verify_plan.h lists the name

// ---- capi_prove.hip ---------------------------------------------------------------------------------------------------------------
int32_t check_n(bbp_ctx* ctx, uint32_t N);
bool os_random(uint8_t* buf, size_t n);
int32_t no_os_random(bbp_ctx* ctx);
int32_t next_device_key(bbp_ctx* ctx, ChachaKey* key);
int32_t draw_enqueue(bbp_ctx* ctx, u32 B, u32 N, u32 kind, const ChachaKey& key, u32 row_base, void* out, hipStream_t s);
hipError_t wait_event_polling(hipEvent_t ev);
int32_t pinned_reserve(bbp_ctx* ctx, void*& p, size_t& cap, size_t bytes);
int32_t upload_inputs(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const uint8_t* a, size_t na, const uint8_t* b, size_t nb, size_t ent_off = 0,
                      const uint8_t* a2 = nullptr, size_t na2 = 0, size_t a2_off = 0);
int32_t fetch_results(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, size_t bytes);
int32_t staging_reserve(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const ProveStaging& L);
int32_t select_kernels_enqueue(bbp_ctx* ctx, u32 B, const u32* recs, const RsFloor& floor, u32 K, u32 cap, u32* sel, u32* counts, u8* state,
                               hipStream_t s);
enum CheckMode { CHECK_AUTO, CHECK_OFF, CHECK_REPROVE };  // context's setting / never (bbp_reserve) / checked, no second prove
struct RoundInput;                                        // bbp_prove_round's table and raw bids
int32_t prove_batch_host(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out, int32_t* status,
                         CheckMode mode = CHECK_AUTO, const RoundInput* round = nullptr);
void async_done(Request* r);  // completion hook of bbp_prove_async and bbp_verify_async

// ---- capi_verify.hip (verify_host: context.h) -------------------------------------------------------------------------------------
int32_t verify_batch_host(bbp_ctx* ctx, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group = 0, uint32_t* n_fallback = nullptr);

// ---- capi_best.hip ----------------------------------------------------------------------------------------------------------------
// where a call's results go (n_duplicates: the one-per-bidder calls, otherwise null)
struct BestOut {
    u32 cap;
    u32 *best, *n_best, *n_candidates, *n_examined, *n_duplicates;
    u32* n_tranches = nullptr;  // the tranches that held at least one row (the many-rounds calls with one round report them)
};
int32_t best_hook_refuse(bbp_ctx* ctx, const std::string& why);
int32_t best_hook_screen(bbp_ctx* ctx, const char* what, u32 B, const int32_t* verdicts, u32* n_ok);
// the three single-round calls behind their screening, as the entry points of one round and the many-rounds calls with R == 1 run them:
// the public host forms; the hooks' call on caller-made keys, ids (null: the plain call) and verdicts; the _dev forms
int32_t best_public_host(bbp_ctx* ctx, u32 N, const uint8_t* round, u32 B, const uint8_t* rows, const uint8_t* floor32, u32 K, u32 tranche, bool distinct,
                         const BestOut& out, int32_t* status);
int32_t best_hook_host(bbp_ctx* ctx, u32 B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts, const uint8_t* floor32, u32 K, u32 tranche,
                       u32 table_log2, const BestOut& out, int32_t* status);
int32_t best_public_dev(bbp_ctx* ctx, u32 N, const void* round_dev, u32 B, const void* rows_dev, const void* entropy_dev, const uint8_t* floor32, u32 K,
                        u32 tranche, bool distinct, const BestOut& out, void* status_dev, void* stream);
// the k_best_pairs launch: the winners' pairs of the n rows in sel (counts: the device-side count) out of the winner records
int32_t best_pairs_enqueue(bbp_ctx* ctx, u32 n, const u32* sel, const u32* counts, const u32* win, u32* pairs, hipStream_t s);
// standings, as the many-standings call (capi_bests.hip) needs them: the context that holds a handle's standings (a pool: member 0); a
// refusal; the open standing behind a handle, or null (caller holds dev->best_mu); what the host keeps of a committed working header
// (STAND_H_* words) after an offer of `rows` rows; the two single-standing offers behind their screening, as the entry points of one
// standing and the many-standings calls with S == 1 run them (out.n_tranches: the tranches that ran)
bbp_ctx* stand_dev(bbp_ctx* ctx);
int32_t stand_refuse(bbp_ctx* ctx, const std::string& why);
bbp_ctx::Standing* stand_find(bbp_ctx* dev, u32 handle);
void stand_record_commit(bbp_ctx::Standing& m, const u32* whdr, u32 rows);
int32_t stand_public_host(bbp_ctx* ctx, const char* what, u32 standing, u32 B, const uint8_t* rows, u32 tranche, const BestOut& out, int32_t* status);
int32_t stand_hook_host(bbp_ctx* ctx, const char* what, u32 standing, u32 B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts, u32 tranche,
                        const BestOut& out, int32_t* status);

}  // namespace bbp
