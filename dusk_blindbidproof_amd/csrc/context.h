// Engine context shared by the translation units of libbbp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bbp.h"
#include "point.h"
#include "msm_index.h"
#include "msm_plan.h"
#include "prove_io.h"
#include "prove_plan.h"
#include "scalar.h"
#include "standing_handles.h"
#include "verify_plan.h"
#include "verify_rows.h"

namespace bbp {

// ---- MSM geometry (see DESIGN.md "K1") ---------------------------------------------------------------
// (MSM_NAF / MSM_W / MSM_K and the split MSMs' SMALL_NAF / SMALL_K / SMALL_W are msm_plan.h's: the plan of a launch names them)
constexpr int MSM_POS = 256;              // table rows per generator: 2^b * P for every bit position b
#ifndef BBP_MSM_T
#define BBP_MSM_T 128
#endif
constexpr int MSM_T = BBP_MSM_T;          // lanes of the accumulate workgroup: 128 (2 wavefronts; -DBBP_MSM_T=64 for experiments)
#ifndef BBP_ACC_T
#define BBP_ACC_T 256
#endif
// lanes of k_msm_acc = equal chunks the sorted entries are cut into (k_msm_fold keeps MSM_T lanes).  Since the fold moved out the
// accumulate kernel is nothing but the chunk loop, and 256 lanes (four wavefronts) per MSM fill the machine better than 128: a
// third-of-a-batch launch is 682 MSMs = 2728 wavefronts for 2048 resident slots instead of 1364 (measured 18.2-18.4 k -> 19.0-19.6 k
// proofs/s; 384 lanes 17.0 k, 512 lanes 18.2 k; more than two waves per SIMD with 256 lanes 18.5-18.8 k)
constexpr int ACC_T = BBP_ACC_T;
static_assert(ACC_T % MSM_T == 0, "the fold kernel deals the accumulate kernel's chunks to its lanes");
constexpr int MSM_G = MSM_K / MSM_T;      // consecutive buckets per lane (8)
constexpr int MSM_LOG_G = MSM_T == 128 ? 3 : 4;
static_assert(MSM_T == 128 || MSM_T == 64, "the cross-lane fold is written for one or two wavefronts");
// IPA tail (prover.hip): from round FOLD_ROUND the folded generators are explicit points; they are materialised by a
// composite-bucket Pippenger pass over the same row table (msm.hip, the <1> instances of k_msm_sort / k_msm_acc)
// (FOLD_ROUND, the first tail round, is prove_plan.h's: the plan of a prove call names it)
// (FOLD_CLS, the folded generators per side, is batch_layout.h's: the batch buffer holds them)
constexpr int FOLD_NAF = 9;                // width-9 NAF: odd digits |d| < 256
constexpr int FOLD_W = 29;                 // most digits per scalar
constexpr int FOLD_M = 128;                // buckets per class
constexpr int FOLD_K = FOLD_CLS * FOLD_M;  // 4096 composite buckets
static_assert(SMALL_W == FOLD_W, "split MSMs recode at the generator-fold pass's width");
// (the extra table bases behind the public ones -- PAD_BASE0, MRG_BASE0, MSM_SKIP_BASE, TAB_BASES -- are msm_index.h's: the index lists name them)
constexpr int GE_WORDS = sizeof(ge) / 4;  // 40: a point in registers / LDS / scratch

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t dirty = 0;  // secret wiping on: the most bytes asked of the buffer since its last wipe (wipe.hip wipe_take erases those)
};

}  // namespace bbp

struct bbp_ctx {
    // One lock per context: every extern "C" entry point that touches the context holds it for the whole call (api_guard below), so
    // the reference's per-connection worker threads (src/main.rs:55, src/futures/main.rs:46-56) may share ONE context.  Recursive:
    // bbp_prove -> bbp_prove_batch, bbp_msm_batch -> bbp_msm_batch_dev nest.  Concurrent single-proof callers do not queue on this
    // lock one by one: submit.hip coalesces them into one batch call (group commit).
    std::recursive_mutex mu;
    void* combiner = nullptr;  // bbp::Combiner* (submit.hip): coalesces concurrent bbp_prove / bbp_verify calls into batch calls
    // Device pool (pool.cpp, bbp_pool_init / bbp_init_all): a context with `members` owns no device state of its own -- it is the
    // handle the reference's prove() / verify() callers share when the node has several GPUs: ONE combiner deals their batches to
    // the members (one ordinary context per GPU), the host-pointer batch calls block-split over them.  A member knows its pool.
    std::vector<bbp_ctx*> members;
    void* pool_workers = nullptr;  // bbp::PoolWorkers* (pool.cpp): the members' persistent host threads for the block-split batch calls
    bbp_ctx* owner = nullptr;
    uint32_t member_index = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;            // opening stage of the prover pipeline (prover.hip)
    hipStream_t copy = nullptr;            // the caller's ingest stream (bbp_context_copy_stream): never used by the engine
    hipStream_t side2 = nullptr;           // second opening stream: batches too small to fill three heavy slices alternate between the two
    bbp::ProveKnobs knobs;                 // how prove calls are scheduled (prove_plan.h): read from the environment by bbp_init ...
                                           // (knobs.blinding_draw is no environment knob: bbp_set_blinding_draw writes it under the lock, capi_ctx.hip)
    bbp::ProveRuleState prove_state;       // ... and what the rules remember from call to call; prover.hip plans every call from the two
    bbp::VerifyKnobs vknobs;               // how verify calls are laid out and launched (verify_plan.h): read from the environment by bbp_init
    std::vector<hipStream_t> spare_streams;  // (experiment BBP_VL_SKIP: placeholders in the hardware-queue round-robin)
    static constexpr int CALL_RING = 8;
    hipEvent_t ev_call[CALL_RING] = {};    // completion of the last CALL_RING prove calls (how many are still in flight)
    bool ev_call_valid[CALL_RING] = {};
    int last_prove_par = -1;               // buffer of the last prove call (last_par is also set by the verifier lanes)
    static constexpr int MAX_SLICES = bbp::PROVE_MAX_SLICES;  // heavy-stage slices of one batch, one stream each (slice 0 = caller's stream)
    hipStream_t lane[MAX_SLICES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_join[MAX_SLICES] = {nullptr, nullptr, nullptr, nullptr}, ev_stagger[MAX_SLICES] = {nullptr, nullptr, nullptr, nullptr};
    bbp::MsmKnobs msm_knobs;    // which kernels an MSM launch takes (msm_plan.h): read from the environment by bbp_init; msm.hip plans every launch from them
    bool sort_lds_attr = false; // k_msm_sort_staged's dynamic-LDS limit has been raised on this context's device
    bool sort_lds_attr1 = false;  // ... and that of the generator-fold instance
    int debug_corrupt = 0;      // bbp_debug_corrupt_scratch: poison the next MSM launch's sorted scratch (tests)
    std::map<const void*, int> serial_attr;
    static constexpr int PROVE_BUFS = bbp::PROVE_BUFS;  // prover batch buffers in rotation (call k of the small-batch path uses buffer k % PROVE_BUFS; large batches alternate between 0 and 1)
    hipEvent_t ev_open[PROVE_BUFS] = {}, ev_done[PROVE_BUFS] = {};
    hipEvent_t ev_entry[PROVE_BUFS] = {};  // caller's stream at entry of a prove call: out_dev is not written before it
    bool ev_done_valid[PROVE_BUFS] = {}, ev_open_valid[PROVE_BUFS] = {};
    // BBP_VERIFY_SERIAL_ACC=1: the verifier lanes' MSM accumulate launches are chained by events so that no two of them are
    // co-resident (each then runs beside the other lanes' thin front-end kernels only).  Helps two lanes that share hardware queues
    // with other streams (6.5 -> 6.3 ms per 1024); with four lanes on queues of their own free-running is faster (5.2 vs 6.05 ms): off.
    int verify_serial_acc = 0;
    static constexpr int VACC_RING = 4;
    hipEvent_t ev_vacc[VACC_RING] = {};
    uint32_t vacc_seq = 0;
    bool vacc_valid = false;
    uint32_t seq_at_last_verify = 0;                     // prover call counter seen by the last verification (interleaving test)
    hipEvent_t ev_prep = nullptr;  // end of the last bbp_prepare_bids_dev: the next prove call's opening stage waits for it
    bool ev_prep_valid = false;
    hipEvent_t ev_draw = nullptr;  // end of the last prove-kind bbp_draw_entropy_dev: the same rule as ev_prep, an event of its own
    bool ev_draw_valid = false;
    // On-device entropy (bbp_set_entropy_source, capi_prove.hip): where host-pointer calls without caller entropy get theirs
    std::atomic<int> entropy_source{BBP_ENTROPY_SOURCE_OS};
    bool debug_key_armed = false;  // bbp_debug_next_entropy_key: the next device draw of a host-pointer call uses debug_key
    uint8_t debug_key[32] = {};
    int last_par = 0;
    // calls on one context share scratch buffers: a call issued on a different caller stream than the previous one is ordered
    // behind it (stream_guard_enter / stream_guard_leave)
    // two families with disjoint scratch: 0 = prover, MSM hook, witness, setup read-backs; 1 = verifier (its own batch buffer,
    // misc scratch and MSM scratch slot VERIFY_SLOT) -- a verification issued on another stream than a prove call is NOT ordered
    // behind it and overlaps its heavy stage on the device
#ifndef BBP_VLANES
#define BBP_VLANES 4
#endif
    static constexpr int VLANES = BBP_VLANES;    // four lanes -- each with a hardware queue of its own at best, see below
    static constexpr int FAMILIES = 1 + VLANES;  // prover | one per verifier lane
    hipStream_t last_stream[FAMILIES] = {};
    hipEvent_t ev_last[FAMILIES] = {};
    bool ev_last_valid[FAMILIES] = {};
    // Two verifier LANES, each with everything a verification call touches (batch buffer, scratch, MSM scratch slot, aggregation
    // buffers, a stream): two calls on the two lanes share nothing, so the front end of one (parse, transcripts, powers, flatten,
    // scalars: latency-bound) runs under the MSM of the other.  The host-pointer API alternates lanes with its staging slots;
    // device-API callers pick a lane by passing that lane's stream (bbp_context_verify_stream), any other stream is lane 0.
    // FOUR lanes (round 3; two before).  A 1024-proof call is a chain of ~10 ms of kernels of which only the 4 ms MSM accumulate fills
    // the machine, so several chains must be in flight.  A third lane first measured 8-10 % SLOWER than two -- because its stream
    // shared a HARDWARE QUEUE with another lane's (fewer queues than the context's 9+ streams): with a queue per stream, 1024
    // verifications per call take 6.3 ms on two lanes, 5.45 on three, 5.17 on four, 5.45 / 5.25 on five / six.
    struct VLane {
        hipStream_t stream = nullptr;
        bbp::DevBuf misc, agg, agg_io;
        void *agg_vs = nullptr, *agg_varsum = nullptr;  // weighted generator scalars [B][4098] / per-proof variable-base sums of the last group pass
        int32_t* agg_gstatus = nullptr;                 // per-group verdicts of that pass (inside agg)
        bbp::u32* agg_count = nullptr;                  // [2] device counters: proofs of the current call on the per-proof path / running total
        hipEvent_t ev_vfork = nullptr, ev_vjoin = nullptr;  // variable-base kernel on lane[1] beside the generator MSM (lane 0 only)
        // mixed-N calls (verifier_mixed.inc): pinned staging of the per-row N upload.  An entry is reused only once its copy has run
        // (its event), so a call queued behind others on the lane never has its Ns overwritten by a later call.
        struct NsStage {
            void* h = nullptr;
            size_t cap = 0;
            hipEvent_t ev = nullptr;
        };
        std::vector<NsStage> ns_ring;
        uint32_t ns_oldest = 0;  // the entry waited for when every entry is still queued (NS_RING of them)
    };
    VLane vl[VLANES];
    std::string err;
    bbp::u32* health = nullptr;  // device word, bit 0: an MSM table gather had to be clamped (corrupted scratch); bit 1: a proof with a
                                 // satisfied witness failed its check twice (checked proving) -- bbp_check_health
    // Checked proving (bbp_set_prove_check, capi_prove.hip): every record is verified on the device before it is handed out.
    std::atomic<int> prove_check{0};
    // Secret wiping (bbp_set_secret_wipe, wipe.hip; the classes are secret_map.h's): while on, every SECRET buffer reads zero whenever
    // no prove-side call is in flight -- each call erases what it wrote, at the end of the stream that guards the buffer
    std::atomic<int> secret_wipe{0};
    // bbp_debug_poison_scratch(.., sticky != 0) (wipe.hip; tests): while set, dev_reserve fills every buffer it newly allocates with
    // poison_word, the way it fills with zero under wiping -- the first call of a fresh context and every regrowth run over poison too
    std::atomic<int> poison_sticky{0};
    uint32_t poison_word = 0;
    struct WipeLog {  // the wipes enqueued since the log was cleared (bbp_debug_wipe_cost): how many bytes in how many launches, over which buffers
        static constexpr int CAP = 24;  // = WIPE_SPANS: what one lone launch replays
        uint64_t bytes = 0;
        uint32_t launches = 0;
        int n = 0;
        bbp::DevBuf* buf[CAP] = {};
        uint64_t span_bytes[CAP] = {};
    } wipe_log;
    std::atomic<uint64_t> chk_checked{0}, chk_reproved{0};  // rows handed to checked calls / records proved a second time
    unsigned long long* chk_counts = nullptr;  // device [2]: rows refused by the witness check / records that failed verification
    int64_t debug_corrupt_proof = -1;          // bbp_debug_corrupt_next_proof: record index of the next prove call to corrupt (tests)
    uint32_t chk_lane = 0;                     // verifier lane of the next check (rotation)
    hipEvent_t ev_chk_fork = nullptr, ev_chk_join = nullptr;  // records complete -> check on a lane stream -> back on the caller's
    // Scratch of bbp_prove_batch_checked_dev calls (verify rows, verifier statuses, witness masks), in rotation: a ring entry is
    // reused only after the status kernel of the call that used it last (ev); host-pointer calls use their staging slot's `chk`.
    static constexpr int CHECK_RING = PROVE_BUFS;
    struct CheckBuf {
        bbp::DevBuf buf;
        hipEvent_t ev = nullptr;
        bool ev_valid = false;
    };
    CheckBuf chk[CHECK_RING];
    uint32_t chk_next = 0;
    // Scratch of bbp_prepare_round_dev / bbp_prove_round_dev calls (reduced table, per-bid results; the latter's prove-input rows and
    // records), in rotation under the same rule: reused only after the last kernel of the call that used it last.  bbp_prove_round
    // keeps its own in its staging slot.  ev_round: the table of a host-pointer round call has been reduced (its later chunks wait).
    CheckBuf rnd[CHECK_RING];
    uint32_t rnd_next = 0;
    hipEvent_t ev_round = nullptr;
    // Phase A of bbp_prove_round_select and bbp_debug_round_select (capi_prove.hip; the layout is prove_io.h's SelectStaging): bids,
    // table, score records, selection on the device and a pinned mirror of what travels.  Both grow on demand (bbp_reserve does not
    // size them); sel_mu serialises the calls that use them, and is taken BEFORE the context lock.
    std::mutex sel_mu;
    bbp::DevBuf sel_dev;
    void* sel_h = nullptr;
    size_t sel_h_cap = 0;
    hipEvent_t ev_sel = nullptr;
    // bbp_verify_round_best, its _dev form and bbp_debug_round_best (capi_best.hip; the layout is round_best.h's BestLayout): keys,
    // candidate and winner records, statuses, one tranche's selection and verdicts on the device, a pinned mirror of what travels, and
    // -- the _dev form only -- the gathered rows of one tranche with their entropy rows.  All PUBLIC (secret_map.h), all grow on demand
    // (bbp_reserve does not size them); best_mu serialises the calls that use them, and is taken BEFORE the context lock.
    // The one-per-bidder calls (bbp_verify_round_best_distinct, ...) use the same allocations: BestDistinctLayout puts the rows' z_img,
    // the identity table and three counters behind BestLayout's state -- public for the same reason: what any verifier is handed.
    // The many-rounds calls (bbp_verify_rounds_best, ...) with R > 1 lay the same allocations out by rounds_best.h's BestsLayout:
    // per-round counters, segments and floors, round_of and row offsets beside the keys, records and statuses.
    // An offer to many standings (bbp_standings_offer; standings.h's StandingsLayout) works behind that state, in the same allocations.
    std::mutex best_mu;
    bbp::DevBuf best_dev, best_rows;
    void* best_h = nullptr;
    size_t best_h_cap = 0;
    hipEvent_t ev_best = nullptr;
    // Standings (bbp_standing_open, ...; capi_best.hip; round_standing.h's StandingLayout): per open standing a device allocation of
    // its OWN -- header, K keys, ids and serials -- that lives from open to close, PUBLIC like the state above, and what the host knows
    // of it: the round, the floor, and a shadow of the header as of the last commit.  An offer works in best_dev and commits at its end.
    // Guarded by best_mu; a pool keeps its standings on member 0.
    struct Standing {
        uint32_t N = 0, K = 0, count = 0, trip = 0;  // trip: bbp_debug_standing_trip (0: none)
        uint32_t floor[8] = {}, bar[8] = {};
        uint64_t offered = 0;
        std::vector<uint8_t> round;
    };
    static constexpr int STANDINGS = BBP_STANDING_MAX_OPEN;
    bbp::StandingHandles stand_handles;  // which are open (standing_handles.h)
    Standing stand_meta[STANDINGS];
    bbp::DevBuf stand[STANDINGS];
    // resident tables
    bbp::ge* gens = nullptr;           // [TAB_BASES] extended points: B_blinding, G[2048], H[2048], B, then the PAD_BASES range sums and the MRG_BASES merged bases
    bbp::niels_row* ptable = nullptr;      // [TAB_BASES * MSM_POS] affine cached 2^b * P_i, 128-byte limb rows (275 MB)
    bbp::ge* btab = nullptr;               // [TAIL_TAB] m * 2^(TAIL_PIECE_BITS k) * B, m = 1..8, k = 0..TAIL_PIECES-1 (scalarmul.h; prover.hip tail rounds)
    bbp::niels_packed* comb = nullptr;     // [2][64][8] radix-16 comb for B and B_blinding (small commits)
    bbp::sc* mimc_c = nullptr;         // [90]
    uint8_t gens_enc_host_valid = 0;
    std::vector<uint8_t> mimc_host;    // 90 * 32
    // grow-only scratch
    bbp::DevBuf scal, idx, sorted, pts, enc, batch[PROVE_BUFS + VLANES], io_in, io_out, io_ent, raw[4];  // batch[3 + lane]: the verifier lanes'; raw[i]: draw buffer of the stream that opens (ProvePlan::raw_index: side, side2, lane[1], lane[2])
    static constexpr int VERIFY_SLOT = MAX_SLICES;  // MSM scratch slots of the verifier lanes: VERIFY_SLOT + lane
    bbp::DevBuf slice_sorted[MAX_SLICES + VLANES], slice_pts[MAX_SLICES + VLANES], slice_fold[MAX_SLICES], slice_vtab[MAX_SLICES];  // per-slice MSM scratch (slice 0 uses sorted / pts)
    // Host-pointer batch calls stage through one of three slots (device in / entropy / out + a pinned host mirror of the results):
    // a call holds the context lock only while it ENQUEUES; it waits for its results on the slot's event with the lock released,
    // so other host threads can enqueue the next batches meanwhile and the engine's cross-call pipeline (opening stage of call
    // k+1 under the MSM stage of call k) also works for bbp_prove_batch / bbp_prove / the UDS server (capi_prove.hip).
    struct IoSlot {
        bbp::DevBuf in, ent, out, chk;               // chk: verify rows + verifier statuses of a checked prove call
        uint32_t* h_flag = nullptr;              // pinned: the context's health word as read back with this slot's results
        void *h_out = nullptr, *h_in = nullptr;  // pinned mirrors: results / inputs (a copy from PAGEABLE memory waits for the whole
        size_t h_cap = 0, h_in_cap = 0;          // device to go idle -- measured 87 ms behind a running batch -- a pinned one does not)
        hipEvent_t ev = nullptr, ev_in = nullptr;
        bool busy = false;
    };
    static constexpr int IO_SLOTS = 3;           // prove calls rotate over slots 0..2
    static constexpr int IO_VSLOTS = VLANES;     // verify calls over their own slots 3..4 (= verifier lane 0 / 1): a verification never
    IoSlot io[IO_SLOTS + IO_VSLOTS];             // waits for a slot that a 100 ms prove call is holding
    std::mutex io_mu;
    std::condition_variable io_cv;
    uint32_t io_next = 0, io_vnext = 0;
    std::map<uint32_t, void*> circuits;  // N -> CircuitDev* (compiled blind-bid circuit tables on the device)
    void* vctab = nullptr;               // mixed-N verification: device table [MAX_ITEMS + 1] of VCirc (verifier_mixed.inc), entry N
    uint8_t vctab_has[256] = {};         // filled once circuit N is compiled
    std::map<uint64_t, bbp::u32*> layout_idx;  // (layout << 32 | n_terms) -> device base-index list of bbp_msm_batch (capi_msm.hip)
    std::vector<float> timings;
    uint64_t scratch_allocs = 0;  // dev_reserve: how many times a grow-only scratch buffer was (re)allocated since bbp_init ...
    size_t scratch_bytes = 0;     // ... and what they hold now (bbp_describe)
    // optional per-kernel HIP-event timing (bbp_set_profiling): (tag, start, stop) on the launch stream
    bool profile = false;
    struct Ev {
        int tag;
        hipEvent_t a, b;
    };
    std::vector<Ev> events;
};

namespace bbp {

// BBP_DEBUG_DEVICE_CHECK=1 (on in every -m gpu test): before EVERY HIP call the engine makes on behalf of a context -- launches
// (their hipGetLastError), event records / waits, allocations, copies -- the calling thread's current device must be the context's.
// A process with one context per GPU (the pool, bbp-uds-server --devices, one combiner thread hopping between members) depends on
// every entry point, every combiner batch thread and every pool worker having called hipSetDevice first; on a one-GPU box a missing
// call is invisible, on the first 8-GPU node it is a stream / event of device A used with device B current.  With the check on such a
// call fails with BBP_ERR_DEVICE and names the call site instead.  (hipSetDevice itself is exempt: it is the call that establishes
// the state.)  Cost when on: one thread-local read per HIP call; when off: one predictable branch.
inline bool device_check_on() {
    static const bool on = [] { const char* e = getenv("BBP_DEBUG_DEVICE_CHECK"); return e && atoi(e) != 0; }();
    return on;
}
inline bool device_affinity_ok(bbp_ctx* ctx, const char* what) {
    if (!device_check_on() || ctx->device < 0) return true;
    if (!strncmp(what, "hipSetDevice", 12) || !strncmp(what, "hipGetDeviceCount", 17)) return true;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == ctx->device) return true;
    ctx->err = "device affinity violated: current device " + std::to_string(cur) + ", context lives on device " + std::to_string(ctx->device) + ", at " + what;
    fprintf(stderr, "[bbp] %s\n", ctx->err.c_str());
    return false;
}

#define BBP_HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                               \
        if (!bbp::device_affinity_ok(ctx, #expr)) return BBP_ERR_DEVICE;                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
            return BBP_ERR_DEVICE;                                                                     \
        }                                                                                              \
    } while (0)

inline int32_t dev_reserve(bbp_ctx* ctx, DevBuf& b, size_t bytes) {
    const bool wipe = ctx->secret_wipe.load(std::memory_order_relaxed) != 0;
    if (wipe && bytes > b.dirty) b.dirty = bytes;  // what the call is about to write: its wipe erases that much
    if (b.cap >= bytes) return BBP_OK;
    if (b.p) {
        if (wipe) {  // old contents never go back to the driver as they are (hipFree would wait for the device anyway)
            BBP_HIP_TRY(ctx, hipDeviceSynchronize());
            BBP_HIP_TRY(ctx, hipMemset(b.p, 0, b.cap));
        }
        BBP_HIP_TRY(ctx, hipFree(b.p));
        ctx->scratch_bytes -= b.cap;
    }
    b.p = nullptr;
    b.cap = 0;
    size_t want = (bytes + (bytes >> 3) + 4096 + 15) & ~(size_t)15;  // whole 16-byte grains: a wipe, a fill and a scan cover all of it
    BBP_HIP_TRY(ctx, hipMalloc(&b.p, want));
    if (ctx->poison_sticky.load(std::memory_order_relaxed) != 0 && !wipe) {  // test hook: a new buffer starts out as the poison word
        BBP_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)b.p, (int)ctx->poison_word, want / 4, nullptr));
        BBP_HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    }
    if (wipe) {  // ... and a new one starts out zero (the driver hands out whatever was freed last): a call erases what it wrote, not the capacity
        BBP_HIP_TRY(ctx, hipMemsetAsync(b.p, 0, want, nullptr));
        BBP_HIP_TRY(ctx, hipStreamSynchronize(nullptr));  // the context's streams do not wait for the null stream
    }
    b.cap = want;
    ctx->scratch_bytes += want;
    ctx->scratch_allocs++;  // bbp_describe reports both: after bbp_reserve the count must stand still (tests/test_gpu_boundary.py)
    static const bool trace = getenv("BBP_TRACE_ALLOC") != nullptr;  // which buffer grew: its offset inside the context names the field
    if (trace)
        fprintf(stderr, "[bbp alloc] device %d: buffer at context offset %zu grows to %zu bytes (allocation %llu)\n", ctx->device,
                (size_t)(reinterpret_cast<const char*>(&b) - reinterpret_cast<const char*>(ctx)), want, (unsigned long long)ctx->scratch_allocs);
    return BBP_OK;
}

enum { TAG_MSM = 1, TAG_ENCODE = 2, TAG_WITNESS = 3, TAG_RNG = 4, TAG_POLY = 5, TAG_IPA_SCALARS = 6, TAG_COMMIT = 7,
       TAG_TRANSCRIPT = 8, TAG_VERIFY_SCALARS = 9, TAG_VARBASE = 10, TAG_MSM_SORT = 11, TAG_MSM_FOLD = 12, TAG_WIPE = 13 /* k_wipe_spans */,
       TAG_SELECT = 14 /* k_round_select_*: the selection launches */ };

struct ScopedEvent {  // records start now, stop at scope exit, when profiling is on
    bbp_ctx* ctx;
    hipStream_t s;
    int idx = -1;
    ScopedEvent(bbp_ctx* c, int tag, hipStream_t st) : ctx(c), s(st) {
        if (!c->profile) return;
        bbp_ctx::Ev e;
        e.tag = tag;
        if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
        (void)hipEventRecord(e.a, st);
        c->events.push_back(e);
        idx = (int)c->events.size() - 1;
    }
    ~ScopedEvent() {
        if (idx >= 0) (void)hipEventRecord(ctx->events[idx].b, s);
    }
};

// see prover.hip "serial_lds_bytes": kernels that must not share a CU with the long-lived serial waves ask for a few bytes of LDS
inline unsigned lds_token(const bbp_ctx* ctx) { return ctx->knobs.lds_token(); }

// One-lane-per-item serial kernels that run beside the MSM stage ask for (nearly) a whole CU's LDS so that nothing else is placed
// on their CU (prover.hip "Serial waves get their own CUs"): raise the kernel's dynamic-LDS limit once per kernel.
inline int32_t serial_lds_bytes(bbp_ctx* ctx, const void* kernel, unsigned* dyn_bytes = nullptr) {
    if (dyn_bytes) *dyn_bytes = 0;
    if (ctx->knobs.serial_lds <= 0) return BBP_OK;
    if (!ctx->serial_attr.count(kernel)) {
        // the reservation is dynamic LDS on top of whatever the kernel declares statically: together they must fit the CU's 160 KB
        hipFuncAttributes fa;
        BBP_HIP_TRY(ctx, hipFuncGetAttributes(&fa, kernel));
        int dyn = ctx->knobs.serial_lds - (int)fa.sharedSizeBytes;
        if (dyn < 0) dyn = 0;
        BBP_HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dyn));
        ctx->serial_attr[kernel] = dyn;
    }
    if (dyn_bytes) *dyn_bytes = (unsigned)ctx->serial_attr[kernel];
    return BBP_OK;
}

// Calls on one context share scratch: a call issued on a different caller stream than the previous one is ordered behind it.
// RAII so that every exit path -- error returns included -- leaves ev_last recorded on the stream that may have work queued.
struct StreamGuard {
    bbp_ctx* ctx;
    hipStream_t s;
    int fam;  // 0: prover family, 1 + lane: a verifier lane (context.h: disjoint scratch, no ordering between families)
    bool entered = false;
    StreamGuard(bbp_ctx* c, hipStream_t st, int family = 0) : ctx(c), s(st), fam(family) {}
    int32_t enter() {
        if (ctx->ev_last_valid[fam] && ctx->last_stream[fam] != s) BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_last[fam], 0));
        entered = true;
        return BBP_OK;
    }
    ~StreamGuard() {
        if (!entered) return;
        if (hipEventRecord(ctx->ev_last[fam], s) == hipSuccess) {
            ctx->ev_last_valid[fam] = true;
            ctx->last_stream[fam] = s;
        }
    }
};

// `stream` argument of the _dev entry points: BBP_STREAM_CONTEXT selects the context's own stream, anything else -- NULL, the
// legacy default stream, included -- is the caller's hipStream_t and is honoured as such (include/bbp.h)
inline hipStream_t pick_stream(bbp_ctx* ctx, void* stream) { return stream == BBP_STREAM_CONTEXT ? ctx->stream : (hipStream_t)stream; }

// ---- the extern "C" barrier: lock + no exception ever crosses the boundary (include/bbp.h promises both) ---------------------
// bbp_last_error reports per calling thread AND per context: a failing call leaves (context, message) in a thread-local slot;
// bbp_last_error(ctx) answers from the slot only if it belongs to ctx, otherwise with the context's own last message -- a thread
// that drives several contexts (one per GPU) never reads one context's failure as another's.
std::string& tls_error();
const void*& tls_error_owner();
inline void set_tls_error(const void* ctx, const std::string& msg) {
    try {
        tls_error() = msg;
        tls_error_owner() = ctx;
    } catch (...) {
    }
}
inline const char* status_text(int32_t rc) {
    static const char* const names[] = {"ok", "verification failed", "bid list needs more than 2048 multipliers", "malformed input", "invalid argument",
                                        "device failure", "internal error"};
    return rc >= 0 && rc <= 6 ? names[rc] : "unknown status";
}
int32_t fault_injected(const char* site);  // BBP_FAULT_INJECT=<site>: throw at that site (tests/test_capi_symbols.py)

template <class F>
int32_t api_guard(bbp_ctx* ctx, F&& body) noexcept {
    int32_t rc;
    try {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        try {
            ctx->err.clear();  // whatever this call reports is this call's own message, never an older failure's
            rc = body();
        } catch (const std::invalid_argument& e) {
            ctx->err = std::string("invalid argument: ") + e.what();
            rc = BBP_ERR_BAD_ARG;
        } catch (const std::bad_alloc&) {
            ctx->err = "host allocation failed";
            rc = BBP_ERR_INTERNAL;
        } catch (const std::exception& e) {
            ctx->err = std::string("internal error: ") + e.what();
            rc = BBP_ERR_INTERNAL;
        } catch (...) {
            ctx->err = "internal error: unknown exception";
            rc = BBP_ERR_INTERNAL;
        }
        if (rc != BBP_OK) {
            try {
                if (ctx->err.empty()) ctx->err = status_text(rc);  // a failure path that set no text still reports its own status
                set_tls_error(ctx, ctx->err);
            } catch (...) {
            }
        }
    } catch (...) {  // the lock itself (std::system_error)
        rc = BBP_ERR_INTERNAL;
    }
    return rc;
}

inline bool is_pool(const bbp_ctx* ctx) { return ctx && !ctx->members.empty(); }
// setup.hip: GPU_MAX_HW_QUEUES is exported by the library itself when the process has not initialised HIP yet (state: 1 the caller's
// environment had it, 2 set here, 3 too late)
void own_hw_queues();
int hw_queues_state();
// pool.cpp: the host-pointer batch calls on a pool handle (block split by index over the members, results in request order)
int32_t pool_prove_batch(bbp_ctx* pool, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out, int32_t* status);
// bbp_prove_round on a pool handle: the bids block-split like pool_prove_batch's rows, every member receives the table
int32_t pool_prove_round(bbp_ctx* pool, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* bids, const uint8_t* entropy, uint8_t* rows_out,
                         uint64_t* toggles_out, int32_t* status);
// every verify form on a pool handle: the rows block-split over the members (VerifyRows::slice); group == 0: the plain entry point
int32_t pool_verify(bbp_ctx* pool, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group, uint32_t* n_fallback);
// capi_verify.hip: the host-pointer verify path of a context or a pool, after the entry point's screening (what a pool runs on its members)
int32_t verify_host(bbp_ctx* ctx, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group, uint32_t* n_fallback);
int32_t pool_msm_batch(bbp_ctx* pool, uint32_t B, uint32_t n_terms, const uint8_t* scalars, uint32_t layout, uint8_t* out32);
int32_t pool_reject(bbp_ctx* pool, const char* what);  // BBP_ERR_BAD_ARG + message: entry points that need ONE device
void pool_workers_start(bbp_ctx* pool);
void pool_workers_stop(bbp_ctx* pool);
int pool_member_numa_node(const bbp_ctx* pool, uint32_t i);

// msm.hip
// base_idx_dev holds n_idx_sets lists of n_terms indices; MSM number i uses list (i % n_idx_sets)
// msm_map_dev / n_active_dev (both or neither): a device-sized launch -- n_msm is the upper bound, *n_active_dev MSMs exist and MSM j
// takes its scalars from row msm_map_dev[j]
// chain_acc: the accumulate launch waits for the previous chained accumulate launch of this context (verifier lanes, see verify_serial_acc)
int32_t msm_launch(bbp_ctx* ctx, uint32_t n_msm, uint32_t n_terms, const u32* scalars_dev, const u32* base_idx_dev,
                   ge* out_points_dev, hipStream_t stream, uint32_t n_idx_sets = 1, int scratch_slot = 0, const u32* msm_map_dev = nullptr,
                   const u32* n_active_dev = nullptr, bool chain_acc = false);
int32_t fold_generators_launch(bbp_ctx* ctx, uint32_t n_proofs, const sc* g_dev, const sc* h_dev, ge* out_dev, hipStream_t stream,
                               int scratch_slot);
int32_t encode_launch(bbp_ctx* ctx, uint32_t n, const ge* pts_dev, uint8_t* out32_dev, hipStream_t stream);
size_t msm_scratch_bytes(uint32_t n_msm, uint32_t n_terms);
// wipe.hip (secret wiping).  A wipe is one k_wipe_spans launch over up to WIPE_SPANS spans; every span is checked against its buffer.
constexpr int WIPE_SPANS = 24;  // the most one launch takes (a call's own lists hold at most four; bbp_debug_wipe_cost replays a whole call's)
struct WipeSpan {
    void* p;
    unsigned long long bytes;  // a multiple of 16
};
struct WipeList {
    int n = 0;
    WipeSpan s[WIPE_SPANS];
    DevBuf* buf[WIPE_SPANS];  // the buffer behind each span
};
inline bool wipe_on(const bbp_ctx* ctx) { return ctx->secret_wipe.load(std::memory_order_relaxed) != 0; }
void wipe_take(WipeList& l, DevBuf& b);                              // what the buffer's users asked of it since its last wipe
int32_t wipe_enqueue(bbp_ctx* ctx, const WipeList& l, hipStream_t s);  // one launch on s (none for an empty list)
int32_t wipe_all(bbp_ctx* ctx);                                      // every SECRET buffer over its capacity, device and pinned; synchronises
int32_t wipe_failed_call(bbp_ctx* ctx, bbp_ctx::IoSlot& sl);         // what a half-enqueued host call reserved, and its slot; synchronises
// prover.hip
int32_t tail_btab_build(bbp_ctx* ctx);
size_t tail_btab_bytes();  // what it allocates for ctx->btab

}  // namespace bbp
