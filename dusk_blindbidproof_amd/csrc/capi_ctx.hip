// C-ABI, what belongs to the handle and to no call family: the error slots, the size functions, bbp_reserve, the batching, mixing and
// round-sharing settings, the debug hooks for challenges, tables and varbase, profiling -- see include/bbp.h.
#include <string.h>

#include <algorithm>
#include <thread>

#include "capi.h"

using namespace bbp;

namespace bbp {
std::string& tls_error() {
    static thread_local std::string e;
    return e;
}
const void*& tls_error_owner() {
    static thread_local const void* c = nullptr;
    return c;
}
int32_t fault_injected(const char* site) {
    const char* e = getenv("BBP_FAULT_INJECT");
    if (e && strcmp(e, site) == 0) throw std::runtime_error(std::string("injected fault at ") + site);
    if (e && strcmp(e, "alloc") == 0 && strcmp(site, "prove_batch") == 0) throw std::bad_alloc();
    return 0;
}
}  // namespace bbp

extern "C" uint32_t bbp_proof_record_size(uint32_t N) { return (uint32_t)proof_record_bytes(N); }
extern "C" uint32_t bbp_entropy_size(uint32_t N) { return (uint32_t)entropy_row_bytes(N); }

extern "C" int32_t bbp_debug_compile_circuit(uint32_t N, uint32_t* n_mul, uint32_t* n_cons) {
    return no_throw([&]() -> int32_t {
        if (N > BBP_MAX_ITEMS) return BBP_ERR_GENS_LEN;
        fault_injected("compile");
        const circuit::Compiled c = circuit::compile(N);  // throws std::invalid_argument for N == 0 (src/gadgets.rs:103 panics)
        if (n_mul) *n_mul = c.n_mul;
        if (n_cons) *n_cons = c.n_cons;
        return BBP_OK;
    });
}

// Grow every per-batch buffer of the context to what batches of `max_batch` need, by running the real paths once per staging
// slot / buffer parity on all-zero dummy rows (a zero row is a well-formed request: canonical scalars, toggle 0): whatever a
// later batch of at most that size touches -- batch buffers in rotation, MSM scratch per slice, draw buffers, staging slots and
// their pinned mirrors, the compiled circuit of list length N -- exists afterwards, so no call pays for (and no neighbour stalls
// behind) a hipFree + hipMalloc of gigabytes: growing scratch under load was measured through the UDS server as one ~0.9 s stall
// per run, i.e. the whole p99.
extern "C" int32_t bbp_reserve(bbp_ctx* ctx, uint32_t max_batch, uint32_t N) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc || max_batch == 0) return rc;
    if (is_pool(ctx)) {  // every member, all at once
        std::vector<int32_t> rcs(ctx->members.size(), BBP_OK);
        std::vector<std::thread> th;
        for (size_t i = 0; i < ctx->members.size(); i++) {
            try {
                th.emplace_back([&, i] { rcs[i] = bbp_reserve(ctx->members[i], max_batch, N); });
            } catch (...) {
                rcs[i] = bbp_reserve(ctx->members[i], max_batch, N);
            }
        }
        for (auto& t : th) t.join();
        for (int32_t r : rcs)
            if (r) return r;
        return BBP_OK;
    }
    return no_throw_ctx(ctx, [&]() -> int32_t {
        const uint32_t B = max_batch;
        const VerifyRows vrows = VerifyRows::uniform(B, N);
        std::vector<uint8_t> in(prove_in_bytes(N) * B, 0), ent(entropy_row_bytes(N) * B, 0), out(proof_record_bytes(N) * B), vin(vrows.row_bytes(0) * B, 0);
        std::vector<int32_t> st(B);
        int32_t rc = BBP_OK;
        // batches below 1024 proofs rotate three buffers and two opening streams, larger ones two buffers: both shapes, every slot
        for (int k = 0; k < bbp_ctx::IO_SLOTS && rc == BBP_OK; k++) rc = prove_batch_host(ctx, B, N, in.data(), ent.data(), out.data(), st.data(), CHECK_OFF);
        // the small-batch path rotates over ALL five batch buffers (buffer = call % PROVE_BUFS): five more calls whatever B is -- with
        // max_batch < 1024 the loop above IS that path but touches only three of them, and the first 4th / 5th call under load would
        // grow its buffer with hipFree + hipMalloc: the stall this function exists to prevent
        const uint32_t small = B < 1023 ? B : 1023;
        for (int k = 0; k < bbp_ctx::PROVE_BUFS && rc == BBP_OK; k++) rc = prove_batch_host(ctx, small, N, in.data(), ent.data(), out.data(), st.data(), CHECK_OFF);
        // ... and the shape a caller with several calls in flight gets (prover.hip "deep"): whole calls of B in rotation, five buffers
        if (B >= 1024 && ctx->knobs.deep_eligible(B)) {
            struct Reset { bool& b; ~Reset() { b = false; } } reset{ctx->prove_state.force_deep};
            ctx->prove_state.force_deep = true;
            for (int k = 0; k < bbp_ctx::PROVE_BUFS && rc == BBP_OK; k++) rc = prove_batch_host(ctx, B, N, in.data(), ent.data(), out.data(), st.data(), CHECK_OFF);
        }
        for (int k = 0; k < bbp_ctx::IO_VSLOTS && rc == BBP_OK; k++) rc = verify_batch_host(ctx, vrows, vin.data(), st.data());
        // What the warm-up calls above did not size, from the layouts the calls themselves use (prove_io.h): every buffer of every
        // staging slot for a round call (bbp_prove_round) and a plain one, as checked calls when checking is on -- the check's scratch,
        // its info block behind the records, its weights behind the entropy (uploaded entropy: the larger input mirror) -- and the
        // device forms' scratch rings.  Checked proving also runs the aggregated verifier (the check's) once per lane.
        const bool check = ctx->prove_check;
        for (int k = 0; check && k < bbp_ctx::IO_VSLOTS && rc == BBP_OK; k++) rc = verify_batch_host(ctx, vrows, vin.data(), st.data(), BBP_AGG_GROUP_DEFAULT);
        if (rc == BBP_OK)
            rc = api_guard(ctx, [&]() -> int32_t {
                int32_t rc = BBP_OK;
                BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
                for (int k = 0; k < bbp_ctx::IO_SLOTS && rc == BBP_OK; k++)
                    if (!(rc = staging_reserve(ctx, ctx->io[k], ProveStaging(B, N, true, check, false)))) rc = staging_reserve(ctx, ctx->io[k], ProveStaging(B, N, false, check, false));
                // source HEDGED: the row keys lie behind everything else in the entropy buffer (32 bytes per row more than the uploaded rows take)
                for (int k = 0; ctx->entropy_source == BBP_ENTROPY_SOURCE_HEDGED && k < bbp_ctx::IO_SLOTS && rc == BBP_OK; k++)
                    rc = staging_reserve(ctx, ctx->io[k], ProveStaging(B, N, false, check, true, true));
                for (int k = 0; k < bbp_ctx::CHECK_RING && rc == BBP_OK; k++)
                    if (!(rc = dev_reserve(ctx, ctx->rnd[k].buf, RoundRing(B, N, true).bytes)) && check) rc = dev_reserve(ctx, ctx->chk[k].buf, CheckRing(B, N).bytes);
                // the draw buffers, one per stream that opens (ProvePlan::raw_index): side's has seen a call of B; the others open dual calls
                // only, below dual_open_below proofs or up to rotate_deep_max in a deep pipeline, and the warm-up reaches those sizes only
                // while B itself is one (a deep warm-up call is skipped beyond rotate_deep_max)
                const CircuitDev* c = nullptr;
                if (rc == BBP_OK && !(rc = circuit_get(ctx, N, &c))) {
                    const uint32_t dual_max = std::max((uint32_t)std::max(ctx->knobs.dual_open_below - 1, 0), ctx->knobs.deep_eligible(1) ? (uint32_t)ctx->knobs.rotate_deep_max : 0u);
                    for (auto& r : ctx->raw)
                        if (rc == BBP_OK) rc = dev_reserve(ctx, r, (size_t)std::min(B, dual_max) * (3 + 2 * (size_t)c->n_mul) * 64);
                    // ... at the merlin draw's size whatever bbp_set_blinding_draw says (the expanded draw keeps 32 bytes per proof there: a
                    // subset), side's too: a context reserved in one mode allocates nothing in the other
                    if (rc == BBP_OK) rc = dev_reserve(ctx, ctx->raw[0], (size_t)B * (3 + 2 * (size_t)c->n_mul) * 64);
                }
                return rc;
            });
        return rc;
    });
}

// The blinding draw of prove calls (include/bbp.h "Expanded blinding draw"): the setting lives in the prove knobs, where plan_prove reads it.
extern "C" int32_t bbp_set_blinding_draw(bbp_ctx* ctx, int32_t mode) {
    if (!ctx || (mode != BBP_BLINDING_DRAW_MERLIN && mode != BBP_BLINDING_DRAW_EXPANDED)) return BBP_ERR_BAD_ARG;
    for (bbp_ctx* m : ctx->members)
        if (int32_t rc = bbp_set_blinding_draw(m, mode)) return rc;
    return api_guard(ctx, [&]() -> int32_t {
        ctx->knobs.blinding_draw = mode;
        return BBP_OK;
    });
}

extern "C" int32_t bbp_blinding_draw(bbp_ctx* ctx) {
    if (!ctx) return -1;  // (the modes are 0 and 1: no status code fits here)
    int32_t mode = -1;
    api_guard(ctx, [&]() -> int32_t {
        mode = ctx->knobs.blinding_draw;
        return BBP_OK;
    });
    return mode;
}

extern "C" int32_t bbp_set_batching(bbp_ctx* ctx, uint32_t window_us, uint32_t max_batch) {
    if (!ctx || !ctx->combiner) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        static_cast<Combiner*>(ctx->combiner)->configure(window_us, max_batch);
        return BBP_OK;
    });
}

extern "C" int32_t bbp_set_verify_mixing(bbp_ctx* ctx, int32_t on) {
    if (!ctx || !ctx->combiner) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        static_cast<Combiner*>(ctx->combiner)->set_verify_mixing(on != 0);
        return BBP_OK;
    });
}

extern "C" int32_t bbp_set_verify_round_sharing(bbp_ctx* ctx, int32_t on) {
    if (!ctx || !ctx->combiner) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        static_cast<Combiner*>(ctx->combiner)->set_round_sharing(on != 0);
        return BBP_OK;
    });
}

extern "C" int32_t bbp_verify_round_sharing_stats(bbp_ctx* ctx, uint64_t* n_calls, uint64_t* n_rows, uint64_t* n_rounds) {
    if (!ctx || !ctx->combiner) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        if (ctx->owner && ctx->owner->combiner)  // a pool member: the rounds calls its pool's combiner has dealt to it
            static_cast<Combiner*>(ctx->owner->combiner)->target_round_stats(ctx->member_index, n_calls, n_rows, n_rounds);
        else
            static_cast<Combiner*>(ctx->combiner)->round_stats(n_calls, n_rows, n_rounds);
        return BBP_OK;
    });
}

extern "C" int32_t bbp_batching_stats(bbp_ctx* ctx, uint64_t* n_calls, uint64_t* n_requests, uint32_t* max_seen) {
    if (!ctx || !ctx->combiner) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        if (ctx->owner && ctx->owner->combiner) {  // a pool member: the batches its pool's combiner has dealt to it
            static_cast<Combiner*>(ctx->owner->combiner)->target_stats(ctx->member_index, n_calls, n_requests);
            if (max_seen) *max_seen = 0;
            return BBP_OK;
        }
        static_cast<Combiner*>(ctx->combiner)->stats(n_calls, n_requests, max_seen);
        return BBP_OK;
    });
}

extern "C" int32_t bbp_debug_challenges(bbp_ctx* ctx, uint32_t B, uint32_t N, uint32_t proof, uint8_t* out32x32) {
    if (!ctx || !out32x32 || proof >= B) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_challenges");
    return api_guard(ctx, [&]() -> int32_t {
        if (wipe_on(ctx)) return ctx->err = "bbp_debug_challenges: secret wiping is on, the challenge block has been erased", BBP_ERR_BAD_ARG;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BBP_HIP_TRY(ctx, hipDeviceSynchronize());
        return debug_read_misc(ctx, B, N, proof, out32x32);
    });
}

extern "C" int32_t bbp_debug_table(bbp_ctx* ctx, uint32_t which, const void** dev, uint64_t* bytes) {
    const uint32_t kind = which & 0xffu, N = which >> 8;
    if (!ctx || !dev || !bytes || kind > BBP_TABLE_IDX_VER) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_table");
    if (kind < BBP_TABLE_IDX_AI ? N != 0 : N == 0) return BBP_ERR_BAD_ARG;  // screened here: no circuit is synthesised for a length
    if (N > BBP_MAX_ITEMS) return BBP_ERR_GENS_LEN;                          // the engine cannot prove
    return api_guard(ctx, [&]() -> int32_t {
        if (kind >= BBP_TABLE_IDX_AI) {  // the base-index lists of circuit N (msm_index.h, uploaded by circuit_get), compiled now if need be
            BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
            const CircuitDev* c;
            if (int32_t rc = circuit_get(ctx, N, &c)) return rc;
            const uint64_t n1 = c->n_mul;
            switch (kind) {
                case BBP_TABLE_IDX_AI: *dev = c->idx_ai, *bytes = 4 * (1 + 2 * n1); break;
                case BBP_TABLE_IDX_AO: *dev = c->idx_ao, *bytes = 4 * (1 + n1); break;
                case BBP_TABLE_IDX_S1: *dev = c->idx_s1, *bytes = 4 * (1 + 2 * n1); break;
                case BBP_TABLE_IDX_IPA: *dev = c->idx_ipa, *bytes = 4 * (uint64_t)(IPA_ROUNDS * 2 * IPA_TERMS); break;
                default: *dev = c->idx_ver, *bytes = 4 * 4098; break;
            }
            return BBP_OK;
        }
        switch (kind) {
            case BBP_TABLE_GENS: *dev = ctx->gens, *bytes = sizeof(ge) * (uint64_t)TAB_BASES; break;
            case BBP_TABLE_PTABLE: *dev = ctx->ptable, *bytes = sizeof(niels_row) * (uint64_t)TAB_BASES * MSM_POS; break;
            case BBP_TABLE_COMB: *dev = ctx->comb, *bytes = sizeof(niels_packed) * 2 * 64 * 8; break;
            default: *dev = ctx->btab, *bytes = tail_btab_bytes(); break;
        }
        return BBP_OK;
    });
}

extern "C" int32_t bbp_debug_varbase(bbp_ctx* ctx, uint32_t form, uint32_t B, uint32_t Q, uint32_t agg, const uint32_t* ns, const uint8_t* vers,
                                     const uint8_t* pts, const uint8_t* scalars, const uint8_t* wv, const uint8_t* uj, uint8_t* sums_out,
                                     uint32_t* digits_out, int32_t* status_out) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_varbase");
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        return debug_varbase(ctx, form, B, Q, agg, ns, vers, pts, scalars, wv, uj, sums_out, digits_out, status_out);
    });
}

extern "C" int32_t bbp_set_profiling(bbp_ctx* ctx, int32_t on) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_set_profiling");
    return api_guard(ctx, [&]() -> int32_t {
        ctx->profile = on != 0;
        return BBP_OK;
    });
}

// Drains the recorded events: out[2i] = kernel tag, out[2i+1] = microseconds. Synchronises the device.
extern "C" int32_t bbp_last_timings(bbp_ctx* ctx, float* out, uint32_t cap, uint32_t* n) {
    if (!ctx || !n) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_last_timings");
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BBP_HIP_TRY(ctx, hipDeviceSynchronize());
        uint32_t k = 0;
        for (auto& e : ctx->events) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess && out && 2 * k + 1 < cap) {
                out[2 * k] = (float)e.tag;
                out[2 * k + 1] = ms * 1000.f;
                k++;
            }
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        ctx->events.clear();
        *n = 2 * k;
        return BBP_OK;
    });
}
