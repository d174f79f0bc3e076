// C-ABI, every verify entry point and the host-pointer verify path behind them -- see include/bbp.h.
#include <string.h>

#include "capi.h"

using namespace bbp;

// The host-pointer verify path of one context; `rows` says what `in` holds (verify_rows.h; a rounds call: its table in host memory,
// uploaded behind the rows in the same staging slot).  Takes the context lock itself, for the enqueue phase only.
int32_t bbp::verify_batch_host(bbp_ctx* ctx, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group, uint32_t* n_fallback) {
    const uint32_t B = rows.B, N = rows.kind == VerifyRows::UNIFORM ? rows.N : 0;
    // Verifier::verify mixes thread_rng into its TranscriptRng (A.7): 32 OS bytes per proof, or (source DEVICE) rows of one key
    const bool dev_draw = ctx->entropy_source.load() != BBP_ENTROPY_SOURCE_OS;  // HEDGED: as DEVICE (a verify row carries no secret to hedge with)
    const VerifyStaging st(rows, group, (uint32_t)ctx->vknobs.group, dev_draw, host_chunk_verify());  // BBP_VERIFY_AGGREGATE, BBP_HOST_CHUNK_VERIFY
    ChachaKey key{};
    std::vector<uint8_t> ent(st.ent_up_bytes);
    if (dev_draw) {
        if (int32_t rc = next_device_key(ctx, &key)) return rc;
    } else if (!os_random(ent.data(), ent.size())) {
        return no_os_random(ctx);
    }
    SlotLease lease(ctx, true);
    bbp_ctx::IoSlot& sl = *lease.sl;
    bbp_ctx::VLane& L = ctx->vl[(&sl - ctx->io) - bbp_ctx::IO_SLOTS];  // verifier lane = staging slot: consecutive host calls overlap on the device
    int32_t rc = api_guard(ctx, [&]() -> int32_t {
        int32_t rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = dev_reserve(ctx, sl.out, st.out_bytes)) || (rc = pinned_reserve(ctx, sl.h_out, sl.h_cap, st.out_bytes)) ||
            (rc = upload_inputs(ctx, sl, in, st.in_bytes, ent.data(), ent.size(), st.ent_drawn, rows.rounds, st.tab_bytes, st.tab_off)))
            return rc;
        if (dev_draw && (rc = draw_enqueue(ctx, B, N, BBP_ENTROPY_VERIFY, key, 0, sl.ent.p, L.stream))) return rc;  // ahead of every chunk on the lane
        for (uint32_t first = 0; first < B; first += st.chunk) {
            const uint32_t nb = B - first < st.chunk ? B - first : st.chunk;
            const u8 *cin = (const u8*)sl.in.p + st.row_off[first], *cent = (const u8*)sl.ent.p + 32 * (size_t)first;
            int32_t* cst = (int32_t*)sl.out.p + first;
            VerifyRows c = rows.slice(first, first + nb);  // a chunk may begin and end inside a round: it takes the whole table
            if (c.rounds) c.rounds = (const u8*)sl.in.p + st.tab_off;
            if (st.group > 1) {  // stream-ordered: no synchronisation while the context lock is held
                if (first == 0 && L.agg_count) BBP_HIP_TRY(ctx, hipMemsetAsync(L.agg_count + 1, 0, sizeof(u32), L.stream));
                if ((rc = verify_batch_agg_dev(ctx, c, st.group, cin, cent, cst, L.stream, nullptr, (u32*)sl.out.p + B))) return rc;
            } else if ((rc = verify_batch_dev(ctx, c, 0, cin, cent, cst, L.stream)))
                return rc;
        }
        BBP_HIP_TRY(ctx, hipEventRecord(sl.ev, L.stream));
        return BBP_OK;
    });
    if (rc) return rc;
    if ((rc = fetch_results(ctx, sl, st.fetch_bytes))) return rc;
    memcpy(status, sl.h_out, 4 * (size_t)B);
    if (st.group > 1 && n_fallback) memcpy(n_fallback, (const uint8_t*)sl.h_out + 4 * (size_t)B, 4);  // running total of this call's chunks
    return BBP_OK;
}

int32_t bbp::verify_host(bbp_ctx* ctx, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group, uint32_t* n_fallback) {
    return no_throw_ctx(ctx, [&]() -> int32_t {
        return is_pool(ctx) ? pool_verify(ctx, rows, in, status, group, n_fallback) : verify_batch_host(ctx, rows, in, status, group, n_fallback);
    });
}

int32_t bbp::verify_batch_locked(bbp_ctx* ctx, uint32_t B, uint32_t N, uint32_t rec_ver, const uint8_t* in, int32_t* status,
                                 std::string* err) {
    const int32_t rc = no_throw_ctx(ctx, [&]() -> int32_t { return verify_batch_host(ctx, VerifyRows::uniform(B, N, rec_ver), in, status); });
    if (rc && err) *err = tls_error();
    return rc;
}

// what the call combiner runs for concurrent bbp_verify callers of different bid-list lengths or record layouts (submit.cpp: the
// runner handed to Combiner::set_mixed_verify).  Ns and vers come from requests that bbp_verify has screened.
int32_t bbp::verify_batch_mixed_locked(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const uint8_t* vers, const uint8_t* in, int32_t* status,
                                       std::string* err) {
    const int32_t rc = no_throw_ctx(ctx, [&]() -> int32_t { return verify_batch_host(ctx, VerifyRows::mixed(B, Ns, vers), in, status); });
    if (rc && err) *err = tls_error();
    return rc;
}

// what the call combiner runs for concurrent bbp_verify callers that share rounds (submit.cpp: the runner handed to
// Combiner::set_round_verify): bbp_verify_rounds' path from verify_host down -- the host chunk loop, the health word, device entropy,
// the aggregated engine when the context verifies aggregated.  Table and rows come from requests that bbp_verify has screened.
int32_t bbp::verify_rounds_locked(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                                  const uint8_t* rows, int32_t* status, std::string* err) {
    const int32_t rc = verify_host(ctx, VerifyRows::of_rounds(B, R, round_Ns, rounds, round_of), rows, status, 0, nullptr);
    if (rc && err) *err = tls_error();
    return rc;
}

// ---- the twelve verify entry points: uniform, mixed-N, rounds (include/bbp.h) x host / device pointers x plain / aggregated --------
// Every row's N is screened on the host before anything is verified: a 0 anywhere is BBP_ERR_BAD_ARG, else an N above
// BBP_MAX_ITEMS anywhere is BBP_ERR_GENS_LEN -- what a uniform call with that N returns.
static int32_t check_ns(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns) {
    for (uint32_t i = 0; i < B; i++)
        if (Ns[i] == 0) return check_n(ctx, 0);
    for (uint32_t i = 0; i < B; i++)
        if (Ns[i] > BBP_MAX_ITEMS) return check_n(ctx, Ns[i]);
    return BBP_OK;
}

// Screening of a call's layout, under the context lock.  Rounds: R, then check_ns's order over all R entries, then round_of.
static int32_t check_rows(bbp_ctx* ctx, const VerifyRows& v) {
    if (v.kind == VerifyRows::UNIFORM) return check_n(ctx, v.N);
    if (v.kind == VerifyRows::MIXED) return check_ns(ctx, v.B, v.ns);
    if (v.R == 0) return ctx->err = "bbp_verify_rounds: no rounds", BBP_ERR_BAD_ARG;
    if (int32_t rc = check_ns(ctx, v.R, v.round_ns)) return rc;
    if (!v.round_of && v.R > 1) return ctx->err = "bbp_verify_rounds: round_of may be NULL with one round only", BBP_ERR_BAD_ARG;
    if (v.round_of)
        for (uint32_t i = 0; i < v.B; i++)
            if (v.round_of[i] >= v.R) return ctx->err = "bbp_verify_rounds: round_of names a round beyond R", BBP_ERR_BAD_ARG;
    return BBP_OK;
}

// The order is part of every form's behaviour: *n_fallback zeroed first; the NULL checks (layout_ok: the form's own array arguments);
// device forms refuse a pool before any screening; uniform and mixed forms are screened BEFORE the B == 0 return, a rounds form
// returns BBP_OK for B == 0 before its table is looked at.
static int32_t verify_entry_host(bbp_ctx* ctx, bool layout_ok, const VerifyRows& rows, const uint8_t* in, int32_t* status, bool aggregated,
                                 uint32_t group, uint32_t* n_fallback) {
    if (n_fallback) *n_fallback = 0;
    if (!ctx || !layout_ok || !in || !status) return BBP_ERR_BAD_ARG;
    if (rows.kind == VerifyRows::ROUNDS && rows.B == 0) return BBP_OK;
    const int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_rows(ctx, rows); });
    if (rc || rows.B == 0) return rc;
    return verify_host(ctx, rows, in, status, aggregated ? (group ? group : BBP_AGG_GROUP_DEFAULT) : 0, n_fallback);
}

static int32_t verify_entry_dev(bbp_ctx* ctx, const char* what, bool layout_ok, const VerifyRows& rows, const void* in_dev, const void* entropy_dev,
                                void* status_dev, bool aggregated, uint32_t group, uint32_t* n_fallback, void* stream) {
    if (n_fallback) *n_fallback = 0;
    if (!ctx || !layout_ok || !in_dev || !entropy_dev || !status_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, what);
    return api_guard(ctx, [&]() -> int32_t {
        if (rows.kind == VerifyRows::ROUNDS && rows.B == 0) return BBP_OK;
        const int32_t rc = check_rows(ctx, rows);
        if (rc || rows.B == 0) return rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (aggregated)
            return verify_batch_agg_dev(ctx, rows, group ? group : BBP_AGG_GROUP_DEFAULT, (const u8*)in_dev, (const u8*)entropy_dev, (int32_t*)status_dev,
                                        pick_stream(ctx, stream), n_fallback);
        return verify_batch_dev(ctx, rows, 0, (const u8*)in_dev, (const u8*)entropy_dev, (int32_t*)status_dev, pick_stream(ctx, stream));
    });
}

extern "C" int32_t bbp_verify_batch(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, int32_t* status) {
    return verify_entry_host(ctx, true, VerifyRows::uniform(B, N), in, status, false, 0, nullptr);
}

extern "C" int32_t bbp_verify_batch_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev,
                                        void* status_dev, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_batch_dev", true, VerifyRows::uniform(B, N), in_dev, entropy_dev, status_dev, false, 0, nullptr, stream);
}

extern "C" int32_t bbp_verify_batch_aggregated(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, int32_t* status, uint32_t group,
                                               uint32_t* n_fallback) {
    return verify_entry_host(ctx, true, VerifyRows::uniform(B, N), in, status, true, group, n_fallback);
}

extern "C" int32_t bbp_verify_batch_aggregated_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev,
                                                   void* status_dev, uint32_t group, uint32_t* n_fallback, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_batch_aggregated_dev", true, VerifyRows::uniform(B, N), in_dev, entropy_dev, status_dev, true, group,
                            n_fallback, stream);
}

// mixed-N verification: rows of any mix of bid-list lengths in one call
extern "C" int32_t bbp_verify_batch_mixed(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const uint8_t* in, int32_t* status) {
    return verify_entry_host(ctx, !B || Ns, VerifyRows::mixed(B, Ns), in, status, false, 0, nullptr);
}

extern "C" int32_t bbp_verify_batch_mixed_aggregated(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const uint8_t* in, int32_t* status, uint32_t group,
                                                     uint32_t* n_fallback) {
    return verify_entry_host(ctx, !B || Ns, VerifyRows::mixed(B, Ns), in, status, true, group, n_fallback);
}

extern "C" int32_t bbp_verify_batch_mixed_dev(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const void* in_dev, const void* entropy_dev,
                                              void* status_dev, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_batch_mixed_dev", !B || Ns, VerifyRows::mixed(B, Ns), in_dev, entropy_dev, status_dev, false, 0, nullptr,
                            stream);
}

extern "C" int32_t bbp_verify_batch_mixed_aggregated_dev(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const void* in_dev, const void* entropy_dev,
                                                         void* status_dev, uint32_t group, uint32_t* n_fallback, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_batch_mixed_aggregated_dev", !B || Ns, VerifyRows::mixed(B, Ns), in_dev, entropy_dev, status_dev, true,
                            group, n_fallback, stream);
}

// rounds: proofs that share a seed and a bid list, sent once per round
extern "C" uint32_t bbp_round_row_size(uint32_t N) { return (uint32_t)round_row_bytes(N); }

extern "C" int32_t bbp_verify_rounds(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                                     const uint8_t* rows, int32_t* status) {
    return verify_entry_host(ctx, round_Ns && rounds, VerifyRows::of_rounds(B, R, round_Ns, rounds, round_of), rows, status, false, 0, nullptr);
}

extern "C" int32_t bbp_verify_rounds_aggregated(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B,
                                                const uint32_t* round_of, const uint8_t* rows, int32_t* status, uint32_t group, uint32_t* n_fallback) {
    return verify_entry_host(ctx, round_Ns && rounds, VerifyRows::of_rounds(B, R, round_Ns, rounds, round_of), rows, status, true, group, n_fallback);
}

extern "C" int32_t bbp_verify_rounds_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B, const uint32_t* round_of,
                                         const void* rows_dev, const void* entropy_dev, void* status_dev, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_rounds_dev", round_Ns && rounds_dev, VerifyRows::of_rounds(B, R, round_Ns, (const u8*)rounds_dev, round_of),
                            rows_dev, entropy_dev, status_dev, false, 0, nullptr, stream);
}

extern "C" int32_t bbp_verify_rounds_aggregated_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B,
                                                    const uint32_t* round_of, const void* rows_dev, const void* entropy_dev, void* status_dev,
                                                    uint32_t group, uint32_t* n_fallback, void* stream) {
    return verify_entry_dev(ctx, "bbp_verify_rounds_aggregated_dev", round_Ns && rounds_dev,
                            VerifyRows::of_rounds(B, R, round_Ns, (const u8*)rounds_dev, round_of), rows_dev, entropy_dev, status_dev, true, group,
                            n_fallback, stream);
}

// Structural parse exactly as R1CSProof::from_bytes / InnerProductProof::from_bytes order their checks: a record of
// any length is either a FormatError, or well formed with a wrong IPA depth (-> VerificationError from verification_scalars,
// n != 2^lg_n), or one of the two layouts the device kernels take (*ver).  BBP_OK = hand it to the device.
static int32_t screen_verify_args(const uint8_t* record, uint32_t record_len, const uint8_t score[32], const uint8_t z_img[32],
                                  const uint8_t seed[32], uint32_t N, uint8_t* ver_out) {
    const uint32_t tail = 32u * (4u + N);
    if (record_len < tail + 1u) return BBP_ERR_FORMAT;
    const uint32_t plen = record_len - tail;
    const uint8_t ver = record[0];
    if (ver != 0 && ver != 1) return BBP_ERR_FORMAT;
    if ((plen - 1u) % 32u != 0) return BBP_ERR_FORMAT;
    const uint32_t nel = (plen - 1u) / 32u, npts = ver == 0 ? 3u : 6u;
    if (nel < npts + 5u + 3u + 2u) return BBP_ERR_FORMAT;
    auto canonical = [&](uint32_t el) {
        u32 w[8];
        memcpy(w, record + 1 + 32 * (size_t)el, 32);
        return sc_is_canonical(w);
    };
    for (uint32_t k = 0; k < 3; k++)
        if (!canonical(npts + 5u + k)) return BBP_ERR_FORMAT;  // t_x, t_x_blinding, e_blinding
    const uint32_t ipp_el = nel - npts - 8u;
    if (ipp_el < 2u || (ipp_el - 2u) % 2u != 0) return BBP_ERR_FORMAT;
    const uint32_t lg_n = (ipp_el - 2u) / 2u;
    if (lg_n >= 32u) return BBP_ERR_FORMAT;
    if (!canonical(nel - 2u) || !canonical(nel - 1u)) return BBP_ERR_FORMAT;  // a, b
    // score, z_img, seed reach Verify::new as serde-deserialised Scalars (verify.rs:100-104): canonical encodings only
    for (const uint8_t* pub : {score, z_img, seed}) {
        u32 w[8];
        memcpy(w, pub, 32);
        if (!sc_is_canonical(w)) return BBP_ERR_FORMAT;
    }
    if (lg_n != 11u) return BBP_ERR_VERIFY;  // padded_n = 2048 != 2^lg_n
    *ver_out = ver;
    return BBP_OK;
}

static void fill_verify_input(std::vector<uint8_t>& in, const uint8_t* record, uint32_t record_len, const uint8_t score[32],
                              const uint8_t z_img[32], const uint8_t seed[32], const uint8_t* pub_list, uint32_t N) {
    in.resize((size_t)record_len + 96 + (size_t)N * 32);
    memcpy(&in[0], record, record_len);
    memcpy(&in[record_len], score, 32);
    memcpy(&in[record_len + 32], z_img, 32);
    memcpy(&in[record_len + 64], seed, 32);
    memcpy(&in[record_len + 96], pub_list, (size_t)N * 32);
}

extern "C" int32_t bbp_verify(bbp_ctx* ctx, const uint8_t* record, uint32_t record_len, const uint8_t score[32], const uint8_t z_img[32],
                              const uint8_t seed[32], const uint8_t* pub_list, uint32_t N) {
    if (!ctx || !record || !score || !z_img || !seed) return BBP_ERR_BAD_ARG;
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc) return rc;
    if (!pub_list) return BBP_ERR_BAD_ARG;
    uint8_t ver = 0;
    if ((rc = screen_verify_args(record, record_len, score, z_img, seed, N, &ver))) {
        set_tls_error(ctx, rc == BBP_ERR_FORMAT ? "malformed proof record or non-canonical public scalar" : "inner-product proof of the wrong depth");
        return rc;
    }
    return no_throw([&]() -> int32_t {
        std::vector<uint8_t> in;
        fill_verify_input(in, record, record_len, score, z_img, seed, pub_list, N);
        Request r;
        r.kind = 1;
        r.N = N;
        r.rec_ver = ver;
        r.in = in.data();
        r.in_len = in.size();
        Combiner* const comb = static_cast<Combiner*>(ctx->combiner);
        if (comb->round_sharing()) {  // on the caller's thread: the cost spreads over the callers
            r.round_hash = hash_bytes(r.in + record_len + 64, round_bytes(N));
            r.round_hash_valid = true;
        }
        const int32_t st = comb->submit(ctx, r);
        if (st != BBP_OK) set_tls_error(ctx, !r.err.empty() ? r.err : st == BBP_ERR_VERIFY ? "proof rejected" : "malformed proof");
        return st;
    }, ctx);
}

extern "C" int32_t bbp_verify_async(bbp_ctx* ctx, const uint8_t* record, uint32_t record_len, const uint8_t score[32],
                                    const uint8_t z_img[32], const uint8_t seed[32], const uint8_t* pub_list, uint32_t N, bbp_done_fn done,
                                    void* user) {
    if (!ctx || !record || !score || !z_img || !seed || !done) return BBP_ERR_BAD_ARG;
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc) return rc;
    if (!pub_list) return BBP_ERR_BAD_ARG;
    uint8_t ver = 0;
    if ((rc = screen_verify_args(record, record_len, score, z_img, seed, N, &ver))) return rc;  // decided on the host: no callback
    return no_throw([&]() -> int32_t {
        Request* r = new Request();
        r->kind = 1;
        r->N = N;
        r->rec_ver = ver;
        fill_verify_input(r->own_in, record, record_len, score, z_img, seed, pub_list, N);
        r->in = r->own_in.data();
        r->in_len = r->own_in.size();
        r->on_done = async_done;
        r->origin = ctx;
        r->user_fn = done;
        r->user = user;
        Combiner* const comb = static_cast<Combiner*>(ctx->combiner);
        if (comb->round_sharing()) {
            r->round_hash = hash_bytes(r->in + record_len + 64, round_bytes(N));
            r->round_hash_valid = true;
        }
        if (!comb->submit_async(ctx, r)) {
            delete r;
            set_tls_error(ctx, "call combiner: cannot start a batch thread");
            return BBP_ERR_INTERNAL;
        }
        return BBP_OK;
    }, ctx);
}
