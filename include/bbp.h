/* bbp.h -- C ABI of the MI355X blind-bid Bulletproofs engine (libbbp_hip.so).
 *
 * The reference (dusk-network/dusk-blindbidproof) has no FFI layer of its own: its hot path sits behind two
 * `pub` Rust functions and two IPC opcodes.  Each entry point below names the reference interface it replaces;
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add in src/blindbid/{proof,verify}.rs.
 *
 * Conventions: all scalars are 32-byte little-endian; points are 32-byte ristretto255 encodings; every buffer is
 * caller-owned host memory unless the name ends in `_dev`; functions return a bbp_status; nothing throws or
 * aborts across this boundary (the reference builds with panic='abort', Cargo.toml:29 -- see SURVEY.md 5): every entry point
 * runs inside a try/catch barrier and turns a C++ exception into BBP_ERR_INTERNAL / BBP_ERR_BAD_ARG.
 * The library has NO CPU compute path: bbp_init fails with BBP_ERR_DEVICE when no gfx950 device is usable.
 *
 * Threading (SURVEY.md 8b "thread-safe after bbp_init"): the reference serves every connection on its own worker thread
 * (src/main.rs:55, src/futures/main.rs:46-56, one Proof::prove / Verify::verify per thread).  ONE context may be shared by any
 * number of host threads: each entry point takes the context's lock, and concurrent bbp_prove / bbp_verify calls are coalesced
 * into batch calls on the device (group commit: whatever queued up while the previous batch ran goes out as the next batch), so
 * N concurrent single proofs cost about one batch of N, not N times one.  bbp_last_error is per calling thread.
 * bbp_free must not race with other calls on the same context; asynchronous requests still queued when it is called are run first
 * (their callbacks fire before bbp_free returns).
 *
 * Several GPUs: bbp_init_all / bbp_pool_init return a POOL handle -- one context per GPU behind the same bbp_ctx* type -- that the
 * host-pointer entry points accept like a context: the reference's worker threads keep calling bbp_prove / bbp_verify on ONE
 * shared handle and every GPU of the node works (see "Device pool" below).
 */
#ifndef BBP_H
#define BBP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbp_ctx bbp_ctx;

typedef enum {
    BBP_OK = 0,
    BBP_ERR_VERIFY = 1,    /* R1CSError::VerificationError (src/error.rs:22 via bulletproofs)            */
    BBP_ERR_GENS_LEN = 2,  /* R1CSError::InvalidGeneratorsLength: N > 202 needs > 2048 multipliers       */
    BBP_ERR_FORMAT = 3,    /* R1CSError::FormatError / Error::Io(InvalidData|UnexpectedEof) (error.rs)    */
    BBP_ERR_BAD_ARG = 4,   /* N == 0 or toggle >= N: the reference panics (src/gadgets.rs:103) or proves garbage */
    BBP_ERR_DEVICE = 5,    /* HIP failure / no device                                                     */
    BBP_ERR_INTERNAL = 6   /* host-side failure (allocation, internal invariant, any C++ exception): reported, never thrown */
} bbp_status;

#define BBP_MIMC_ROUNDS 90      /* src/gadgets.rs:4 */
#define BBP_GENS_CAPACITY 2048  /* src/blindbid/mod.rs:36 */
#define BBP_MAX_ITEMS 202       /* 1442 + 3N <= 2048 */
#define BBP_R1CS_PROOF_BYTES 1121 /* 1-phase compact R1CSProof::to_bytes */

/* Base-table indices for bbp_msm_batch layouts (device generator table order). */
#define BBP_BASE_BBLIND 0u /* PedersenGens::B_blinding */
#define BBP_BASE_G0 1u     /* BulletproofGens G[0..2048) */
#define BBP_BASE_H0 2049u  /* BulletproofGens H[0..2048) */
#define BBP_BASE_B 4097u   /* PedersenGens::B (ristretto basepoint) */
#define BBP_NUM_BASES 4098u

/* Layout ids for bbp_msm_batch. */
#define BBP_LAYOUT_BLIND_G_H 0u /* terms: B_blinding, G[0..m), H[0..m); n_terms = 1 + 2m  (A_I1, S1)   */
#define BBP_LAYOUT_BLIND_G 1u   /* terms: B_blinding, G[0..m);          n_terms = 1 + m   (A_O1)       */

/* Replaces generate_cs_transcript()'s per-call generator derivation (src/blindbid/mod.rs:34-40) and the
 * lazy_static CONSTANTS (src/blindbid/mod.rs:7-24): derives them ONCE on `device` and keeps them resident.
 * `device` is a HIP device ordinal (one context per GPU / per rank); -1 = a pool over every visible GPU (bbp_init_all below). */
int32_t bbp_init(int32_t device, bbp_ctx** out);

/* ---- Device pool -----------------------------------------------------------------------------------------------------------------
 * The reference's concurrency model is "one Proof::prove / Verify::verify per worker thread, all threads share the process-wide
 * state" (src/main.rs:55, src/futures/main.rs:46-56).  On a node with several GPUs that shared state is a pool: ONE handle, one
 * ordinary context per GPU behind it (tables replicated per GPU, no data ever crosses between GPUs -- proofs are independent).
 *   bbp_init_all            one member per visible HIP device (every one must be gfx950); bbp_init(-1, &h) is the same call
 *   bbp_pool_init           an explicit device list; a device may be named more than once (two members on one card: tests, or two
 *                           engine pipelines per GPU)
 * What a pool handle accepts:
 *   bbp_prove / bbp_verify  ONE call combiner for the whole pool: concurrent callers are coalesced into device batches as on a
 *                           single context, and every batch goes to the member with the fewest batches in flight; a burst is cut
 *                           into fair shares over the idle members
 *   bbp_prove_batch / bbp_verify_batch / bbp_verify_batch_aggregated / bbp_msm_batch
 *                           contiguous block split by index over the members (block sizes differ by at most one: member i of n
 *                           gets [i*B/n ...), the split of SURVEY.md 8e), one host thread per member, outputs and per-item
 *                           statuses in request order; the call returns the first member's non-zero status, if any
 *   bbp_witness_batch, bbp_get_generator, bbp_get_mimc_constant, bbp_ubench   served by member 0
 *   bbp_prove_round_select  scoring and selection served by member 0, the selected bids proved as bbp_prove_round on the pool
 *   bbp_verify_round_best   keys, selection and marks served by member 0, every tranche verified as bbp_verify_rounds_aggregated on the pool
 *   bbp_verify_round_best_distinct   the same: keys, identities, selection and marks on member 0, tranches verified on the pool
 *   bbp_verify_rounds_best  the same over many rounds: keys, segments, selection and marks on member 0, every step verified on the pool
 *   bbp_verify_rounds_best_distinct   the same, one per bidder: identities and drops on member 0 as well, every step verified on the pool
 *   bbp_standing_open / _offer / _read / _close   a standing's state lives on member 0, an offer's tranches are verified on the pool
 *   bbp_check_health        the members' flags OR-ed;  bbp_set_batching / bbp_batching_stats: the pool's combiner
 *   bbp_free                frees the members too
 * What it refuses (BBP_ERR_BAD_ARG; device pointers and streams belong to one device -- take a member with bbp_pool_member and
 * call it directly): every *_dev entry point, bbp_debug_challenges, bbp_debug_table, bbp_debug_varbase, bbp_debug_round_select, bbp_debug_round_best,
 * bbp_debug_round_best_distinct, bbp_debug_standing_offer, bbp_debug_standing_trip, bbp_debug_rounds_best, bbp_debug_rounds_best_distinct, bbp_set_profiling /
 * bbp_last_timings; the stream getters return NULL. */
int32_t bbp_init_all(bbp_ctx** out);
int32_t bbp_pool_init(const int32_t* devices, uint32_t n_devices, bbp_ctx** out);
uint32_t bbp_pool_size(const bbp_ctx* ctx);               /* number of members; 0 for an ordinary context */
bbp_ctx* bbp_pool_member(bbp_ctx* ctx, uint32_t i);        /* borrowed: owned and freed by the pool */
/* combined bbp_prove / bbp_verify device calls the pool has dealt to member i, and the requests they carried
 * (bbp_batching_stats on the member handle reports the same pair) */
int32_t bbp_pool_member_stats(bbp_ctx* ctx, uint32_t i, uint64_t* n_calls, uint64_t* n_requests);

/* `stream` arguments of the _dev entry points: a hipStream_t of the caller -- NULL is the legacy default stream and is honoured
 * as such -- or BBP_STREAM_CONTEXT for the context's own (non-blocking) stream. */
#define BBP_STREAM_CONTEXT ((void*)(intptr_t)-1)
/* The context's own stream as a hipStream_t, for callers that want to enqueue their own work (copies, consumers of the records)
 * in order with the engine's: passing this handle is the same as passing BBP_STREAM_CONTEXT.  Recommended for throughput: the
 * engine's four streams are created together at bbp_init and land on distinct hardware queues, whereas a stream the caller
 * created elsewhere may share a hardware queue with one of them (measured on MI355X: 61.5 vs 55.6 ms per 1024-proof batch
 * with a stream from PyTorch's pool as the caller's stream). */
void* bbp_context_stream(bbp_ctx* ctx);
/* A second stream of the context that the engine itself leaves idle, for the caller's ingest side (H2D copies of the next chunk,
 * bbp_prepare_bids_dev) while the first one carries prove / verify calls: same reason as above -- created at bbp_init beside
 * the engine's streams, it does not share a hardware queue with them. */
void* bbp_context_copy_stream(bbp_ctx* ctx);
/* The verifier has four independent lanes (own scratch each): calls issued on the streams of different lanes (lane < 4; NULL beyond)
 * overlap on the device -- the latency-bound front end of one runs under the MSM of another -- instead of being ordered one behind
 * the other like calls on any other pair of streams.  The host-pointer verify calls rotate over the lanes by themselves. */
void* bbp_context_verify_stream(bbp_ctx* ctx, uint32_t lane);
void bbp_free(bbp_ctx* ctx);
const char* bbp_last_error(const bbp_ctx* ctx);

/* Setup read-back for parity tests: compressed generator `index` (table order above) / MiMC constant i. */
int32_t bbp_get_generator(bbp_ctx* ctx, uint32_t index, uint8_t out32[32]);
int32_t bbp_get_mimc_constant(bbp_ctx* ctx, uint32_t i, uint8_t out32[32]);

/* Kernel-level hook (BASELINE.json configs[1]): B independent multiscalar multiplications over the shared
 * generator table; what bulletproofs' Prover::prove does with RistrettoPoint::multiscalar_mul for
 * A_I1 / A_O1 / S1 (reached from src/blindbid/proof.rs:88).  scalars: B * n_terms * 32 bytes, canonical (< l).
 * out32: B * 32 bytes, compressed results. */
int32_t bbp_msm_batch(bbp_ctx* ctx, uint32_t B, uint32_t n_terms, const uint8_t* scalars, uint32_t layout,
                      uint8_t* out32);

/* Device-resident variant used by bench.py so the timed region starts with inputs in HBM: same semantics with
 * `scalars_dev` / `out32_dev` being device pointers; `stream` is a hipStream_t (or BBP_STREAM_CONTEXT); does not
 * synchronise.  The device scalars cannot be screened on the host: they MUST be canonical (< l < 2^253) -- the recoding
 * only looks at bits 0..255 and silently drops a final carry, so a non-canonical scalar yields a wrong point (never a fault).
 * Scratch is grown inside the context on first use of a batch shape. */
int32_t bbp_msm_batch_dev(bbp_ctx* ctx, uint32_t B, uint32_t n_terms, const void* scalars_dev, uint32_t layout,
                          void* out32_dev, void* stream);

/* Witness helper: what the Go caller computes upstream of Proof::prove (defined by src/gadgets.rs:20-33,70-86):
 * m = mimc(k,0), x = mimc(d,m), y = mimc(seed,x), z_img = mimc(seed,m), y_inv = 1/y, q = d*y_inv.  Batched on
 * the device.  in: B * 96 bytes (d,k,seed); out: B * 192 bytes (m,x,y,y_inv,q,z_img). */
int32_t bbp_witness_batch(bbp_ctx* ctx, uint32_t B, const uint8_t* dks, uint8_t* out);

/* the caller-side pass on the device, feeding the batch prover / verifier directly (all pointers device
 * pointers, `stream` a hipStream_t, no synchronisation).  Per bid: bids_dev 96 B (d,k,seed as for bbp_witness_batch), lists_dev
 * N*32 B (the public bid list; entry `toggle` is overwritten with the bid's own x = mimc(d, mimc(k,0))), toggles_dev u64 (< N,
 * caller's responsibility).  Writes prove_in_dev rows in bbp_prove_batch_dev's input layout (7*32 + N*32 + 8 bytes) and, unless
 * NULL, verify_tail_dev rows score || z_img || seed || pub_list (96 + N*32 bytes) -- what follows the record in a
 * bbp_verify_batch row.  The next bbp_prove_batch_dev on this context waits for these rows by itself (the one exception to
 * "inputs must be complete at call time" below); anything else that reads them must be ordered after `stream` by the caller.
 * Give it a stream of its own when proving back to back: on the prover's stream it would queue behind the previous batch. */
int32_t bbp_prepare_bids_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* bids_dev, const void* lists_dev,
                             const void* toggles_dev, void* prove_in_dev, void* verify_tail_dev, void* stream);

/* Replaces Proof::prove (src/blindbid/proof.rs:36-46).
 * scalars7 = d,k,y,y_inv,q,z_img,seed; pub_list = N*32 bytes (Scalar::from_bits semantics, src/blindbid/bid.rs:27);
 * entropy = (4+N)*32 bytes of commitment blindings + 32 bytes rng seed (replaces thread_rng, proof.rs:53-64), or NULL
 * to draw from the OS.  proof_out record = R1CSProof bytes || 4*32 commitments || N*32 t_c;
 * *proof_len receives the R1CSProof byte count (1121). */
int32_t bbp_prove(bbp_ctx* ctx, const uint8_t scalars7[7 * 32], const uint8_t* pub_list, uint32_t N, uint64_t toggle,
                  const uint8_t* entropy, uint8_t* proof_out, uint32_t* proof_len);
uint32_t bbp_proof_record_size(uint32_t N); /* 1121 + 32*(4+N) */
uint32_t bbp_entropy_size(uint32_t N);      /* 32*(4+N) + 32 */

/* Replaces Verify::new(..).verify() (src/blindbid/verify.rs:27-89). record layout as produced by bbp_prove.
 * Concurrent callers (blocking or asynchronous, on a context or a pool) share device calls whatever their N and whichever of the
 * two R1CSProof layouts (compact, two-phase) their records have: callers that agree on both run bbp_verify_batch, any other
 * group runs one mixed-N call, and every caller receives the status of its own proof (bbp_set_verify_mixing, below). */
int32_t bbp_verify(bbp_ctx* ctx, const uint8_t* record, uint32_t record_len, const uint8_t score[32],
                   const uint8_t z_img[32], const uint8_t seed[32], const uint8_t* pub_list, uint32_t N);

/* Asynchronous forms of the two calls above, for hosts that cannot park a thread per request (an epoll server; a Rust Future --
 * the reference's ProveFuture / VerifyFuture, src/futures/prove.rs:21-26, verify.rs:21-26, can store its Waker in `user` and be
 * woken by `done`).  Same arguments, same screening, same combining into device batches (verify requests across bid-list lengths,
 * see bbp_verify).  Return value: BBP_OK = queued, and
 * `done(user, status)` will be called exactly once, on an engine thread, with the status bbp_prove / bbp_verify would have
 * returned; anything else = decided at once (bad arguments, a record that fails the structural parse), `done` is NOT called.
 * The inputs are copied before the call returns; proof_out must stay valid until `done` runs (it is written before).  Inside
 * the callback bbp_last_error(ctx) is the request's message.  `done` runs on a thread that every request of the next batch is
 * waiting for: hand the result over and return (no blocking, no engine calls on the same context from inside it). */
typedef void (*bbp_done_fn)(void* user, int32_t status);
int32_t bbp_prove_async(bbp_ctx* ctx, const uint8_t scalars7[7 * 32], const uint8_t* pub_list, uint32_t N, uint64_t toggle,
                        const uint8_t* entropy, uint8_t* proof_out, bbp_done_fn done, void* user);
int32_t bbp_verify_async(bbp_ctx* ctx, const uint8_t* record, uint32_t record_len, const uint8_t score[32], const uint8_t z_img[32],
                         const uint8_t seed[32], const uint8_t* pub_list, uint32_t N, bbp_done_fn done, void* user);

/* The data-parallel path: B independent proofs with a common list length N, fixed-stride records.
 * in:  B * (7*32 + N*32 + 8) bytes: scalars7 || pub_list || toggle(u64 LE)
 * entropy: B * bbp_entropy_size(N) or NULL.  out: B * bbp_proof_record_size(N).  status: B entries. */
int32_t bbp_prove_batch(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy,
                        uint8_t* out, int32_t* status);
/* in: B * (record_size(N) + 3*32 + N*32): record || score || z_img || seed || pub_list.  status: B entries
 * (BBP_OK / BBP_ERR_VERIFY / BBP_ERR_FORMAT). */
int32_t bbp_verify_batch(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, int32_t* status);

/* Device-resident variants (bench.py / pipelined callers): same record layouts, every pointer a device pointer,
 * `stream` a hipStream_t (or BBP_STREAM_CONTEXT), no host synchronisation, no host-side argument screening
 * (toggle < N and canonical inputs are the caller's responsibility).  in_dev / entropy_dev must be COMPLETE when the call
 * is made: the prover's opening stage (witness, commitments, transcript rng) starts at once on an internal stream so that
 * it overlaps the previous call's MSM stage; outputs are ordered on `stream` as usual: complete for anything enqueued on
 * `stream` after the call, and not written before everything enqueued on `stream` ahead of the call has finished.  entropy_dev: B * bbp_entropy_size(N) for prove,
 * B * 32 for verify (the verifier's TranscriptRng seed).  status_dev: B * int32.
 * Scheduling (results never depend on it): a prove call's MSM-heavy stage runs as three slices on three streams; calls below 1024
 * proofs, and calls of any size up to 4096 made while THREE OR MORE earlier prove calls are still in flight, run it unsliced on one
 * of three internal streams in rotation instead (whole calls overlap; higher throughput for a caller that queues ahead, at the
 * price of a longer time to each call's records: BBP_ROTATE_DEEP_FROM / BBP_ROTATE_DEEP_MAX). */
int32_t bbp_prove_batch_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev, void* out_dev,
                            void* stream);
int32_t bbp_verify_batch_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev, void* status_dev,
                             void* stream);

/* Aggregated verification -- SURVEY.md 8f-4, an extension: the reference verifies one proof per call (verify.rs:88) and has
 * no equivalent.  Proofs are checked in groups of `group` (0 = BBP_AGG_GROUP_DEFAULT) with ONE generator MSM per group: the
 * per-proof mega-checks are summed with random weights drawn from each proof's verifier TranscriptRng (seeded by the OS /
 * entropy_dev).  The members of every group that fails are then checked one by one (an MSM each over the scalars already
 * computed), so status[] is what bbp_verify_batch reports (a bad proof slipping through needs a ~2^-250 accident).  Same record layout as bbp_verify_batch.  *n_fallback (may be NULL)
 * receives how many proofs were checked individually.  The _dev variant is stream-ordered like bbp_verify_batch_dev -- which
 * groups failed is decided on the device, the per-proof pass sizes itself from a device counter -- unless n_fallback is non-NULL:
 * delivering that count synchronises `stream`.  The rows of entropy_dev must be distinct and unpredictable to whoever produced
 * the proofs (the _dev forms here and the mixed-N ones below): proofs that share a row share a weight, and forged proofs whose
 * residuals add up to the identity then pass their group's check.
 * Environment of the verify calls (BBP_VERIFY_AGGREGATE, BBP_VERIFY_OVERLAP, BBP_VARBASE_LANES, BBP_VARBASE_V1,
 * BBP_HOST_CHUNK_VERIFY): one list, with defaults, clamps and when each is read, in csrc/verify_plan.h (VerifyKnobs). */
#define BBP_AGG_GROUP_DEFAULT 32u
int32_t bbp_verify_batch_aggregated(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, int32_t* status, uint32_t group,
                                    uint32_t* n_fallback);
int32_t bbp_verify_batch_aggregated_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev,
                                        void* status_dev, uint32_t group, uint32_t* n_fallback, void* stream);

/* Mixed-N verification: one call verifies rows whose bid lists have different lengths (a node catching up verifies many rounds'
 * proofs, and the public list changes between rounds).  Ns: B host entries, read during the call only, in every form.  Rows are
 * packed back to back in request order; row i is record(Ns[i]) || score || z_img || seed || pub_list(Ns[i]), i.e.
 * bbp_proof_record_size(Ns[i]) + 96 + 32*Ns[i] bytes (bbp_verify_batch's row for that N).  status: B entries, each exactly what
 * bbp_verify_batch with that row's N reports (BBP_OK / BBP_ERR_VERIFY / BBP_ERR_FORMAT).  Ns is screened first: a 0 in any row
 * returns BBP_ERR_BAD_ARG, else an N above BBP_MAX_ITEMS in any row BBP_ERR_GENS_LEN, and nothing is verified; B == 0 returns
 * BBP_OK.  The aggregated forms keep bbp_verify_batch_aggregated's contract; groups are cut by index across any mix of N.  The
 * _dev forms are stream-ordered like bbp_verify_batch_dev (the aggregated one synchronises `stream` when n_fallback is non-NULL):
 * the library uploads Ns and derives the row offsets on `stream`.  One call makes the same number of launches whatever its mix of
 * N: one front end and one generator MSM (per group when aggregated).  A pool takes the host forms (rows split by index into
 * contiguous blocks) and refuses the _dev forms. */
int32_t bbp_verify_batch_mixed(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const uint8_t* in, int32_t* status);
int32_t bbp_verify_batch_mixed_aggregated(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const uint8_t* in, int32_t* status, uint32_t group,
                                          uint32_t* n_fallback);
int32_t bbp_verify_batch_mixed_dev(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const void* in_dev, const void* entropy_dev, void* status_dev,
                                   void* stream);
int32_t bbp_verify_batch_mixed_aggregated_dev(bbp_ctx* ctx, uint32_t B, const uint32_t* Ns, const void* in_dev, const void* entropy_dev,
                                              void* status_dev, uint32_t group, uint32_t* n_fallback, void* stream);

/* Rounds: proofs that share a seed and a bid list, sent once.  In the blind-bid protocol seed and bid list are public and belong to a
 * ROUND; only record, score and z_img belong to a proof (the reference sends both with every request because it verifies one proof per
 * call, src/blindbid/verify.rs:27-47, :100-117).  These calls take a table of R rounds and rows that name their round:
 *   round_Ns   R host entries, read during the call only, in every form
 *   rounds     packed back to back: round r is seed(32) || pub_list(32 * round_Ns[r]), 32 * (1 + round_Ns[r]) bytes; host memory in the
 *              host forms, device memory (rounds_dev) in the _dev forms
 *   round_of   B host entries below R, read during the call only; may be NULL when R == 1 (every row belongs to round 0)
 *   rows       packed back to back in request order: row i is record(N) || score || z_img, bbp_round_row_size(N) bytes, with
 *              N = round_Ns[round_of[i]]; compact records only, as in the mixed calls
 * status[i] is exactly what bbp_verify_batch_mixed reports for the expanded row record || score || z_img || seed_r || pub_list_r
 * (BBP_OK / BBP_ERR_VERIFY / BBP_ERR_FORMAT): a non-canonical seed in round r gives every row of round r BBP_ERR_FORMAT and leaves
 * the rows of other rounds alone; list items keep Scalar::from_bits semantics.  The table is reduced once per call on the device
 * (1 + N scalars per round instead of per proof) and a batch of one round uploads 7 777 instead of 14 273 bytes per proof at N = 202.
 * Screening, before anything is verified, the first failing check decides: a NULL among the required pointers BBP_ERR_BAD_ARG; B == 0
 * BBP_OK; R == 0 BBP_ERR_BAD_ARG; a 0 anywhere in round_Ns BBP_ERR_BAD_ARG, else an entry above BBP_MAX_ITEMS BBP_ERR_GENS_LEN;
 * round_of[i] >= R, or round_of == NULL with R > 1, BBP_ERR_BAD_ARG.  A round that no row names is allowed.
 * The aggregated forms keep bbp_verify_batch_aggregated's contract, groups cut by index across rounds; *n_fallback and the stream
 * ordering of the _dev forms are those of the mixed aggregated calls; entropy_dev holds B rows of 32 bytes under bbp_verify_batch_dev's
 * contract (distinct, unpredictable rows).  The _dev forms do no host screening of device data.  A pool takes the host forms (rows split
 * by index into contiguous blocks, every member receives the round table) and refuses the _dev forms. */
uint32_t bbp_round_row_size(uint32_t N); /* bbp_proof_record_size(N) + 64 */
int32_t bbp_verify_rounds(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                          const uint8_t* rows, int32_t* status);
int32_t bbp_verify_rounds_aggregated(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                                     const uint8_t* rows, int32_t* status, uint32_t group, uint32_t* n_fallback);
int32_t bbp_verify_rounds_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B, const uint32_t* round_of,
                              const void* rows_dev, const void* entropy_dev, void* status_dev, void* stream);
int32_t bbp_verify_rounds_aggregated_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B,
                                         const uint32_t* round_of, const void* rows_dev, const void* entropy_dev, void* status_dev, uint32_t group,
                                         uint32_t* n_fallback, void* stream);

/* Proving a round from raw bids: the prove side of the calls above.  What the reference's Go caller computes upstream of Proof::prove
 *  -- the witness of bbp_witness_batch and the bid's place in the public list -- happens on the device, and seed and bid
 * list travel once per call instead of once per proof (64 instead of 6 696 bytes per bid at N = 202).  One round per call:
 *   round      seed(32) || pub_list(32 N): the table layout of bbp_verify_rounds with R = 1
 *   bids       B rows of BBP_ROUND_BID_BYTES: d || k
 *   entropy    B * bbp_entropy_size(N) as for bbp_prove_batch, or NULL (bbp_set_entropy_source; the ChaCha row is the bid's index)
 *   rows_out   B * bbp_round_row_size(N): row i = record || score || z_img -- exactly the rows bbp_verify_rounds takes
 * Per bid, decided on the device in every form (status[i]; a refused bid's row, score, z_img and toggle are all zero):
 *   BBP_ERR_FORMAT    the seed is not canonical (every row: it is one of the seven scalars), or d or k is not
 *   BBP_ERR_BAD_ARG   no list item equals x = mimc(d, mimc(k, 0)) under Scalar::from_bits (an item stored as x + l, or with bit 255
 *                     set, matches): no witness exists -- the status bbp_prove_batch gives for toggle >= N
 *   BBP_OK            m, x, y, y_inv, q, z_img are byte for byte bbp_witness_batch's; toggle is the LOWEST matching index; record is
 *                     byte-equal to bbp_prove_batch's for the row d,k,y,y_inv,q,z_img,seed || pub_list || toggle under the same entropy
 *                     row (the list bytes raw from the table); score = q
 * Screening, before anything runs, the first failing check decides: a NULL required pointer BBP_ERR_BAD_ARG; N == 0 BBP_ERR_BAD_ARG,
 * N > BBP_MAX_ITEMS BBP_ERR_GENS_LEN; B == 0 BBP_OK.
 * bbp_prove_round honours the context's settings as bbp_prove_batch does on the expanded rows: entropy source, BBP_HOST_CHUNK_PROVE,
 * checked proving (a failed record is proved once more from its bid, same entropy; a second failure raises health bit 1), the health
 * word read back with the results, bbp_reserve (a reserved context allocates nothing in a round call).  A pool takes it (bids split by
 * index into contiguous blocks, every member receives the table, results in request order) and refuses the two _dev forms.
 * The _dev forms do no host screening of device data and no synchronisation; outputs are ordered on `stream`.
 *   bbp_prepare_round_dev   the device pass alone.  Writes prove_in_dev rows in bbp_prove_batch_dev's input layout (a refused bid: the
 *                           all-zero stand-in, so a batch keeps its geometry), tails_dev rows score || z_img (64 bytes; may be NULL),
 *                           toggles_dev u64 (may be NULL), status_dev int32.  The next prove call on the context waits for these rows
 *                           by itself, like bbp_prepare_bids_dev's (the same event).
 *   bbp_prove_round_dev     that pass, bbp_prove_batch_dev, row assembly and statuses on the caller's stream; the prover's opening
 *                           stage waits for the pass through the event, not for the caller's stream. */
#define BBP_ROUND_BID_BYTES 64u /* d || k */
int32_t bbp_prepare_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, void* prove_in_dev,
                              void* tails_dev, void* toggles_dev, void* status_dev, void* stream);
int32_t bbp_prove_round(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* bids, const uint8_t* entropy,
                        uint8_t* rows_out, uint64_t* toggles_out, int32_t* status);
int32_t bbp_prove_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, const void* entropy_dev,
                            void* rows_out_dev, void* toggles_out_dev, void* status_dev, void* stream);

/* Selecting a round's bids: a round ends with "the proof with the highest score wins", so a holder of many bids wants proofs for the few
 * that can still win -- the K highest scores, none below the best score already seen.  These calls score every bid on the device (three
 * MiMC chains and one inversion per bid; 40 bytes written per bid instead of an expanded row), select, and prove only the selected bids.
 * For round (seed, pub_list), bids 0..B-1 (B <= BBP_SELECT_MAX_BIDS), floor32 and K:
 *   floor32      32 bytes, an unsigned 256-bit little-endian integer; any value
 *   status[i]    exactly what bbp_prove_round reports for bid i (BBP_ERR_FORMAT, BBP_ERR_BAD_ARG, BBP_OK; the same order of checks)
 *   score[i]     q = d * y^-1 mod l as the canonical integer in [0, l) for an accepted bid (score_gadget, src/gadgets.rs:70-86), zero for a
 *                refused one; scores are ordered as integers, the only order the 32-byte score field of a record admits
 *   Q            { i : status[i] == BBP_OK and score[i] >= floor }: floor 0 admits every accepted bid, a floor >= l none; "strictly
 *                better than the best seen" is best + 1
 *   Sel          Q when K == 0 or |Q| <= K, else the K members of Q that come first under (score descending, index ascending) -- equal
 *                scores happen: the same (d, k) twice
 *   sel          Sel in ASCENDING INDEX order; n_sel = |Sel|, n_qualified = |Q|
 * Proving is bbp_prove_round over bids[sel[0]], bids[sel[1]], ...: entropy row j goes to sel[j] (the row follows the rank in sel, not
 * the bid's index -- a caller cannot know the indices in advance), and under entropy source DEVICE or HEDGED the row index of sel[j] is j.
 *
 * bbp_prove_round_select, the host form, runs in two phases.  A: table and bids are uploaded, scored and selected; counts, sel, statuses
 * and (scores_out != NULL) scores come back -- the call's one synchronisation.  Phase A calls of one context are serialised among
 * themselves; their device scratch and pinned mirror grow on demand: bbp_reserve does NOT size them (it sizes everything phase B uses).
 * B: the selected bids are gathered from the caller's `bids` on the host (no secret travels back from the device) and proved by
 * bbp_prove_round's own path, so entropy source, BBP_HOST_CHUNK_PROVE, checked proving, hedged row keys, secret wiping and bbp_reserve
 * hold as they do there and rows_out is byte-equal to bbp_prove_round's on the gathered bids.  A bid that scoring accepted and proving
 * refuses is BBP_ERR_INTERNAL.
 *   entropy      cap * bbp_entropy_size(N), row j for sel[j]; or NULL (bbp_set_entropy_source)
 *   rows_out     cap * bbp_round_row_size(N); sel_out cap entries; toggles_out cap entries or NULL: rows j < n_sel are written
 *   scores_out   B * 32 or NULL; status B entries; n_qualified may be NULL
 * Screening, before anything runs, the first failing check decides: a NULL required pointer BBP_ERR_BAD_ARG (rows_out and sel_out may
 * be NULL only when cap == 0); N == 0 BBP_ERR_BAD_ARG, N > BBP_MAX_ITEMS BBP_ERR_GENS_LEN; B > BBP_SELECT_MAX_BIDS BBP_ERR_BAD_ARG;
 * B == 0 BBP_OK with n_sel = 0.  After phase A: n_sel > cap is BBP_ERR_BAD_ARG (bbp_last_error names both numbers) -- status, scores_out,
 * n_sel and n_qualified are written, sel_out and rows_out are untouched, nothing is proved; with K > 0 and cap >= K it cannot happen.
 * n_sel == 0 is BBP_OK and no prove call is made.  Scoring alone is the call with the all-ones floor and cap = 0.
 * A pool takes it: phase A is served by member 0 (as bbp_witness_batch), phase B is bbp_prove_round on the pool.
 * Secret wiping: the phase-A buffers are SECRET and erased before the call returns.
 *
 * bbp_select_round_dev, the device form: stream-ordered, no synchronisation, no host screening of device data; a pool refuses it.
 * Scoring, selection, then -- when cap > 0 and any of prove_in_dev, tails_dev, toggles_dev is given -- the selected bids gathered and
 * taken through bbp_prepare_round_dev's own kernels, sized by cap (lanes at or beyond the device-side count leave at once).
 *   sel_dev      cap x u32: the first min(n_sel, cap) entries of sel, in index order
 *   counts_dev   2 x u32: n_sel, n_qualified -- the true values also when n_sel > cap
 *   status_dev   B x int32; scores_dev B x 32 or NULL
 *   prove_in_dev, tails_dev (64 bytes: score || z_img), toggles_dev (u64): each cap rows or NULL; row j < min(n_sel, cap) is byte for
 *                byte what bbp_prepare_round_dev writes for bid sel[j], rows at or beyond that are not written
 * The rows are announced as bbp_prepare_round_dev's are (the same event): the next prove call on the context waits for them by itself.
 * A caller reads counts, calls bbp_prove_batch_dev(min(n_sel, cap), ...) and joins records and tails itself.  NULL is BBP_ERR_BAD_ARG for
 * round_dev, bids_dev, floor32, counts_dev, status_dev, and for sel_dev when cap > 0; then N, then B as above; B == 0 writes zero counts.
 *
 * bbp_debug_round_select, test hook: the shipped selection kernel on caller-made host arrays -- scores B x 32 (each below l), statuses B
 * (each one of the three) -- with a floor, K and cap; sel_out receives min(n_sel, cap) entries.  Synchronises.  BBP_ERR_BAD_ARG, nothing
 * launched: a NULL pointer, B == 0 or above BBP_SELECT_MAX_BIDS, a score >= l, a status outside the three.  A pool refuses it. */
#define BBP_SELECT_MAX_BIDS (1u << 20)
int32_t bbp_select_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, const uint8_t floor32[32], uint32_t K,
                             uint32_t cap, void* sel_dev, void* counts_dev, void* status_dev, void* scores_dev, void* prove_in_dev, void* tails_dev,
                             void* toggles_dev, void* stream);
int32_t bbp_prove_round_select(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* bids, const uint8_t floor32[32], uint32_t K,
                               uint32_t cap, const uint8_t* entropy, uint8_t* rows_out, uint32_t* sel_out, uint32_t* n_sel, uint32_t* n_qualified,
                               uint64_t* toggles_out, uint8_t* scores_out, int32_t* status);
int32_t bbp_debug_round_select(bbp_ctx* ctx, uint32_t B, const uint8_t* scores, const int32_t* statuses, const uint8_t floor32[32], uint32_t K,
                               uint32_t cap, uint32_t* sel_out, uint32_t* n_sel, uint32_t* n_qualified);

/* Best valid proofs of a round: the verify side of "the proof with the highest score wins".  A node that has collected B candidate
 * proofs of one round wants the best valid one, or the K best.  The score is a public input of the circuit, so a valid proof cannot
 * claim a score it did not earn and a forged high score costs the verifier one failed check: these calls order the rows by CLAIMED
 * score, verify from the top in tranches that double, and stop at the K-th proof that holds -- one small tranche for honest traffic,
 * at most all B verifications for a flood of forged high scores.
 * Inputs: one round seed || pub_list (N items) and B rows record || score || z_img -- bbp_verify_rounds' layout with R = 1, compact
 * records, bbp_round_row_size(N) bytes each, packed back to back (B <= BBP_SELECT_MAX_BIDS) -- and floor32, K, tranche.
 *   key[i]        the 32 score bytes of row i as an unsigned 256-bit little-endian integer: the field the verifier reads
 *   screening     in this order: key[i] >= l: status[i] = BBP_ERR_FORMAT, the row is never verified (what bbp_verify_rounds reports for
 *                 a non-canonical score whatever else the row holds); key[i] < floor: status[i] = BBP_ROW_SKIPPED ("the call did not
 *                 have to verify this row"; not a bbp_status); any other row is a candidate, n_candidates counts them
 *   order         candidates by key descending, then index ascending (byte-equal rows do occur)
 *   tranches      T_0 = max(tranche, K), tranche == 0 meaning BBP_BEST_TRANCHE_DEFAULT; with K == 0, T_0 = n_candidates (one tranche,
 *                 every candidate is examined); T_t = T_0 * 2^t.  Tranche t is the next min(T_t, remaining) candidates in that order;
 *                 every row of it is verified, and its status[i] is exactly what bbp_verify_rounds reports for that row in that round
 *                 (BBP_OK / BBP_ERR_VERIFY / BBP_ERR_FORMAT)
 *   stopping      at the end of the first tranche after which at least K rows have verified OK (K > 0), or when no candidate is left;
 *                 candidates never reached keep BBP_ROW_SKIPPED; n_examined counts the verified rows
 *   best          the OK rows in candidate order, the first K of them (all when K == 0), in rank order: best[0] is the winner.
 *                 n_best is its true length, best_out receives min(n_best, cap) entries (entries beyond are not written)
 * Which rows are examined depends only on the inputs and `tranche`, never on timing.  At most n_candidates rows are verified, in at
 * most ceil(log2(n_candidates / T_0 + 1)) tranches.
 * Screening of the arguments, before anything runs, the first failing check decides: a NULL required pointer BBP_ERR_BAD_ARG (best_out
 * may be NULL only when cap == 0); N == 0 BBP_ERR_BAD_ARG; N > BBP_MAX_ITEMS BBP_ERR_GENS_LEN; B > BBP_SELECT_MAX_BIDS BBP_ERR_BAD_ARG;
 * B == 0 BBP_OK with all counts zero.
 *
 * bbp_verify_round_best, the host form (a context or a pool): only the 32 key bytes of every row go up (gathered into a pinned staging
 * area); keys, selection and the examined marks live on one device -- the context, or member 0 of a pool.  Per tranche the selected
 * indices come down, the tranche's rows are gathered from the caller's memory and verified through bbp_verify_rounds_aggregated's own
 * path (so the pool split, BBP_HOST_CHUNK_VERIFY, the entropy source, verify mixing and the health word hold as they do there), and its
 * statuses go back up to mark the rows.  A row that is not examined never crosses PCIe.  Calls on one context are serialised among
 * themselves; their device state and pinned mirror grow on demand: bbp_reserve does NOT size them.
 *
 * bbp_verify_round_best_dev, rows resident in device memory; a pool refuses it.  rows_dev may have any alignment; entropy_dev holds
 * B x 32 bytes, row i for row i under bbp_verify_batch_dev's contract (distinct, unpredictable rows), gathered with its row; a tranche
 * runs through bbp_verify_rounds_aggregated_dev's path on the gathered rows, in engine calls of at most BBP_HOST_CHUNK_VERIFY rows as a
 * host-pointer call's are (which also bounds the gathered copy).  The call SYNCHRONISES `stream`: once after the first
 * selection (the candidate count), once per tranche to read two counters (rows examined, rows OK), and once to deliver the results.
 * The host outputs are valid on return; status_dev (B x int32) is complete on `stream`.  No host screening of device data.
 *
 * bbp_debug_round_best, test hook (synchronises; a pool refuses it): the shipped key, selection, mark and ranking kernels on caller-made
 * host arrays -- keys B x 32 bytes, verdicts B x int32, each BBP_OK, BBP_ERR_VERIFY or BBP_ERR_FORMAT: what verification would say of
 * that row.  Nothing is verified: a tranche's statuses are read from verdicts.  BBP_ERR_BAD_ARG, nothing launched: a NULL pointer, B == 0
 * or above BBP_SELECT_MAX_BIDS, a verdict outside the three. */
#define BBP_ROW_SKIPPED (-1)
#define BBP_BEST_TRANCHE_DEFAULT 16u
int32_t bbp_verify_round_best(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* rows, const uint8_t floor32[32], uint32_t K,
                              uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                              int32_t* status);
int32_t bbp_verify_round_best_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* rows_dev, const void* entropy_dev,
                                  const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                  uint32_t* n_candidates, uint32_t* n_examined, void* status_dev, void* stream);
int32_t bbp_debug_round_best(bbp_ctx* ctx, uint32_t B, const uint8_t* keys, const int32_t* verdicts, const uint8_t floor32[32], uint32_t K,
                             uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined,
                             int32_t* status);

/* Best proofs of a round, one per bidder.  z_img = mimc(seed, mimc(k, 0)) is the only per-bidder value a verifier sees: two valid rows
 * of one round with equal z_img come from the same secret k.  The calls above treat every row as a bidder of its own, so with K > 1 a
 * proof that was sent twice -- the same bytes, or the same bid proved again under fresh blindings -- takes two places and hides the real
 * runners-up.  These calls return at most one row per z_img, and rows of an identity that already has a verified row leave the
 * candidate set without being uploaded or verified.
 * Inputs as bbp_verify_round_best, plus id[i]: the 32 raw z_img bytes of row i.  Identities are compared as BYTES; that is exact for
 * every row that can win, because a row whose z_img is not canonical gets BBP_ERR_FORMAT from the verifier and never BBP_OK.
 *   key, screening, order, n_candidates, T_0, T_t    as bbp_verify_round_best
 *   settled       an identity is settled once a row carrying it has verified BBP_OK; its holder is the first such row in candidate order
 *   tranches      tranche t is the next min(T_t, live) LIVE candidates in order; every one is verified and its status[i] is exactly what
 *                 bbp_verify_rounds reports.  Rows of one identity inside one tranche are all verified and keep their true status; only
 *                 the first OK one in candidate order becomes holder
 *   stopping      after the first tranche that leaves at least K identities settled (K > 0), or when no live candidate is left
 *   duplicates    otherwise, before the next tranche, every live candidate whose id is settled gets BBP_ROW_DUPLICATE ("could not have
 *                 entered the result; not verified"; not a bbp_status) and leaves the candidate set; n_duplicates counts these rows.
 *                 Once the call has stopped, rows never reached keep BBP_ROW_SKIPPED: no drop pass runs after the last tranche.  A
 *                 forged row that borrows a victim's z_img under a higher claimed score fails verification and settles nothing: the
 *                 victim's row stays live
 *   best          the holders in candidate order, the first K of them (all when K == 0); n_best is the true length, best_out receives
 *                 min(n_best, cap) entries
 * n_examined + n_duplicates <= n_candidates; the bound on the tranches of bbp_verify_round_best holds; which rows are examined depends
 * only on the inputs and `tranche`, never on timing.
 * Argument screening and its order, the pool (the host form is accepted: state on member 0, tranches verified by the pool; the _dev form
 * and the hook are refused), the serialisation of calls on one context, the synchronisation points of the _dev form (one more per
 * tranche in the host form: the count of settled identities decides whether another tranche runs) and "bbp_reserve does not size the
 * state" are those of the three calls above.  n_duplicates is a required pointer.
 * The host form uploads 64 bytes per row, score || z_img (adjacent in a row: one gather per row); a tranche's rows come from the
 * caller's memory exactly as above, and a duplicate row never crosses PCIe.  The _dev form reads both fields byte by byte at any
 * alignment.
 * bbp_debug_round_best_distinct, test hook: as bbp_debug_round_best, plus ids (B x 32 bytes, any values) and table_log2: 0 for the call's
 * own sizing of the identity table (the least 2^s >= 2 B slots), or an explicit size of 2^table_log2 slots.  BBP_ERR_BAD_ARG, nothing
 * launched, also when table_log2 > 21, or when table_log2 > 0 and 2^table_log2 is not greater than the number of BBP_OK verdicts. */
#define BBP_ROW_DUPLICATE (-2)
int32_t bbp_verify_round_best_distinct(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* rows, const uint8_t floor32[32],
                                       uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates,
                                       uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status);
int32_t bbp_verify_round_best_distinct_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* rows_dev, const void* entropy_dev,
                                           const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                                           uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, void* status_dev, void* stream);
int32_t bbp_debug_round_best_distinct(bbp_ctx* ctx, uint32_t B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts,
                                      const uint8_t floor32[32], uint32_t K, uint32_t tranche, uint32_t cap, uint32_t table_log2, uint32_t* best_out,
                                      uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status);

/* Best valid proofs of many rounds: bbp_verify_round_best for every round of a bbp_verify_rounds call at once.  A node that is catching
 * up holds B candidate rows spread over R rounds and wants the winner, or the K best, of every round.  round_Ns, rounds, round_of and
 * rows are exactly bbp_verify_rounds' arguments: rows packed back to back in request order, row i of bbp_round_row_size(round_Ns[
 * round_of[i]]) bytes, any mix of sizes; R <= BBP_BEST_MAX_ROUNDS, B <= BBP_SELECT_MAX_BIDS.  floors: R x 32 bytes, one floor32 per
 * round, or NULL for all zero.
 * The rule: let I_r be the rows with round_of[i] == r in ascending index.  The outputs for round r -- status[i] for i in I_r, n_best[r],
 * n_candidates[r], n_examined[r] and best_out[r * cap ..], which receives min(n_best[r], cap) entries (entries beyond are not written) --
 * are exactly what bbp_verify_round_best reports for the rows of I_r, round r of the table, floor floors[r] and the call's K, tranche
 * and cap, with local row indices mapped back to indices into the call's rows (ascending global index is ascending local index: ties
 * break the same way).  A round that no row names reports zeros.
 *   steps         at step t = 0, 1, ... every round that has not stopped under the single-round stopping rule contributes its tranche
 *                 t; with K == 0 there is one step, and it holds every candidate of every round.  All the rows of a step are verified
 *                 together, and every one gets exactly the status bbp_verify_rounds reports for it.  A round that has stopped
 *                 contributes nothing to later steps.  n_steps (may be NULL) is the number of steps that held at least one row: the
 *                 maximum, over the rounds, of the tranches each round ran.
 * Which rows are examined depends only on the inputs and `tranche`, never on timing.
 * Screening of the arguments, before anything runs, the first failing check decides: a NULL required pointer BBP_ERR_BAD_ARG (best_out may
 * be NULL only when cap == 0; floors and n_steps may be NULL); R == 0 or R > BBP_BEST_MAX_ROUNDS BBP_ERR_BAD_ARG; a 0 in round_Ns
 * BBP_ERR_BAD_ARG, otherwise an entry above BBP_MAX_ITEMS BBP_ERR_GENS_LEN; B > BBP_SELECT_MAX_BIDS BBP_ERR_BAD_ARG; B == 0 BBP_OK with
 * every count of every round zero; round_of == NULL with R > 1, or round_of[i] >= R, BBP_ERR_BAD_ARG.
 * With R == 1 every form runs the single-round call above it (one large round is what that call's many-workgroup selection is for) and
 * reports its tranches as n_steps.  With R > 1 a round is selected by ONE workgroup, in time linear in the round's candidates per
 * pass: the intended shape is many rounds of modest size.
 *
 * bbp_verify_rounds_best, the host form (a context or a pool): only the 32 score bytes of every row go up, with round_of and the floors;
 * keys, segments, selection and marks live on one device -- the context, or member 0 of a pool.  Per step the selected indices come down
 * grouped by round in ascending round order, the rows are gathered from the caller's memory and verified in one rounds call through
 * bbp_verify_rounds_aggregated's own path (so the pool split, BBP_HOST_CHUNK_VERIFY, the entropy source, verify mixing and the health
 * word hold as they do there; the whole round table travels with every step), and the statuses go back up to mark the rows.  A row that
 * is never examined never crosses PCIe.  Serialised with the other best calls of the context; bbp_reserve does NOT size the state.
 *
 * bbp_verify_rounds_best_dev, table, rows and entropy resident in device memory; a pool refuses it.  rows_dev may have any alignment;
 * entropy_dev holds B x 32 bytes, row i for row i, gathered with its row.  round_Ns, round_of and floors are host arrays.  The host
 * computes the byte offset of every row once and uploads them; a step's rows, of mixed sizes, are packed on the device and verified
 * through bbp_verify_rounds_aggregated_dev's path in engine calls of at most BBP_HOST_CHUNK_VERIFY rows.  The call SYNCHRONISES `stream`:
 * once after the keys are segmented (the per-round candidate counts), once per step (the per-round rows of the next step), and once to
 * deliver.  The host outputs are valid on return; status_dev (B x int32) is complete on `stream`.  No host screening of device data.
 *
 * bbp_debug_rounds_best, test hook (synchronises; a pool refuses it): the shipped kernels on caller-made keys (B x 32 bytes) and
 * verdicts (B x int32, each BBP_OK, BBP_ERR_VERIFY or BBP_ERR_FORMAT); nothing is verified.  BBP_ERR_BAD_ARG, nothing launched, also for
 * B == 0 and for a verdict outside the three. */
#define BBP_BEST_MAX_ROUNDS (1u << 16)
int32_t bbp_verify_rounds_best(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                               const uint8_t* rows, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best,
                               uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_steps, int32_t* status);
int32_t bbp_verify_rounds_best_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B, const uint32_t* round_of,
                                   const void* rows_dev, const void* entropy_dev, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap,
                                   uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_steps, void* status_dev,
                                   void* stream);
int32_t bbp_debug_rounds_best(bbp_ctx* ctx, uint32_t R, uint32_t B, const uint32_t* round_of, const uint8_t* keys, const int32_t* verdicts,
                              const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates,
                              uint32_t* n_examined, uint32_t* n_steps, int32_t* status);

/* Best proofs of many rounds, one per bidder: bbp_verify_round_best_distinct for every round of a bbp_verify_rounds call at once.  A node
 * that gathers gossip from several peers holds resent proofs as a matter of course; with K > 1 bbp_verify_rounds_best lets the copies
 * take the places of the real runners-up, and bbp_verify_round_best_distinct repairs that for one round per call only.  Inputs as
 * bbp_verify_rounds_best; id[i] is the 32 raw z_img bytes of row i, as for bbp_verify_round_best_distinct.
 * The rule: let I_r be the rows with round_of[i] == r in ascending index.  The outputs for round r -- status[i] for i in I_r, n_best[r],
 * n_candidates[r], n_examined[r], n_duplicates[r] and best_out[r * cap ..], which receives min(n_best[r], cap) entries (entries beyond are
 * not written) -- are exactly what bbp_verify_round_best_distinct reports for the rows of I_r, round r of the table, floor floors[r] and
 * the call's K, tranche and cap, with local row indices mapped back to indices into the call's rows.  A round that no row names reports
 * zeros.
 *   identities    belong to a round: the same 32 z_img bytes in two rounds are two identities (z_img depends on the seed; and a table may
 *                 list two rounds with equal seeds: still two rounds)
 *   steps         step t holds tranche t of every round that has not stopped under the single-round one-per-bidder rule: K identities
 *                 settled in it, or no live candidate left.  All the rows of a step are verified in one engine call, and every one gets
 *                 exactly the status bbp_verify_rounds reports for it
 *   drop pass     before round r's next tranche, live candidates of r whose identity is settled in r leave with BBP_ROW_DUPLICATE.  A
 *                 round that has stopped runs no drop pass: its unreached rows keep BBP_ROW_SKIPPED even when their identity is settled,
 *                 and even while other rounds go on for more steps
 *   n_steps       (may be NULL) the largest number of tranches any round ran; under drops it is counted, not derived from n_examined
 * n_examined[r] + n_duplicates[r] <= n_candidates[r].  Which rows are examined depends only on the inputs and `tranche`, never on timing.
 * n_duplicates (R entries) is a required pointer; floors and n_steps may be NULL; screening of the arguments and its order are exactly
 * bbp_verify_rounds_best's.  With R == 1 every form runs the single-round one-per-bidder call and reports its tranches as n_steps.
 *
 * bbp_verify_rounds_best_distinct, the host form (a context or a pool): 64 bytes of every row go up, score || z_img, with round_of and
 * the floors; keys, identities, segments, selection, marks and drops live on one device -- the context, or member 0 of a pool.  The
 * device plans every step from its own counters (the host knows the verdicts, not the identities): one submission per step carries the
 * statuses of the step before up and brings the next step's rows down, which are gathered from the caller's memory and verified through
 * bbp_verify_rounds_aggregated's own path, as for bbp_verify_rounds_best.  A row that is never examined and a duplicate row never cross
 * PCIe.  Serialised with the other best calls of the context; bbp_reserve does NOT size the state.
 *
 * bbp_verify_rounds_best_distinct_dev: as bbp_verify_rounds_best_dev, the same synchronisation points; z_img is read byte by byte at any
 * alignment.  status_dev is complete on `stream`.  No host screening of device data.  A pool refuses it.
 *
 * bbp_debug_rounds_best_distinct, test hook (synchronises; a pool refuses it): as bbp_debug_rounds_best, plus ids (B x 32 bytes, any
 * values) and table_log2 under the rules of bbp_debug_round_best_distinct: 0 for the call's own sizing of the ONE identity table of the
 * call (the least 2^s >= 2 B slots), or 2^table_log2 slots.  BBP_ERR_BAD_ARG, nothing launched, also when table_log2 > 21, or when
 * table_log2 > 0 and 2^table_log2 is not greater than the number of BBP_OK verdicts. */
int32_t bbp_verify_rounds_best_distinct(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                                        const uint8_t* rows, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t* best_out,
                                        uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, uint32_t* n_steps,
                                        int32_t* status);
int32_t bbp_verify_rounds_best_distinct_dev(bbp_ctx* ctx, uint32_t R, const uint32_t* round_Ns, const void* rounds_dev, uint32_t B,
                                            const uint32_t* round_of, const void* rows_dev, const void* entropy_dev, const uint8_t* floors, uint32_t K,
                                            uint32_t tranche, uint32_t cap, uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates,
                                            uint32_t* n_examined, uint32_t* n_duplicates, uint32_t* n_steps, void* status_dev, void* stream);
int32_t bbp_debug_rounds_best_distinct(bbp_ctx* ctx, uint32_t R, uint32_t B, const uint32_t* round_of, const uint8_t* keys, const uint8_t* ids,
                                       const int32_t* verdicts, const uint8_t* floors, uint32_t K, uint32_t tranche, uint32_t cap, uint32_t table_log2,
                                       uint32_t* best_out, uint32_t* n_best, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates,
                                       uint32_t* n_steps, int32_t* status);

/* Standing of a round: the K best valid rows of a round SO FAR, one per z_img, kept on the device while candidates arrive.  The calls
 * above are one-shot: the caller holds all B rows of a round and hands them over together.  A node receives a round by gossip, in
 * bursts, from several peers, with resends; re-running bbp_verify_round_best_distinct over everything received verifies examined rows
 * again, and calling it on a burst alone loses the identity table between calls.  A standing is the state that outlives a call.
 * It belongs to one round (seed || pub_list, N items; copied by bbp_standing_open, the caller's buffer is free on return), one floor32
 * and one K in 1..BBP_STANDING_MAX_K (K == 0, "every valid row", is refused: nothing would ever leave).
 *   entries       at most K of (key, z_img, serial); key as bbp_verify_round_best's; serial (u64) is the number of rows offered to this
 *                 standing before that row: row j of an offer has serial offered + j.  Kept in RANK ORDER: key descending, then serial
 *                 ascending.  bar is the key of entry K-1 once the standing is full; it never falls
 * An offer of B rows (bbp_verify_round_best's row layout: record || score || z_img, bbp_round_row_size(N) bytes each):
 *   screening     in this order: key >= l BBP_ERR_FORMAT, never verified; key < floor BBP_ROW_SKIPPED; the standing is full and (key,
 *                 serial) does not come before entry K-1 in rank order BBP_ROW_SKIPPED (at the start of an offer: key <= bar); every
 *                 other row is a candidate, n_candidates counts them
 *   leave pass    before tranche 0 and after every tranche, over the live candidates: a row that no longer passes the third screening
 *                 test leaves, its status stays BBP_ROW_SKIPPED; otherwise a row whose z_img is held by an entry that comes BEFORE it in
 *                 rank order leaves with BBP_ROW_DUPLICATE, n_duplicates counts these.  A row whose identity is held with a LOWER key stays
 *                 live: a bidder may improve
 *   tranches      T_0 = max(tranche, K) (tranche == 0: BBP_BEST_TRANCHE_DEFAULT), T_t = T_0 2^t; tranche t is the next min(T_t, live)
 *                 live candidates in candidate order (key descending, index ascending); every one is verified, its status is exactly
 *                 what bbp_verify_rounds reports, n_examined counts them
 *   merge         after each tranche every BBP_OK row enters; one whose identity is already held replaces that entry only if it comes
 *                 before it in rank order; the standing is cut to its first K entries, and what falls out is forgotten
 *   stop          when no live candidate is left
 *   entered       the offer's rows that are entries after it, offer-local indices in rank order; n_entered is the true length,
 *                 entered_out receives min(n_entered, cap) of them, entries beyond are not written.  The standing keeps no row bytes: the
 *                 caller keeps the rows that entered_out names
 *   failure       an offer that fails with BBP_ERR_DEVICE or BBP_ERR_INTERNAL leaves the standing and its offered count exactly as they
 *                 were: the call works on a copy in its own scratch and commits once, at the end
 * What follows: an offer to a fresh standing reports what bbp_verify_round_best_distinct reports for the same rows, floor, K and tranche
 * (status, n_candidates, n_examined, n_duplicates, entered == best).  After any sequence of offers the entries are the first K, in rank
 * order, of: per z_img the first BBP_OK row at or above the floor in rank order, over ALL rows offered so far -- whatever the cuts
 * between bursts and whatever `tranche`.  A valid row that is offered again is never verified again (BBP_ROW_SKIPPED or
 * BBP_ROW_DUPLICATE) and is not uploaded.  A forged row with a high claimed score costs one failed check each time it is sent: rejected
 * rows are not remembered.  n_examined + n_duplicates <= n_candidates; which rows are examined depends only on the inputs, never on timing.
 *
 * bbp_standing_open: screening, the first failing check decides: a NULL pointer BBP_ERR_BAD_ARG; N == 0 BBP_ERR_BAD_ARG; N > BBP_MAX_ITEMS
 * BBP_ERR_GENS_LEN; K == 0 or K > BBP_STANDING_MAX_K BBP_ERR_BAD_ARG; BBP_STANDING_MAX_OPEN standings already open on the handle
 * BBP_ERR_BAD_ARG.  *standing is the handle of the new standing.  Its state is a device allocation of its OWN (a header -- count, bar,
 * offered -- and K x (8 + 8 + 2) words; on a pool: on member 0), not part of the scratch the best calls share: other best calls, and
 * offers to other standings, may run between two offers.  bbp_reserve does not size it.
 * bbp_standing_offer, the host form (a context or a pool): screening: an unknown or closed handle BBP_ERR_BAD_ARG; a NULL pointer
 * BBP_ERR_BAD_ARG (entered_out may be NULL only when cap == 0); B > BBP_SELECT_MAX_BIDS BBP_ERR_BAD_ARG; B == 0 BBP_OK with zero counts
 * and the standing unchanged.  64 bytes per row go up, score || z_img; a tranche's rows are gathered from the caller's memory and
 * verified through bbp_verify_rounds_aggregated's own path exactly as bbp_verify_round_best_distinct does it (entropy source,
 * BBP_HOST_CHUNK_VERIFY, the health word, verify mixing and the pool split hold as they do there); one more wait than that call: the
 * commit.  Serialised with the other best calls of the context.
 * bbp_standing_read: the entries in rank order: serials_out (u64 each), scores_out and z_imgs_out (32 bytes each) receive min(count,
 * cap) entries; any output except n_entries may be NULL; n_entries is the true count, n_offered the rows offered so far.
 * bbp_standing_close: closes the standing and frees its state; the handle may be handed out again.  bbp_free closes what is still open.
 * bbp_debug_standing_offer, test hook (synchronises; a pool refuses it): an offer of made-up keys, ids (B x 32 bytes each) and verdicts
 * (B x int32) through the shipped kernels against a real standing's state; nothing is verified.  Screening as the offer's (B == 0 is
 * BBP_OK with zero counts); beyond that it refuses what bbp_debug_round_best_distinct refuses: a verdict outside the three.
 * bbp_debug_standing_trip, test hook: the next offer to the standing raises the offer's internal flag word on the device behind its
 * after-th merge (after >= 1) and so ends with BBP_ERR_INTERNAL, as an offer whose bounded loops ran out does; no device fault is involved.
 * Out of scope: a _dev form of the offer; a server opcode; keeping the winning rows' bytes; a
 * memory of rejected rows; a round table resident across offers (the round travels with every tranche, as in the one-shot calls). */
#define BBP_STANDING_MAX_K 1024u
#define BBP_STANDING_MAX_OPEN 64u
int32_t bbp_standing_open(bbp_ctx* ctx, uint32_t N, const uint8_t* round, const uint8_t floor32[32], uint32_t K, uint32_t* standing);
int32_t bbp_standing_offer(bbp_ctx* ctx, uint32_t standing, uint32_t B, const uint8_t* rows, uint32_t tranche, uint32_t cap, uint32_t* entered_out,
                           uint32_t* n_entered, uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status);
int32_t bbp_standing_read(bbp_ctx* ctx, uint32_t standing, uint32_t cap, uint64_t* serials_out, uint8_t* scores_out, uint8_t* z_imgs_out,
                          uint32_t* n_entries, uint64_t* n_offered);
int32_t bbp_standing_close(bbp_ctx* ctx, uint32_t standing);
int32_t bbp_debug_standing_offer(bbp_ctx* ctx, uint32_t standing, uint32_t B, const uint8_t* keys, const uint8_t* ids, const int32_t* verdicts,
                                 uint32_t tranche, uint32_t cap, uint32_t* entered_out, uint32_t* n_entered, uint32_t* n_candidates,
                                 uint32_t* n_examined, uint32_t* n_duplicates, int32_t* status);
int32_t bbp_debug_standing_trip(bbp_ctx* ctx, uint32_t standing, uint32_t after);

/* Standings of many rounds: one offer to S open standings at once.  A node that follows several rounds receives each gossip burst with
 * rows of all of them mixed; cut by round and offered one standing at a time, every bbp_standing_offer pays the floor of a small call --
 * seed, keys, leave pass, at least one tranche, finish, commit, several host waits each -- and they are serialised.  Here step t of every
 * standing that still runs rides ONE engine call, as in bbp_verify_rounds_best_distinct.
 * standings[s] are S handles of open standings of this context or pool, all different; standing_of[i] < S names the standing that row i
 * is offered to (NULL only when S == 1: every row to standings[0]); rows as bbp_verify_rounds_best takes the rows of rounds with
 * different N: row i is bbp_round_row_size(N of its standing) bytes, rows back to back.  A standing of the call may receive no row.
 * The rule: for every s the call reports what bbp_standing_offer(standings[s], the rows with standing_of[i] == s in ascending call index,
 * tranche, cap) would report -- n_entered[s], n_candidates[s], n_examined[s], n_duplicates[s] (S entries each), the statuses of its rows
 * (status: B entries) and entered_out[s * cap ..], which receives min(n_entered[s], cap) CALL indices in rank order (entries beyond are
 * not written) -- and afterwards bbp_standing_read of standings[s] returns what it would return after that single offer, serials
 * included: the j-th row of standing s in call order has serial offered_s + j.
 *   per standing  each standing keeps its own N, round, floor and K from bbp_standing_open; T_0 of standing s is max(tranche, K_s)
 *   steps         step t holds tranche t of every standing that still has a live candidate; a standing stops when it has none, and one
 *                 that still runs has run every step so far.  All the rows of a step are gathered by standing and verified in one
 *                 call through bbp_verify_rounds_aggregated's own path, the round table made of the S standings' stored rounds; entropy
 *                 source, BBP_HOST_CHUNK_VERIFY, the health word, verify mixing and the pool split hold as they do for
 *                 bbp_verify_rounds_best_distinct
 *   n_steps       (may be NULL) the largest number of tranches any standing ran
 *   identities    never meet across standings: one z_img resent to every standing is S identities
 *   one commit    the call works on copies in its own scratch and commits all S standings with one launch at the end, after the host's
 *                 checks.  A call that ends with BBP_ERR_DEVICE or BBP_ERR_INTERNAL leaves EVERY standing of the call and its offered
 *                 count exactly as before -- also when the flag word was raised for one standing only, as bbp_debug_standing_trip set on
 *                 any one of them does (the trip is consumed by the next offer of either kind)
 * Only score || z_img (64 bytes per row) go up for screening; a row's full bytes go up only in the step that verifies it.
 * Screening, the first failing check decides: a NULL pointer BBP_ERR_BAD_ARG (entered_out may be NULL only when cap == 0, standing_of only
 * when S == 1, n_steps always); S == 0 or S > BBP_STANDING_MAX_OPEN BBP_ERR_BAD_ARG; a handle that is unknown or closed BBP_ERR_BAD_ARG;
 * the same handle twice BBP_ERR_BAD_ARG; B > BBP_SELECT_MAX_BIDS BBP_ERR_BAD_ARG; B == 0 BBP_OK with zero counts and nothing changed;
 * standing_of[i] >= S BBP_ERR_BAD_ARG.  S == 1 runs bbp_standing_offer's own driver, as R == 1 does in the many-rounds best calls.
 * Serialised with the other best calls of the context; on a pool the standings live on member 0; bbp_reserve does NOT size the state.
 * bbp_debug_standings_offer, test hook (synchronises; a pool refuses it): the same with made-up keys, ids (B x 32 bytes each) and
 * verdicts (B x int32) in place of rows, through the shipped kernels; nothing is verified.  Beyond the screening above it refuses what
 * bbp_debug_standing_offer refuses: a verdict outside the three.
 * Out of scope: a _dev form; a server opcode; more than BBP_STANDING_MAX_OPEN standings in one call. */
int32_t bbp_standings_offer(bbp_ctx* ctx, uint32_t S, const uint32_t* standings, uint32_t B, const uint32_t* standing_of, const uint8_t* rows,
                            uint32_t tranche, uint32_t cap, uint32_t* entered_out, uint32_t* n_entered, uint32_t* n_candidates, uint32_t* n_examined,
                            uint32_t* n_duplicates, uint32_t* n_steps, int32_t* status);
int32_t bbp_debug_standings_offer(bbp_ctx* ctx, uint32_t S, const uint32_t* standings, uint32_t B, const uint32_t* standing_of, const uint8_t* keys,
                                  const uint8_t* ids, const int32_t* verdicts, uint32_t tranche, uint32_t cap, uint32_t* entered_out, uint32_t* n_entered,
                                  uint32_t* n_candidates, uint32_t* n_examined, uint32_t* n_duplicates, uint32_t* n_steps, int32_t* status);

/* Optional, once after bbp_init (or whenever a new list length N shows up): grow every per-batch buffer of the context (every member
 * of a pool) to what batches of up to max_batch proofs / verifications of list length N need, and compile the circuit for N.
 * Without it the buffers grow on demand, and a call that finds them too small frees and reallocates gigabytes under load (the
 * whole device waits: ~0.1-1 s, once per new high-water mark).  Costs about a dozen prove batches of that size (every schedule's buffers:
 * two for sliced calls, five for calls in rotation, the staging slots of the host-pointer calls); ~1.3 MB of device memory per proof and buffer. */
int32_t bbp_reserve(bbp_ctx* ctx, uint32_t max_batch, uint32_t N);

/* Micro-batching window of the call combiner, microseconds (default 0: a batch leaves as soon as the engine is free).  With a
 * window the leader of a batch waits that long for more concurrent bbp_prove / bbp_verify callers before it goes to the device --
 * what the UDS server (server/) uses to turn concurrent connections into GPU batches.  max_batch bounds one combined call. */
int32_t bbp_set_batching(bbp_ctx* ctx, uint32_t window_us, uint32_t max_batch);
/* Verify mixing (default on): concurrent bbp_verify / bbp_verify_async requests form ONE batch whatever their bid-list length and
 * record layout; a batch that holds several runs the mixed-N verifier (bbp_verify_batch_mixed's kernels, with the layout read
 * per row), one that holds a single N and layout runs bbp_verify_batch as before.  Off: one batch per bid-list length and record
 * layout, as before mixing existed -- there to measure the old grouping in the same build, and the switch to reach for should
 * mixing misbehave.  The verdicts are the same either way.  A mixed call sizes its per-row scratch by its largest N (see
 * bbp_reserve: reserve for the largest N expected).  On a pool: the pool's combiner.  bbp_describe reports the setting. */
int32_t bbp_set_verify_mixing(bbp_ctx* ctx, int32_t on);
/* Verify round sharing (default OFF): concurrent bbp_verify / bbp_verify_async requests that carry a byte-equal seed || pub_list
 * leave the call combiner as ONE bbp_verify_rounds call whose table holds every distinct round once, instead of a batch in which
 * every row repeats its round (at N = 202: 7 777 instead of 14 273 bytes per request copied and uploaded, and the table's scalars
 * reduced once per round instead of once per row).  Contract:
 *   - The status of every request is exactly what bbp_verify returns with sharing off.
 *   - Equality of rounds is equality of BYTES: two requests share a table entry when their N is equal and the 32 * (1 + N) bytes of
 *     seed || pub_list are the same.  A hash only finds the candidate; it never decides.  Lists that differ in a raw byte are two
 *     rounds even where they reduce to the same scalars, so every proof is checked against the very bytes its caller sent.
 *   - A batch takes the rounds call when every member has a compact record and it holds fewer distinct rounds than requests
 *     (R < B: the call then uploads strictly fewer bytes than the expanded rows; no tuned threshold).
 *   - Every other batch takes the path it takes with sharing off, unchanged: a batch that holds a two-phase record, a batch in
 *     which no two requests share a round (R == B, which covers a batch of one), any batch while sharing is off.
 *   - How batches are formed does not change (bbp_set_batching, bbp_set_verify_mixing: with mixing off a batch is one N and layout,
 *     and still shares the rounds of that N).
 * A rounds call of several rounds sizes its per-row scratch by its largest N, as a mixed call does (bbp_set_verify_mixing, bbp_reserve).
 * On a pool: the pool's combiner.  bbp_describe reports the setting while it is on.
 * bbp_verify_round_sharing_stats: rounds calls the combiner has issued / rows they carried / rounds their tables held since
 * bbp_init (any may be NULL); n_rounds < n_rows says that requests did share.  On a pool member: the calls dealt to that member. */
int32_t bbp_set_verify_round_sharing(bbp_ctx* ctx, int32_t on);
int32_t bbp_verify_round_sharing_stats(bbp_ctx* ctx, uint64_t* n_calls, uint64_t* n_rows, uint64_t* n_rounds);
/* Combiner statistics since bbp_init: combined device calls issued / requests they carried / largest batch (any may be NULL). */
int32_t bbp_batching_stats(bbp_ctx* ctx, uint64_t* n_calls, uint64_t* n_requests, uint32_t* max_seen);

/* Host-only synthesis check (no context, no device): compiles the blind-bid circuit for list length N exactly as bbp_prove would
 * (csrc/circuit.h mirrors src/gadgets.rs) and reports its size: n_mul = 1442 + 3N, n_cons = 2 n_mul + 3 + 3N.  N == 0 is
 * BBP_ERR_BAD_ARG (the reference panics at src/gadgets.rs:103), N > 202 BBP_ERR_GENS_LEN.  Also the place where the exception
 * barrier can be exercised without a GPU (BBP_FAULT_INJECT=compile in the environment makes the synthesis throw). */
int32_t bbp_debug_compile_circuit(uint32_t N, uint32_t* n_mul, uint32_t* n_cons);

/* Diagnostics: a short text report of what the context (every member of a pool) runs on and how it is configured -- device, free
 * memory, scheduling knobs -- into buf (NUL-terminated, truncated to cap).  Conditions known to cost throughput silently are
 * reported as lines starting with "WARNING:" (today: GPU_MAX_HW_QUEUES below the library's default, or unset while HIP was already
 * initialised when the engine was created; little free device memory).  The report also says where the hardware-queue setting came
 * from -- bbp_init exports the library's default (two queues) itself when the variable is unset and the process has not initialised
 * HIP yet -- and how much
 * scratch the context holds in how many allocations (after bbp_reserve that count stands still).
 * Environment, read once per process: BBP_DEBUG_DEVICE_CHECK=1 asserts before every HIP call made for a context that the calling
 * thread's current device is the context's (first multi-GPU bring-up); BBP_TRACE_ALLOC=1 names every scratch buffer that grows. */
int32_t bbp_describe(bbp_ctx* ctx, char* buf, uint32_t cap);

/* Test hook: poisons the sorted scratch of the context's NEXT MSM launch with an out-of-range entry (what a stray write would leave).
 * The accumulate kernel clamps the gather (no fault), raises health bit 0, and -- the point of the hook -- the host-pointer call whose
 * results were fetched next returns BBP_ERR_DEVICE instead of BBP_OK with a wrong proof. */
int32_t bbp_debug_corrupt_scratch(bbp_ctx* ctx);

/* Engine self-check (synchronises the device).  *flags bit 0: an MSM table gather was out of range since bbp_init and had to be
 * clamped, i.e. engine scratch was corrupted (the one GPU fault of round 1 was such a state); bit 1: with checked proving
 * on, a proof whose witness is satisfied failed its check twice (bbp_set_prove_check); 0 = healthy.  Both flags are
 * sticky.  Every host-pointer call (bbp_prove[_batch], bbp_verify[_batch][_aggregated], bbp_msm_batch, the asynchronous forms)
 * reads it back with its results and returns BBP_ERR_DEVICE for the whole call once it is set -- never BBP_OK with results computed
 * from corrupted scratch; callers of the stream-ordered *_dev entry points poll this function at their own synchronisation points. */
int32_t bbp_check_health(bbp_ctx* ctx, uint32_t* flags);

/* ---- Checked proving ------------------------------------------------------------------------------------------------------------
 * Proof::prove does not check its witness (src/blindbid/proof.rs:36-91): inputs that do not satisfy the circuit prove to a record
 * every verifier rejects, and a record the device computed wrongly would go out as BBP_OK too.  With checking on, every record is
 * verified on the device before it is handed out.  OFF by default; set through this call only (no environment variable).  On a
 * pool it applies to every member.
 * A witness is satisfied when the blind-bid circuit accepts it (src/gadgets.rs): m = mimc(k, 0), x = mimc(d, m); toggle < N and
 * pub_list[toggle] = x mod l (Scalar::from_bits items: an encoding of x + l passes); z_img = mimc(seed, m); mimc(seed, x) * y_inv = 1;
 * q = d * y_inv.  y is committed but not constrained: a wrong y with the right y_inv passes.
 * Host-pointer calls with checking on (bbp_prove, bbp_prove_async, bbp_prove_batch, on a context or a pool, combined or not):
 *   rows whose witness is not satisfied   BBP_ERR_BAD_ARG and a zeroed record; bbp_last_error names the first relation that failed
 *   every other record                    verified on the device (the aggregated verifier, on a verifier lane's stream)
 *   a record that fails                   proved once more with the same inputs and the same entropy (the entropy the call drew when
 *                                         none was given) and checked again: OK then, with the bytes an unchecked call with that
 *                                         entropy returns; a second failure returns BBP_ERR_DEVICE for the whole call and raises
 *                                         health bit 1 (the rule bbp_check_health's bit 0 follows)
 * Costs: one aggregated verification per proof (DESIGN.md section 10 has the measured share). */
int32_t bbp_set_prove_check(bbp_ctx* ctx, int32_t on);
/* Counts since bbp_init (a pool: the sum over its members; any pointer may be NULL; synchronises the device): rows handed to checked
 * calls, rows refused by the witness check (toggle >= N and non-canonical rows included), records proved a second time, and checks
 * that failed (on the host path each is followed by one re-prove, whose check counts again). */
int32_t bbp_prove_check_stats(bbp_ctx* ctx, uint64_t* n_checked, uint64_t* n_unsatisfied, uint64_t* n_reproved, uint64_t* n_failed);
/* The device form, whatever bbp_set_prove_check says: same input contract and stream ordering as bbp_prove_batch_dev (no host
 * screening, no synchronisation); check_entropy_dev holds B * 32 bytes that seed the verifier's weights (bbp_verify_batch_dev's
 * entropy_dev).  status_dev: B int32, per proof
 *   BBP_OK            the record verified
 *   BBP_ERR_FORMAT    one of the seven scalars is non-canonical
 *   BBP_ERR_BAD_ARG   toggle >= N, or the witness is not satisfied
 *   BBP_ERR_VERIFY    the record failed its check
 * Records of non-OK rows are zeroed; nothing is proved twice (the caller decides).  A pool refuses it, like every *_dev call. */
int32_t bbp_prove_batch_checked_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev,
                                    const void* check_entropy_dev, void* out_dev, void* status_dev, void* stream);
/* Test hook: the next prove call on the context (any of the prove entry points) adds 1 mod l to the t_x scalar of its record `index`,
 * on the device, after the prover wrote it and before any check reads it: the record still parses and fails verification (no write
 * out of bounds; an index beyond the call's batch corrupts nothing and is consumed all the same).  A pool refuses it. */
int32_t bbp_debug_corrupt_next_proof(bbp_ctx* ctx, uint32_t index);

/* ---- On-device entropy ----------------------------------------------------------------------------------------------------------
 * Every proof needs (4+N) commitment blindings and a 32-byte TranscriptRng seed (thread_rng, src/blindbid/proof.rs:53-64); every
 * verification a 32-byte seed for its weights.  These calls expand ONE 32-byte key on the device with ChaCha20 (RFC 8439 2.3:
 * 256-bit key, 32-bit block counter, 96-bit nonce, 64-byte blocks) into exactly the layouts the prove / verify entry points take,
 * one ChaCha20 stream per row (rows are re-derivable one by one):
 *   prove row i, list length N, m = 4+N   nonce = "BBPE" || u32le(N) || u32le(i); blinding k < m = the 64-byte block(key, k, nonce)
 *                                         read as a little-endian integer, mod l (from_bytes_mod_order_wide), 32 canonical bytes at 32k;
 *                                         the rng seed = the first 32 bytes of block(key, m, nonce), at 32m -- bbp_entropy_size(N) bytes
 *   verify row i                          nonce = "BBPV" || u32le(0) || u32le(i); the row = the first 32 bytes of block(key, 0, nonce)
 * A KEY USED FOR TWO CALLS REUSES EVERY BLINDING: two proofs with equal blindings reveal their witness (d, k), exactly as reusing
 * explicit `entropy` does.  Pass key32 = NULL (32 fresh OS bytes per call) unless the rows must be reproducible (tests). */
#define BBP_ENTROPY_PROVE 0u  /* rows of bbp_entropy_size(N) bytes */
#define BBP_ENTROPY_VERIFY 1u /* rows of 32 bytes (N ignored)      */
/* B rows of `kind` into out_dev (device memory, B * bbp_entropy_size(N) or B * 32 bytes) under key32 (host memory; NULL = 32 fresh
 * OS bytes).  Stream-ordered on `stream` (a hipStream_t or BBP_STREAM_CONTEXT), no synchronisation.  Prove rows follow the exception of
 * bbp_prepare_bids_dev: the next bbp_prove_batch_dev / bbp_prove_batch_checked_dev on this context waits for them by itself (an event of
 * their own: a prepare and a draw on two different streams are both waited for); verify rows are ordered by the caller, like any other
 * _dev input.  A pool refuses it, like every *_dev call. */
int32_t bbp_draw_entropy_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, uint32_t kind, const uint8_t* key32, void* out_dev, void* stream);
/* Where the host-pointer calls get their randomness when the caller gives none (bbp_prove / bbp_prove_async / bbp_prove_batch with
 * entropy == NULL, combined or not; bbp_verify[_async] / bbp_verify_batch[_aggregated], which never take any):
 *   BBP_ENTROPY_SOURCE_OS       (default) the calling thread reads 64 bytes per blinding and 32 per seed from /dev/urandom and reduces
 *                               the blindings on the host, then uploads them with the inputs
 *   BBP_ENTROPY_SOURCE_DEVICE   one 32-byte OS key per engine call (per member of a pool), expanded on the device as above, ordered
 *                               before the prover's opening stage / the verifier; the host reads 32 bytes per call
 * Rows with caller entropy are untouched; a host batch cut into chunks (BBP_HOST_CHUNK_PROVE) draws each chunk's own row range of the
 * call's key; checked proving re-proves a failed record with its row re-derived from the same key (the bytes an unchecked call returns
 * under that key).  The *_dev entry points still require entropy_dev.  On a pool: every member.  bbp_describe reports the source.
 *   BBP_ENTROPY_SOURCE_HEDGED   prove calls: as DEVICE, but every row draws under a key of its own, derived on the device from the
 *                               call's key and the row's inputs ("Hedged on-device entropy" below); verify calls draw exactly as
 *                               under DEVICE (a verification row carries no secret to hedge with) */
#define BBP_ENTROPY_SOURCE_OS 0
#define BBP_ENTROPY_SOURCE_DEVICE 1
#define BBP_ENTROPY_SOURCE_HEDGED 2
int32_t bbp_set_entropy_source(bbp_ctx* ctx, int32_t source);
/* ---- Hedged on-device entropy -----------------------------------------------------------------------------------------------------
 * Under source DEVICE the 32 OS bytes of an engine call are all that keeps its blindings from repeating: a VM snapshot restored
 * twice, a forked supervisor or a broken /dev/urandom gives the same key again, and row i of the second call then carries the
 * blindings of row i of the first over another witness (the warning in capitals above).  Source HEDGED binds each row's entropy to
 * the row itself.  For prove row i of a call with list length N, call key K (32 bytes) and input row
 *   row_i    = scalars7 || pub_list || toggle (u64 LE)            232 + 32 N raw bytes, as bbp_prove_batch takes them
 *   rowkey_i = SHA3-256("BBP-hedge-v1" || K || u32le(N) || row_i)   (FIPS 202: rate 136, suffix 0x06; 12 + 32 + 4 + 232 + 32 N bytes)
 *   nonce_i  = "BBPH" || u32le(N) || u32le(i)
 *   blinding k < 4+N = block(rowkey_i, k, nonce_i) as a little-endian integer mod l, 32 canonical bytes at 32 k
 *   rng seed         = the first 32 bytes of block(rowkey_i, 4+N, nonce_i), at 32 (4+N)
 * i.e. the prove row above under the row's own key and the nonce word "BBPH".  i is the row's index in the host call: in the
 * combined batch for combined callers, first + r in a call cut into chunks (source DEVICE numbers rows the same way).
 *   - With a repeated K, two rows share entropy only when N, all 232 + 32 N input bytes and the index are equal; their records are
 *     then byte-identical and nothing new is revealed.
 *   - With a K the adversary knows, the blindings are still unpredictable without the row's secret k (the hash's input holds it).
 * It does not hedge caller-supplied entropy or source OS, is not constant-time, and is opt-in: the default source stays OS.
 * Host-pointer prove calls without caller entropy (bbp_prove, bbp_prove_async, bbp_prove_batch, bbp_prove_round; combined or not; a
 * context or a pool) follow DEVICE's path with one change of order: the rows first (a round call: its device pass), then the row
 * keys, then the draw, all on the chunk's opening stream.  bbp_prove_round under K returns what bbp_prove_batch returns for the
 * expanded rows under K.  Checked proving keeps its contract: a failed record is proved again under the entropy row it had -- a rows
 * call re-derives the row key on the host, a round call (whose expanded row never exists on the host) fetches the failed rows' keys
 * from the device with the check's verdicts.  Row keys are secret like the rows; they live in the call's entropy buffer behind the
 * drawn rows and nowhere else.
 *
 * The device form: B prove rows into out_dev (B * bbp_entropy_size(N) bytes) from the rows at in_dev (B * (232 + 32 N) bytes, 4-byte
 * aligned; 8-byte aligned rows are read with 64-bit loads) under key32 (host memory; NULL = 32 fresh OS bytes).  Arguments are screened
 * as bbp_draw_entropy_dev screens them for prove rows; a pool refuses it.  Stream-ordered on `stream`, no synchronisation.  It READS
 * in_dev: when a bbp_prepare_bids_dev / bbp_prepare_round_dev is pending on the context, `stream` is made to wait for it first (the
 * pending prepare stays pending: the next prove call still waits for it), and the draw is then recorded as bbp_draw_entropy_dev's
 * is, so the next prove call waits for both.  Rows written by anything else are ordered by the caller.  The row keys pass through
 * the rows' own seed slots and are overwritten by the seeds: out_dev is the only memory written. */
int32_t bbp_draw_entropy_hedged_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* key32, const void* in_dev, void* out_dev, void* stream);
/* Test hook: the key of the next host-pointer call that draws on the device (source DEVICE or HEDGED, no caller entropy) instead of 32 OS bytes,
 * so that its records can be compared with an explicit-entropy call; consumed by that call.  A pool refuses it (take a member). */
int32_t bbp_debug_next_entropy_key(bbp_ctx* ctx, const uint8_t key32[32]);

/* ---- Expanded blinding draw -------------------------------------------------------------------------------------------------------
 * Every proof draws 3 + 2 n1 blinding scalars after its commitments: i_blinding1, o_blinding1, s_blinding1, s_L[n1], s_R[n1] (n1 the
 * circuit's multipliers, 1442 + 3 N: 2935 draws at N = 8, 4099 at N = 202).  merlin's TranscriptRng gives one Keccak-f[1600] per draw,
 * each permutation feeding the next: the one stretch of a prove call that no batch parallelism shortens.  The protocol needs these
 * scalars uniform and secret, not merlin's bytes, and the reference's bytes are not reproducible either (its rng is finalised with 32
 * bytes of thread_rng).  This setting chooses how they are drawn, for every prove entry point of the context (bbp_prove[_async],
 * bbp_prove_batch[_dev], bbp_prove_batch_checked_dev and checked proving's second attempt, bbp_prove_round[_dev], bbp_prove_round_select,
 * the combiner's batches):
 *   BBP_BLINDING_DRAW_MERLIN    (default) draw j = rng.fill_bytes(64) mod l, as the reference and the oracles draw
 *   BBP_BLINDING_DRAW_EXPANDED  1. transcript and TranscriptRng exactly as under MERLIN: the rng is cloned from the transcript after the
 *                                  "m" message, rekeyed with every v_blinding ("v_blinding", 32 canonical bytes each, in commit order)
 *                                  and finalised ("rng") with the row's 32-byte seed
 *                               2. key = rng.fill_bytes(32): merlin's ordinary draw, meta-AD of u32le(32), PRF of 32 bytes
 *                               3. draw j, 0 <= j < 3 + 2 n1 = the 64-byte ChaCha20 block (RFC 8439 2.3) under key, block counter j,
 *                                  nonce words ("BBPX" as a little-endian word, 0, 0), its 16 little-endian words read as one integer
 *                                  mod l (from_bytes_mod_order_wide); j = 0 i_blinding1, 1 o_blinding1, 2 s_blinding1, 3 + i s_L[i],
 *                                  3 + n1 + i s_R[i]: the order of the merlin draws
 *                               4. every later draw (the five t blindings) comes from the same rng, continuing after step 2
 *                               Commitments, challenges, the record layout and the entropy row layout stay as they are.
 *   - What the key depends on: the transcript (every commitment), every v_blinding and the external 32 bytes, through merlin's own
 *     construction.  merlin's hedge is kept: with a repeated or known seed the key still differs with the witness blindings, and with
 *     repeated blindings it still differs with the seed.
 *   - What is given up: under injected entropy an EXPANDED record is NOT the C oracle's or the reference's bytes (A_I1, A_O1, S1 and
 *     everything after them differ; the 4 + N commitments are equal).
 *   - What is kept: every verifier accepts the record (the verifier never sees how a blinding was drawn), and the record is deterministic
 *     under injected entropy (tests/expanded_draw_model.py restates the draw; tests/golden/proofs_expanded_draw.json holds records).
 *   - The default is MERLIN, with byte parity under injected entropy as before.
 * The setter takes the context lock and holds for prove calls planned after it returns; on a pool it applies to every member.  Anything
 * but the two modes: BBP_ERR_BAD_ARG, nothing changes.  bbp_blinding_draw reads the setting back (-1 for a NULL context); bbp_describe
 * names it.  bbp_reserve covers both modes whichever is set: the expanded draw needs a subset of the merlin draw's scratch. */
#define BBP_BLINDING_DRAW_MERLIN 0
#define BBP_BLINDING_DRAW_EXPANDED 1
int32_t bbp_set_blinding_draw(bbp_ctx* ctx, int32_t mode);
int32_t bbp_blinding_draw(bbp_ctx* ctx);

/* ---- Secret wiping ------------------------------------------------------------------------------------------------------------------
 * The engine proves with the bidder's secrets -- d, k, y, y^-1, the toggle, every commitment blinding, the TranscriptRng seed, a call's
 * entropy key and its hedged row keys -- and by default keeps what it computed in its batch buffers, MSM scratch, draw buffers,
 * staging slots and their pinned host mirrors until a later call overwrites it.  With wiping on, no blinding and no witness outlives
 * the call that used it.  Opt-in, default off; with it off no launch, copy or host write is added anywhere.
 *
 * Invariant while on: whenever no prove-side call is in flight on the context, every byte of every buffer the context owns and that
 * csrc/secret_map.h classes SECRET is zero, in device memory and in pinned host memory.  (Default-secret: whatever a prove-side call
 * writes is SECRET unless that table names it PUBLIC and says why.)
 *   bbp_set_secret_wipe(ctx, 1)   erases everything once and synchronises, so the invariant holds from that moment (call it while no
 *                                 call is in flight); afterwards each call erases only what it wrote.  0: erases nothing, adds nothing.
 *                                 On a pool: every member.
 *   bbp_wipe_secrets(ctx)         erases every SECRET buffer over its whole capacity now, whatever the setting; synchronises the
 *                                 device.  On a pool: every member.
 * Per call: when a host-pointer prove-side call returns, or its `done` callback fires, that call's wipes have completed (bbp_prove,
 * bbp_prove_async, bbp_prove_batch, bbp_prove_round, bbp_witness_batch, bbp_msm_batch; combined or not; a context or a pool).  For the
 * _dev forms (bbp_prove_batch_dev, bbp_prove_batch_checked_dev, bbp_prove_round_dev, bbp_prepare_round_dev, bbp_msm_batch_dev) the wipes
 * of library-owned memory are stream-ordered: complete for anything enqueued on `stream` after the call.  bbp_prepare_bids_dev and
 * bbp_draw_entropy*_dev write the caller's buffers only.  Records, statuses, toggles and every other output are byte for byte what
 * they are with wiping off; verify calls are untouched.  Also while on: a buffer that is about to be freed to grow is erased first,
 * bbp_free erases before it frees, bbp_debug_challenges returns BBP_ERR_BAD_ARG (the challenge block is erased), and bbp_describe
 * prints "secret wipe: on".
 * After a FAILED prove-side call the invariant may lapse: a _dev form that returns an error after some of its launches were enqueued
 * erases nothing more (what it reserved is erased by the next call that uses the same buffers, or by bbp_wipe_secrets); a failed
 * host-pointer call erases its staging slot and whatever it had reserved, behind a device synchronise (other calls are untouched).  Call bbp_wipe_secrets after an error that must leave nothing.
 * What it is NOT: it does not scrub caches, LDS or registers; it does not erase the caller's own buffers (inputs, entropy, device
 * rows handed to a _dev form); and it is not a constant-time claim. */
int32_t bbp_set_secret_wipe(bbp_ctx* ctx, int32_t on);
int32_t bbp_wipe_secrets(bbp_ctx* ctx);
/* Test hooks; both synchronise the whole context; a pool refuses them (take a member).
 * residue: the number of non-zero bytes over the whole capacity of every SECRET buffer, device and pinned; `where` (cap bytes, may be
 * NULL with cap 0) receives the table name of the first buffer with residue, or "".
 * scan: exact matches of pattern[0 .. len) at every 4-byte offset of every grow-only device buffer, ring, staging slot and pinned mirror
 * of the context, SECRET and PUBLIC alike, and of the resident tables (gens, ptable, btab, comb, MiMC constants).  Not walked: the
 * compiled circuits' lists and the mixed-N circuit table (uploaded once from host tables that are functions of N) and the counter
 * words (health, check counts, aggregation counts, the pinned health mirror).  len is a multiple of 4 from 4 to 64, anything else is
 * BBP_ERR_BAD_ARG.
 * wipe_cost: what the wipes enqueued since the log was last cleared stored -- *bytes in *launches k_wipe_spans launches -- and
 * *lone_us, the device time (events) of ONE k_wipe_spans launch over exactly those spans, made now on the idle device; clear != 0
 * empties the log afterwards (turning wiping on and bbp_wipe_secrets empty it too).  At most 24 spans replay in one launch (one prove
 * call logs 6 to 18): with more in the log the call is BBP_ERR_BAD_ARG, and bytes / launches are still reported. */
int32_t bbp_debug_secret_residue(bbp_ctx* ctx, uint64_t* dev_bytes, uint64_t* host_bytes, char* where, uint32_t cap);
int32_t bbp_debug_secret_scan(bbp_ctx* ctx, const uint8_t* pattern, uint32_t len, uint64_t* dev_hits, uint64_t* host_hits);
int32_t bbp_debug_wipe_cost(bbp_ctx* ctx, int32_t clear, uint64_t* bytes, uint32_t* launches, float* lone_us);
/* Test hook only -- scratch discipline: a call reads only what it wrote itself, the resident tables, or state that outlives a call by
 * contract.  The hook fills everything else with `word`, so that a kernel that reads a row, counter or bucket of an earlier call, or
 * one that it should have cleared first, computes a wrong byte instead of a plausible one.
 * It takes the context lock, synchronises the device and fills, over their whole capacity (the allocation slack included), every
 * grow-only device buffer, ring and staging slot of the context with the 32-bit `word`, and on the host every pinned mirror and the
 * verifier lanes' pinned N staging; then it synchronises again.  Not filled: the buffers csrc/secret_map.h exempts with a reason
 * (BBP_POISON_EXEMPT: an open standing's entries), the resident tables, the compiled circuits and the counter words (health, check
 * counts, aggregation counts, the pinned health mirror).  What a wiping call owes is left as it is.  *dev_bytes / *host_bytes: the
 * bytes filled; *n_buffers: the device buffers filled.
 * sticky != 0: the context remembers `word`, and until a call with sticky == 0 every buffer the context newly allocates -- the first
 * call of a fresh context, every regrowth -- starts out filled with it (with secret wiping on it starts out zero, as always).
 * Use small words (the tests use 1 and 3): an index or count read from the fill then stays inside the allocation slack, a status is a
 * real error code, a scalar is canonical and non-zero.  No call of the context may be in flight; a pool refuses it (take a member). */
int32_t bbp_debug_poison_scratch(bbp_ctx* ctx, uint32_t word, int32_t sticky, uint64_t* dev_bytes, uint64_t* host_bytes, uint32_t* n_buffers);

/* Parity hook: the 32-scalar challenge block of proof `proof` of the LAST batch call of geometry (B, N):
 * y z u x w y^-1 t1..t6 tb1..tb6 t_x t_x~ e~ ... (MiscSlot order in csrc/batch_layout.h), 32 x 32 bytes. */
int32_t bbp_debug_challenges(bbp_ctx* ctx, uint32_t B, uint32_t N, uint32_t proof, uint8_t* out32x32);

/* Test hook: where one of the context's resident tables lives on the device and how large it is (csrc/context.h "resident tables"):
 *   BBP_TABLE_GENS     8396 extended points of 160 bytes: the BBP_NUM_BASES public bases at their BBP_BASE_* indices, then the 202 range
 *                      sums (index 4098 + N - 1 = H[418 + 3N] + .. + H[1023]), then MRG1(i) = G[i] + H[i] + H[i+1] at 4300 + i and
 *                      MRG2(i) = G[i] + G[i+1] + H[i+1] at 4300 + 2048 + i, i = 0..2047 (i = 2047: some valid point, never referenced)
 *   BBP_TABLE_PTABLE   8396 x 256 rows of 128 bytes: row (i, b) is 2^b * gens[i] in the MSM kernels' cached affine form
 *   BBP_TABLE_COMB     2 x 64 x 8 entries of 96 bytes: entry (base, j, m - 1) is m * 16^j * Base, Base = B, B_blinding
 *   BBP_TABLE_BTAB     the tail table of B that the prover's k_tail_tables built at bbp_init: 160-byte points
 *   BBP_TABLE_IDX(list, N)   one of the base-index lists (uint32 indices into gens; 0xffffffff: a term that rides on a merged
 *                      base) that the MSMs of list length N are launched with, the circuit compiled now if it was not yet:
 *                      BBP_TABLE_IDX_AI / _AO / _S1 (1 + 2 n_mul, 1 + n_mul, 1 + 2 n_mul entries, n_mul = 1442 + 3N), _IPA
 *                      (11 rounds x {L, R} x 2049), _VER (4098).  N == 0 is BBP_ERR_BAD_ARG, N > BBP_MAX_ITEMS BBP_ERR_GENS_LEN.
 * The pointer stays valid until bbp_free and is for reading, by kernels of the same process.  A pool refuses it (take a member). */
#define BBP_TABLE_GENS 0u
#define BBP_TABLE_PTABLE 1u
#define BBP_TABLE_COMB 2u
#define BBP_TABLE_BTAB 3u
#define BBP_TABLE_IDX_AI 4u
#define BBP_TABLE_IDX_AO 5u
#define BBP_TABLE_IDX_S1 6u
#define BBP_TABLE_IDX_IPA 7u
#define BBP_TABLE_IDX_VER 8u
#define BBP_TABLE_IDX(list, N) ((list) | ((uint32_t)(N) << 8))
int32_t bbp_debug_table(bbp_ctx* ctx, uint32_t which, const void** dev, uint64_t* bytes);

/* Test hook: the verifier's variable-base kernels, as shipped and with the verify path's launch geometry, on caller-made rows; the
 * call synchronises.  form:
 *   BBP_VARBASE_LANES         k_varbase, Q lanes and Q partial sums per row
 *   BBP_VARBASE_PREP_SUM      k_varprep + k_varsum, one sum per row (Q ignored)
 *   BBP_VARBASE_MX_LANES      k_varbase_mx   } rows of any mix of list lengths and record versions, the row stride
 *   BBP_VARBASE_MX_PREP_SUM   k_varprep_mx + k_varsum_mx   } that of the largest row; the first two forms take one N and one version
 * Row p has list length ns[p] (m = 4 + N, np = 6 + m + 5 + 22 point slots) and record version vers[p] (0: one-phase, slots 3..5
 * are skipped; 1: two-phase).  Host arrays, rows packed back to back:
 *   pts       np 32-byte encodings per row, in slot order: A_I1 A_O1 S1 A_I2 A_O2 S2, the m commitments, T_1 T_3..T_6, L[11], R[11]
 *   scalars   x, r, u, rho per row (4 x 32 bytes);  wv: m scalars per row;  uj: u_j[11] then u_j^-1[11] per row
 * Every scalar must be canonical.  agg != 0: every slot's scalar is multiplied by rho (the aggregated verifier's weight).
 * Outputs: sums_out, nq 32-byte encodings per row (nq = Q for the LANES forms, 1 otherwise; a lane without a point gives the
 * identity); digits_out, 8 words per point slot, packed like pts (slots no kernel wrote stay 0); status_out, B statuses (BBP_OK,
 * or BBP_ERR_VERIFY for a row with a point that does not decode).
 * B is 1..1024, N 1..202, Q 1..1024: anything else, a null pointer or a non-canonical scalar is BBP_ERR_BAD_ARG and nothing is
 * launched; every device buffer is sized from these counts.  A pool refuses it. */
#define BBP_VARBASE_LANES 0u
#define BBP_VARBASE_PREP_SUM 1u
#define BBP_VARBASE_MX_LANES 2u
#define BBP_VARBASE_MX_PREP_SUM 3u
int32_t bbp_debug_varbase(bbp_ctx* ctx, uint32_t form, uint32_t B, uint32_t Q, uint32_t agg, const uint32_t* ns, const uint8_t* vers,
                          const uint8_t* pts, const uint8_t* scalars, const uint8_t* wv, const uint8_t* uj, uint8_t* sums_out,
                          uint32_t* digits_out, int32_t* status_out);

/* Integer-ALU roofline microbenchmarks (register-resident chains, no memory): kind 0 = v_mad_u64_u32, 1 = field multiply,
 * 2 = field square, 3 = mixed point addition, 4 = Montgomery product mod l, 5 = mixed point addition with an operand the
 * compiler cannot hoist (a gathered table row).  *ops_per_sec receives operations per second. */
int32_t bbp_ubench(bbp_ctx* ctx, int32_t kind, uint32_t blocks, uint32_t iters, double* ops_per_sec);

/* Per-kernel device timings: with profiling on, every kernel launch is bracketed by HIP events on its launch stream.
 * bbp_last_timings synchronises, drains them as (tag, microseconds) float pairs (tags: 1 = MSM accumulate kernel, 11 = MSM sort kernel, 12 = MSM fold kernel, 2 = encode, ...)
 * and reports the number of floats written in *n. */
int32_t bbp_set_profiling(bbp_ctx* ctx, int32_t on);
int32_t bbp_last_timings(bbp_ctx* ctx, float* out, uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif
