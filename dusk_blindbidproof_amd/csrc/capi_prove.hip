// C-ABI: prove / verify / witness entry points -- see include/bbp.h for the reference interface each replaces.
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <optional>
#include <thread>

#include "batch.h"
#include "chacha.h"
#include "hedge.h"
#include "round_bids.h"
#include "round_best.h"
#include "round_select.h"
#include "round_standing.h"
#include "rounds_best.h"
#include "rounds_best_distinct.h"
#include "secret_map.h"
#include "submit.h"
#include "witness_check.h"

namespace bbp {
int32_t prove_batch_dev(bbp_ctx* ctx, u32 B, u32 N, const u8* in_dev, const u8* ent_dev, u8* out_dev, hipStream_t s,
                        const std::function<int32_t(hipStream_t)>* open_hook = nullptr);
// verifier.inc: the plain and the aggregated driver; what the rows are travels in the descriptor (verify_rows.h)
int32_t verify_batch_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s);
int32_t verify_batch_agg_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s,
                             u32* n_fallback, u32* total_out_dev = nullptr);
int32_t debug_read_misc(bbp_ctx* ctx, u32 B, u32 N, u32 proof, uint8_t* out);
int32_t debug_varbase(bbp_ctx* ctx, u32 form, u32 B, u32 Q, u32 agg, const u32* ns, const u8* vers, const u8* pts, const u8* scal, const u8* wv,
                      const u8* uj, u8* sums_out, u32* digits_out, int32_t* status_out);
// verifier.inc: k_round_consts for one round (the prove side's table reduction)
int32_t round_consts_launch(bbp_ctx* ctx, u32 N, const u8* round_dev, const u32* roff_dev, sc* rblk, int32_t* rflag, hipStream_t s);

// native (non-circuit) image of the gadget wiring: what the reference's Go caller computes before Proof::prove
// (src/gadgets.rs:20-33 for m,x,y,z; :70-86 for y_inv and q)
__device__ sc mimc_native(sc x, const sc& key, const sc* __restrict__ c) {
    for (int i = 0; i < BBP_MIMC_ROUNDS; i++) {
        sc a = sc_add(sc_add(x, key), ld_sc(&c[i]));
        sc a2 = sc_mul(a, a), a3 = sc_mul(a2, a), a4 = sc_mul(a2, a2);
        x = sc_mul(a4, a3);
    }
    return sc_add(x, key);
}

__global__ void k_witness_native(u32 B, const u8* __restrict__ dks, const sc* __restrict__ mimc, u8* __restrict__ out) {
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const u32* in = reinterpret_cast<const u32*>(dks + 96 * (size_t)p);
    sc d = sc_reduce256(in), k = sc_reduce256(in + 8), seed = sc_reduce256(in + 16);
    sc m = mimc_native(k, sc_zero(), mimc);
    sc x = mimc_native(d, m, mimc);
    sc y = mimc_native(seed, x, mimc);
    sc z = mimc_native(seed, m, mimc);
    sc yi = sc_invert(y);
    sc q = sc_mul(d, yi);
    sc* o = reinterpret_cast<sc*>(out + 192 * (size_t)p);
    st_sc(&o[0], m);
    st_sc(&o[1], x);
    st_sc(&o[2], y);
    st_sc(&o[3], yi);
    st_sc(&o[4], q);
    st_sc(&o[5], z);
}

// the caller-side pass (Go, upstream of Proof::prove) on the device, writing the prover's and the verifier's
// input rows directly.  One lane per bid.  bids: d || k || seed (96 B); lists: N x 32 B (entry `toggle` is replaced by the
// bid's own x); toggles: u64.  prove_in row: d,k,y,y_inv,q,z_img,seed || list || toggle; verify_tail row: q || z_img || seed || list.
__global__ void k_prepare_bids(u32 B, u32 N, const u8* __restrict__ bids, const u8* __restrict__ lists, const u64* __restrict__ toggles,
                               const sc* __restrict__ mimc, u32* __restrict__ prove_in, u32* __restrict__ verify_tail) {
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const u32* in = reinterpret_cast<const u32*>(bids + 96 * (size_t)p);
    sc d = sc_reduce256(in), k = sc_reduce256(in + 8), seed = sc_reduce256(in + 16);
    sc m = mimc_native(k, sc_zero(), mimc);
    sc x = mimc_native(d, m, mimc);
    sc y = mimc_native(seed, x, mimc);
    sc z = mimc_native(seed, m, mimc);
    sc yi = sc_invert(y);
    sc q = sc_mul(d, yi);
    const u64 toggle = toggles[p];
    const size_t pw = prove_in_words(N), vw = verify_tail_words(N);  // row lengths in words
    u32* o = prove_in + pw * p;
    const sc seven[7] = {d, k, y, yi, q, z, seed};
    for (int i = 0; i < 7; i++)
        for (int w = 0; w < 8; w++) o[8 * i + w] = seven[i].v[w];
    o[prove_in_toggle_word(N)] = (u32)toggle;
    o[prove_in_toggle_word(N) + 1] = (u32)(toggle >> 32);
    u32* v = verify_tail ? verify_tail + vw * p : nullptr;
    if (v)
        for (int w = 0; w < 8; w++) {
            v[w] = q.v[w];
            v[8 + w] = z.v[w];
            v[16 + w] = seed.v[w];
        }
    const u32* li = reinterpret_cast<const u32*>(lists + 32 * (size_t)N * p);
    for (u32 i = 0; i < N; i++)
        for (int w = 0; w < 8; w++) {
            const u32 word = (u64)i == toggle ? x.v[w] : li[8 * i + w];
            o[PROVE_IN_LIST_WORD + 8 * i + w] = word;
            if (v) v[VERIFY_TAIL_LIST_WORD + 8 * i + w] = word;
        }
}

// ---- checked proving (bbp_set_prove_check, bbp_prove_batch_checked_dev) -------------------------------------------------------
// Witness check: one lane per proof, the relations of witness_check.h on the input row; reads inputs only, so it runs on the
// opening stream beside the draw chain (prove_batch_dev's open_hook).  mask[p] = failed-relation bits (0 = satisfied).
__global__ void k_witness_check(u32 B, u32 N, const u8* __restrict__ in, const sc* __restrict__ mimc, u32* __restrict__ mask) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    mask[p] = witness_check_row(N, reinterpret_cast<const u32*>(in) + prove_in_words(N) * p, mimc);
}

// Verify-row assembly: record || q || z_img || seed || pub_list (bbp_verify_batch's row) from the output records and the input rows
// (scalars 4, 5, 6 and the list).  Records are 1121 + 32 m bytes -- odd -- so the copy goes byte by byte, one byte per lane.
__global__ void k_check_rows(u32 B, u32 N, const u8* __restrict__ in, const u8* __restrict__ recs, u8* __restrict__ rows) {
    const size_t rec = BBP_R1CS_PROOF_BYTES + 32 * (4 + (size_t)N), in_stride = prove_in_bytes(N), row = rec + verify_tail_bytes(N);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= row * B) return;
    const size_t p = i / row, o = i - p * row;
    rows[i] = o < rec ? recs[rec * p + o] : in[in_stride * p + PROVE_IN_Q + (o - rec)];  // o - rec < 96: q, z_img, seed; beyond: the list, which follows them
}

// Status merge (caller's stream, after the check has joined): per proof, in the host path's screening order,
//   toggle >= N -> BBP_ERR_BAD_ARG, non-canonical scalar -> BBP_ERR_FORMAT, witness not satisfied -> BBP_ERR_BAD_ARG,
//   record rejected -> BBP_ERR_VERIFY, else BBP_OK.
// Records of non-OK rows are zeroed.  counts[0] / counts[1] (context-wide) count refused rows / rejected records; with fail_idx,
// the rejected rows (idx_base + p) are compacted there behind the counter *fail_n (host path: the rows it proves once more).
__global__ void k_check_merge(u32 B, u32 N, const u32* __restrict__ mask, const int32_t* __restrict__ vstatus, u8* __restrict__ recs,
                              int32_t* __restrict__ status, unsigned long long* __restrict__ counts, u32* __restrict__ fail_n,
                              u32* __restrict__ fail_idx, u32 idx_base) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const u32 f = mask[p];
    const int32_t st = (f & WC_TOGGLE) ? BBP_ERR_BAD_ARG : (f & WC_FORMAT) ? BBP_ERR_FORMAT : f ? BBP_ERR_BAD_ARG
                     : vstatus[p] != BBP_OK ? BBP_ERR_VERIFY : BBP_OK;
    status[p] = st;
    if (st == BBP_OK) return;
    const size_t rec = BBP_R1CS_PROOF_BYTES + 32 * (4 + (size_t)N);
    for (size_t o = 0; o < rec; o++) recs[rec * p + o] = 0;
    atomicAdd(&counts[st == BBP_ERR_VERIFY ? 1 : 0], 1ull);
    if (st == BBP_ERR_VERIFY && fail_idx) fail_idx[atomicAdd(fail_n, 1u)] = idx_base + p;
}

// bbp_debug_corrupt_next_proof: t_x (record bytes 257..288: version, eight points, then t_x) += 1 mod l, still canonical
__global__ void k_corrupt_tx(u8* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    u8* t = rec + 1 + 8 * 32;
    u32 w[8];
    for (int i = 0; i < 8; i++) w[i] = (u32)t[4 * i] | (u32)t[4 * i + 1] << 8 | (u32)t[4 * i + 2] << 16 | (u32)t[4 * i + 3] << 24;
    const sc v = sc_add(sc_reduce256(w), sc_one());
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) t[4 * i + b] = (u8)(v.v[i] >> (8 * b));
}

// On-device entropy (bbp_draw_entropy_dev, bbp_set_entropy_source; the expansion is csrc/chacha.h): one lane per 32-byte slot, i.e.
// one ChaCha20 block, consecutive lanes on consecutive slots of a row (prove rows: 5 + N slots, verify rows: one), so a wavefront's
// stores cover 2 KB without a gap.  Rows row_base.. of the key's streams; no LDS, no atomics.
__global__ void __launch_bounds__(64) k_draw_entropy(u32 n_slots, u32 N, u32 kind, u32 row_base, ChachaKey key, u32* __restrict__ out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_slots) return;
    u32 w[8];
    if (kind == BBP_ENTROPY_PROVE) {
        const u32 per = 5 + N, r = g / per;
        entropy_prove_slot(key, N, row_base + r, g - r * per, w);
    } else {
        entropy_verify_row(key, row_base + g, w);
    }
    u32* o = out + 8 * (size_t)g;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = w[i];
}

// Hedged on-device entropy (bbp_set_entropy_source(HEDGED), bbp_draw_entropy_hedged_dev; the derivation is csrc/hedge.h).
// A device row as 64-bit words: one 64-bit load where the rows are 8-byte aligned (their stride always is), else two 32-bit loads.
template <bool A8>
struct HedgeRowDev {
    const u32* p;
    __device__ __forceinline__ u64 operator()(u32 r) const {
        if (A8) return reinterpret_cast<const u64*>(p)[r];
        return (u64)p[2 * r] | (u64)p[2 * r + 1] << 32;
    }
};
// Row keys: one wavefront (one 64-lane workgroup) per row, the sponge spread over the lanes (hedge.h hedge_row_key_wave; 3 blocks at
// N = 8, 50 at N = 202): the state stays in registers, a block is one 136-byte load of 17 lanes.  Row p of `in` (stride
// prove_in_words(N)) -> 8 words at keys + key_stride p.  No LDS memory, no atomics, no private segment.
template <bool A8>
__global__ void __launch_bounds__(64) k_hedge_keys(u32 B, u32 N, ChachaKey key, const u32* __restrict__ in, u32* __restrict__ keys, u32 key_stride) {
    const u32 p = blockIdx.x;
    if (p >= B) return;
    hedge_row_key_wave(key, N, HedgeRowDev<A8>{in + prove_in_words(N) * p}, threadIdx.x, keys + (size_t)key_stride * p);
}
// The draw under per-row keys: k_draw_entropy's layout (one lane per 32-byte slot, consecutive lanes on consecutive slots), the key read
// from keys + key_stride r.  A launch covers slots slot0 .. slot0 + per - 1 of every row (the whole row: slot0 = 0, per = 5 + N).
// keys may lie inside out (bbp_draw_entropy_hedged_dev keeps each row's key in the row's seed slot): the launch that writes that slot
// has per = 1, so the only lane that reads the key is the one that overwrites it, after reading.
__global__ void __launch_bounds__(64) k_draw_entropy_rowkey(u32 n_slots, u32 N, u32 row_base, u32 per, u32 slot0, const u32* keys, u32 key_stride,
                                                            u32* out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_slots) return;
    const u32 r = g / per, slot = slot0 + (g - r * per);
    ChachaKey k;
    const u32* kp = keys + (size_t)key_stride * r;
#pragma unroll
    for (int i = 0; i < 8; i++) k.w[i] = kp[i];
    u32 w[8];
    hedge_prove_slot(k, N, row_base + r, slot, w);
    u32* o = out + 8 * ((size_t)r * (5 + N) + slot);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = w[i];
}

__global__ void k_health_or(u32* __restrict__ health, u32 bits) {
    if (threadIdx.x == 0) atomicOr(health, bits);
}

// proofs per engine call when a host-pointer batch API is handed more (BBP_HOST_CHUNK_PROVE / BBP_HOST_CHUNK_VERIFY)
static uint32_t env_chunk(const char* name, uint32_t dflt) {
    const char* e = getenv(name);
    const long v = e ? atol(e) : 0;
    return v >= 1 ? (uint32_t)v : dflt;
}
static uint32_t host_chunk_prove() { return env_chunk("BBP_HOST_CHUNK_PROVE", 16384); }
static uint32_t host_chunk_verify() { return VerifyKnobs::host_chunk_now(); }  // verify_plan.h lists the name

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static bool os_random(uint8_t* buf, size_t n) {
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) return false;
    size_t got = fread(buf, 1, n, f);
    fclose(f);
    return got == n;
}

// B rows of `kind` (rows row_base.. of the key's streams) into out on s
static int32_t draw_enqueue(bbp_ctx* ctx, u32 B, u32 N, u32 kind, const ChachaKey& key, u32 row_base, void* out, hipStream_t s) {
    const u64 n = kind == BBP_ENTROPY_PROVE ? (u64)B * (5 + N) : (u64)B;
    if (n > 0x7fffffffull || (u64)row_base + B > 0x100000000ull) {
        ctx->err = "entropy draw: too many rows for one call";
        return BBP_ERR_BAD_ARG;
    }
    ScopedEvent ev(ctx, TAG_RNG, s);
    hipLaunchKernelGGL(k_draw_entropy, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (u32)n, N, kind, row_base, key, (u32*)out);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

// Hedged: B prove rows (rows row_base.. of the call) into out on s from the device rows `in` under call key `key`.  keys != NULL: the
// row keys go to keys (32 bytes per row) and stay there; NULL: each passes through its row's seed slot in `out` and is overwritten by
// the seed (slots 0 .. 3+N first, then the seed slot by the lane that read the key).
static int32_t hedged_draw_enqueue(bbp_ctx* ctx, u32 B, u32 N, const ChachaKey& key, u32 row_base, const void* in, void* keys, void* out, hipStream_t s) {
    const u32 per = 5 + N;
    const u64 n = (u64)B * per;
    if (n > 0x7fffffffull || (u64)row_base + B > 0x100000000ull) {
        ctx->err = "entropy draw: too many rows for one call";
        return BBP_ERR_BAD_ARG;
    }
    u32* const kp = keys ? (u32*)keys : (u32*)out + 8 * (per - 1);
    const u32 kstride = keys ? 8 : 8 * per;
    {  // bbp_set_profiling: two TAG_RNG entries per call, the row keys and then the draw
        ScopedEvent ev(ctx, TAG_RNG, s);
        if (((uintptr_t)in & 7) == 0)
            hipLaunchKernelGGL(k_hedge_keys<true>, dim3(B), dim3(64), 0, s, B, N, key, (const u32*)in, kp, kstride);
        else
            hipLaunchKernelGGL(k_hedge_keys<false>, dim3(B), dim3(64), 0, s, B, N, key, (const u32*)in, kp, kstride);
        BBP_HIP_TRY(ctx, hipGetLastError());
    }
    ScopedEvent ev(ctx, TAG_RNG, s);
    if (keys) {
        hipLaunchKernelGGL(k_draw_entropy_rowkey, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (u32)n, N, row_base, per, 0u, (const u32*)kp, kstride, (u32*)out);
        BBP_HIP_TRY(ctx, hipGetLastError());
        return BBP_OK;
    }
    const u64 n1 = n - B;
    hipLaunchKernelGGL(k_draw_entropy_rowkey, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, (u32)n1, N, row_base, per - 1, 0u, (const u32*)kp, kstride, (u32*)out);
    BBP_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_draw_entropy_rowkey, dim3((B + 63) / 64), dim3(64), 0, s, B, N, row_base, 1u, per - 1, (const u32*)kp, kstride, (u32*)out);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}


// The device pass of a round call on s (round_bids.h), in the three steps that can be enqueued separately.  scratch: the RoundScratch
// `rs` of the whole call.  (1) the table, reduced once per call: the two round offsets k_round_consts reads are written in stream order
// (no host memory involved)
static int32_t round_reduce_enqueue(bbp_ctx* ctx, u32 N, const u8* table, u8* scratch, const RoundScratch& rs, hipStream_t s) {
    u32* roff = (u32*)(scratch + rs.roff);
    BBP_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)roff, 0, 1, s));
    BBP_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(roff + 1), (int)(1 + N), 1, s));
    return round_consts_launch(ctx, N, table, roff, (sc*)(scratch + rs.rblk), (int32_t*)(scratch + rs.rflag), s);
}
// (2) the bid kernel over B bids into rb; n_dev (or NULL): a device-side count below B (round_bids.h)
static int32_t round_bids_enqueue(bbp_ctx* ctx, u32 N, u8* scratch, const RoundScratch& rs, u32 B, const u8* bids, u32* rb, const u32* n_dev,
                                  hipStream_t s) {
    int32_t rc;
    unsigned hog = 0;  // a serial wave of four MiMC chains beside other calls' heavy stages: fenced onto CUs of its own, as k_prepare_bids
    if ((rc = serial_lds_bytes(ctx, (const void*)k_round_bids, &hog))) return rc;
    hipLaunchKernelGGL(k_round_bids, dim3((B + 63) / 64), dim3(64), hog, s, B, N, bids, (const sc*)(scratch + rs.rblk), (const int32_t*)(scratch + rs.rflag),
                       ctx->mimc_c, rb, n_dev);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}
// (3) the expansion of rb into the prover's rows, tails, toggles, statuses
static int32_t round_expand_enqueue(bbp_ctx* ctx, u32 N, const u8* table, u32 B, const u8* bids, const u32* rb, u32* prove_in, u32* tails, u32* toggles,
                                    int32_t* status, const u32* n_dev, hipStream_t s) {
    const u64 n = (u64)B * (round_in_words(N) + RB_EXTRA_WORDS);
    hipLaunchKernelGGL(k_round_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), lds_token(ctx), s, (u32)n, N, bids, table, rb, prove_in, tails, toggles,
                       status, n_dev);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}
static int32_t round_lanes_ok(bbp_ctx* ctx, u32 N, u32 B) {
    if ((u64)B * (round_in_words(N) + RB_EXTRA_WORDS) > 0x7fffffffull) {
        ctx->err = "round prepare: too many bids for one call";
        return BBP_ERR_BAD_ARG;
    }
    return BBP_OK;
}
// All three: bids first.. of a call; `reduce`: the table is reduced first.  bids / prove_in / tails / toggles / status point at bid `first`.
static int32_t round_prepare_enqueue(bbp_ctx* ctx, u32 N, const u8* table, u8* scratch, const RoundScratch& rs, bool reduce, u32 first, u32 B,
                                     const u8* bids, u32* prove_in, u32* tails, u32* toggles, int32_t* status, hipStream_t s) {
    int32_t rc;
    if ((rc = round_lanes_ok(ctx, N, B))) return rc;
    u32* rb = (u32*)(scratch + rs.rb) + (size_t)RB_WORDS * first;
    if (reduce && (rc = round_reduce_enqueue(ctx, N, table, scratch, rs, s))) return rc;
    ScopedEvent ev(ctx, TAG_WITNESS, s);
    if ((rc = round_bids_enqueue(ctx, N, scratch, rs, B, bids, rb, nullptr, s))) return rc;
    return round_expand_enqueue(ctx, N, table, B, bids, rb, prove_in, tails, toggles, status, nullptr, s);
}

// record || score || z_img rows from the records and the per-bid results of the pass, on s
static int32_t round_rows_enqueue(bbp_ctx* ctx, u32 B, u32 N, const u8* recs, const u32* rb, u8* rows, hipStream_t s) {
    const u64 n = (u64)round_row_bytes(N) * B;
    if ((n + 255) / 256 > 0x7fffffffull) {
        ctx->err = "round rows: too many bids for one call";
        return BBP_ERR_BAD_ARG;
    }
    ScopedEvent ev(ctx, TAG_VERIFY_SCALARS, s);
    hipLaunchKernelGGL(k_round_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), lds_token(ctx), s, B, N, recs, rb, rows);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

}  // namespace bbp

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

extern "C" int32_t bbp_witness_batch(bbp_ctx* ctx, uint32_t B, const uint8_t* dks, uint8_t* out) {
    if (!ctx || !dks || !out) return BBP_ERR_BAD_ARG;
    if (B == 0) return BBP_OK;
    if (is_pool(ctx)) return bbp_witness_batch(ctx->members[0], B, dks, out);  // microseconds of work: one member does it
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        int32_t rc;
        if ((rc = dev_reserve(ctx, ctx->io_in, 96 * (size_t)B)) || (rc = dev_reserve(ctx, ctx->io_out, 192 * (size_t)B))) return rc;
        StreamGuard guard(ctx, ctx->stream);  // io_in / io_out are shared with the other host-pointer entry points
        if ((rc = guard.enter())) return rc;
        BBP_HIP_TRY(ctx, hipMemcpyAsync(ctx->io_in.p, dks, 96 * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
        {
            ScopedEvent ev(ctx, TAG_WITNESS, ctx->stream);
            hipLaunchKernelGGL(k_witness_native, dim3((B + 63) / 64), dim3(64), 0, ctx->stream, B, (const u8*)ctx->io_in.p, ctx->mimc_c,
                               (u8*)ctx->io_out.p);
            BBP_HIP_TRY(ctx, hipGetLastError());
        }
        BBP_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->io_out.p, 192 * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
        if (wipe_on(ctx)) {  // secret wiping: d, k, seed and what was computed from them, behind the copy that hands the results out
            WipeList wl;
            wipe_take(wl, ctx->io_in);
            wipe_take(wl, ctx->io_out);
            if ((rc = wipe_enqueue(ctx, wl, ctx->stream))) return rc;
        }
        BBP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return BBP_OK;
    });
}

static int32_t check_n(bbp_ctx* ctx, uint32_t N) {
    if (N == 0) {
        ctx->err = "empty bid list (the reference panics at src/gadgets.rs:103)";
        return BBP_ERR_BAD_ARG;
    }
    if (N > BBP_MAX_ITEMS) {
        ctx->err = "bid list needs more than 2048 multipliers (R1CSError::InvalidGeneratorsLength)";
        return BBP_ERR_GENS_LEN;
    }
    return BBP_OK;
}

extern "C" int32_t bbp_prepare_bids_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* bids_dev, const void* lists_dev,
                                        const void* toggles_dev, void* prove_in_dev, void* verify_tail_dev, void* stream) {
    if (!ctx || !bids_dev || !lists_dev || !toggles_dev || !prove_in_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_prepare_bids_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc = check_n(ctx, N);
        if (rc) return rc;
        if (B == 0) return BBP_OK;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        // one lane per bid, 4 x 90 sequential MiMC rounds: a serial wave that lives for milliseconds.  In a pipeline it runs beside
        // another chunk's MSM stage, so it is fenced onto CUs of its own like the prover's opening kernels
        unsigned hog = 0;  // what the launch may ask for: the reservation minus the kernel's own static LDS (serial_lds_bytes sets the attribute to exactly this)
        if ((rc = serial_lds_bytes(ctx, (const void*)k_prepare_bids, &hog))) return rc;
        {
            ScopedEvent ev(ctx, TAG_WITNESS, s);
            hipLaunchKernelGGL(k_prepare_bids, dim3((B + 63) / 64), dim3(64), hog, s, B, N, (const u8*)bids_dev, (const u8*)lists_dev,
                               (const u64*)toggles_dev, ctx->mimc_c, (u32*)prove_in_dev, (u32*)verify_tail_dev);
            BBP_HIP_TRY(ctx, hipGetLastError());
        }
        // the prover's opening stage does not wait for the caller's stream (bbp.h); it does wait for this event
        BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_prep, s));
        ctx->ev_prep_valid = true;
        return BBP_OK;
    });
}

// ---- host-pointer batch calls: three staging slots, lock held only while enqueueing (context.h IoSlot) ---------------------------
namespace bbp {
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
// Waiting for a slot's event with the context lock released.  hipEventSynchronize by default; BBP_WAIT_POLL_US=n polls
// hipEventQuery every n microseconds instead (no measurable difference on MI355X / ROCm 7.2 once the copies were kept out of
// the DMA queues' way -- see fetch_results -- 18.7 k vs 18.6 k proofs/s from two threads; kept as a knob for runtimes where a
// thread parked in the runtime gets in the way of other threads' launches).
static hipError_t wait_event_polling(hipEvent_t ev) {
    static const int poll_us = [] {
        const char* e = getenv("BBP_WAIT_POLL_US");
        return e ? atoi(e) : 0;
    }();
    if (poll_us <= 0) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        usleep((useconds_t)poll_us);
    }
}

static int32_t pinned_reserve(bbp_ctx* ctx, void*& p, size_t& cap, size_t bytes) {
    if (cap >= bytes) return BBP_OK;
    if (p && wipe_on(ctx)) secure_zero(p, cap);  // secret wiping: a mirror goes back to the driver erased (its slot is this call's: nothing is in flight on it)
    if (p) BBP_HIP_TRY(ctx, hipHostFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = (bytes + (bytes >> 3) + 4096 + 15) & ~(size_t)15;  // whole 16-byte grains, like dev_reserve's
    BBP_HIP_TRY(ctx, hipHostMalloc(&p, want, hipHostMallocDefault));
    if (wipe_on(ctx)) memset(p, 0, want);  // ... and a new one starts out zero: a call erases what it wrote, not the capacity
    cap = want;
    return BBP_OK;
}
// inputs of a host-pointer call: caller's (pageable) memory -> the slot's pinned mirror -> device, on the context's copy stream.
// The main stream may still be busy with the previous call's MSM stage, and the opening stage of THIS call is meant to run under
// it; it only needs complete inputs (include/bbp.h), hence the wait -- on the copy's own event, polled.
// `b` lands at byte ent_off of the slot's entropy buffer, which holds at least ent_off + nb bytes afterwards (a device draw fills
// what lies below ent_off).  a2 (na2 bytes, optional): a second input that travels in the same copy and lands at byte a2_off >= na of the
// slot's input buffer (the round table of bbp_verify_rounds behind its rows).
static int32_t upload_inputs(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const uint8_t* a, size_t na, const uint8_t* b, size_t nb, size_t ent_off = 0,
                             const uint8_t* a2 = nullptr, size_t na2 = 0, size_t a2_off = 0) {
    int32_t rc;
    const size_t na1 = na;
    if (a2) na = a2_off + na2;
    if ((rc = dev_reserve(ctx, sl.in, na)) || (rc = dev_reserve(ctx, sl.ent, ent_off + nb)) || (rc = pinned_reserve(ctx, sl.h_in, sl.h_in_cap, na + nb))) return rc;
    memcpy(sl.h_in, a, na1);
    if (a2) memcpy((uint8_t*)sl.h_in + a2_off, a2, na2);
    if (nb) memcpy((uint8_t*)sl.h_in + na, b, nb);
    BBP_HIP_TRY(ctx, hipMemcpyAsync(sl.in.p, sl.h_in, na, hipMemcpyHostToDevice, ctx->copy));
    if (nb) BBP_HIP_TRY(ctx, hipMemcpyAsync((uint8_t*)sl.ent.p + ent_off, (uint8_t*)sl.h_in + na, nb, hipMemcpyHostToDevice, ctx->copy));
    BBP_HIP_TRY(ctx, hipEventRecord(sl.ev_in, ctx->copy));
    BBP_HIP_TRY(ctx, wait_event_polling(sl.ev_in));
    return BBP_OK;
}
// Second half of a host-pointer call, context lock NOT held: wait for the slot's compute to finish, THEN copy the results down.
// The copy is issued only now, on the copy stream, on purpose: a D2H copy enqueued behind the kernels would sit at the head of a
// DMA engine's in-order queue waiting for them, and the NEXT call's input copy -- which that call's opening stage is waiting for
// -- would queue up behind it (measured: the input copy "took" 87 ms, i.e. the previous batch's whole MSM stage; two host
// threads got no overlap at all).  Issued after the wait, either copy takes ~0.2 ms whatever the compute queues are doing.
static int32_t fetch_results(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, size_t bytes) {
    hipError_t e = hipSetDevice(ctx->device);  // the lock is not held here and nothing has set this thread's device yet (pool workers)
    if (e == hipSuccess) e = wait_event_polling(sl.ev);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_out, sl.out.p, bytes, hipMemcpyDeviceToHost, ctx->copy);
    // ... and the context's health word with them: a call whose kernels (or any earlier call's) had to clamp a table gather reports
    // BBP_ERR_DEVICE for the whole call instead of handing out results computed from corrupted scratch with status 0
    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_flag, ctx->health, sizeof(u32), hipMemcpyDeviceToHost, ctx->copy);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_in, ctx->copy);
    if (e == hipSuccess) e = wait_event_polling(sl.ev_in);
    if (e != hipSuccess) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string("collecting results: ") + hipGetErrorString(e), BBP_ERR_DEVICE; });
        return BBP_ERR_DEVICE;
    }
    if (*sl.h_flag) {
        const u32 flags = *sl.h_flag;
        api_guard(ctx, [&]() -> int32_t {
            char buf[200];
            snprintf(buf, sizeof buf, "engine health flags %#x: %s; results since then are not trustworthy -- free this context and create a new one", flags,
                     (flags & 1u) ? "an MSM table gather was out of range and had to be clamped (corrupted engine scratch)"
                                  : "a proof with a satisfied witness failed its check twice (checked proving)");
            return ctx->err = buf, BBP_ERR_DEVICE;
        });
        return BBP_ERR_DEVICE;
    }
    return BBP_OK;
}
}  // namespace bbp

static int32_t no_os_random(bbp_ctx* ctx) {
    api_guard(ctx, [&]() -> int32_t { return ctx->err = "cannot read /dev/urandom", BBP_ERR_DEVICE; });
    return BBP_ERR_DEVICE;
}

// key of a host-pointer call that draws on the device: the armed test key (bbp_debug_next_entropy_key), else 32 OS bytes
static int32_t next_device_key(bbp_ctx* ctx, ChachaKey* key) {
    uint8_t k[32];
    bool armed = false;
    api_guard(ctx, [&]() -> int32_t {
        if ((armed = ctx->debug_key_armed)) memcpy(k, ctx->debug_key, 32);
        ctx->debug_key_armed = false;
        return BBP_OK;
    });
    if (!armed && !os_random(k, sizeof k)) return no_os_random(ctx);
    *key = chacha_key_from_bytes(k);
    if (wipe_on(ctx)) secure_zero(k, sizeof k);
    return BBP_OK;
}

// bbp_debug_corrupt_next_proof: the armed record index, relative to this launch's first proof, is corrupted on `s` right after the
// prover wrote it (before any check reads it); the hook fires once
static int32_t corrupt_hook(bbp_ctx* ctx, u32 first, u32 nb, u32 N, u8* out_dev, hipStream_t s) {
    const int64_t i = ctx->debug_corrupt_proof - (int64_t)first;
    if (ctx->debug_corrupt_proof < 0 || i < 0 || i >= (int64_t)nb) return BBP_OK;
    ctx->debug_corrupt_proof = -1;
    hipLaunchKernelGGL(k_corrupt_tx, dim3(1), dim3(64), 0, s, out_dev + (size_t)bbp_proof_record_size(N) * (size_t)i);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

// One checked prove launch (context lock held): witness check on the opening stream, the prover, the verify rows and the aggregated
// verifier on a verifier lane's stream -- forked from the records' completion on `s`, joined back before the status merge on `s`.
// Everything this call writes is complete for work enqueued on `s` afterwards.  `scratch` holds CheckRing(B, N).scratch_bytes;
// `reuse` (optional) is the event after which `scratch` and `mask` may be overwritten; `draw` (optional) writes `ent` on the opening stream.
static int32_t prove_checked_enqueue(bbp_ctx* ctx, u32 B, u32 N, const u8* in, const u8* ent, const u8* cent, u8* out, int32_t* status,
                                     u32* mask, u8* scratch, u32* fail_n, u32* fail_idx, u32 idx_base, hipStream_t s, hipEvent_t reuse,
                                     const std::function<int32_t(hipStream_t)>* draw = nullptr) {
    int32_t rc;
    if (!ctx->chk_counts) {
        BBP_HIP_TRY(ctx, hipMalloc(&ctx->chk_counts, 2 * sizeof(unsigned long long)));
        BBP_HIP_TRY(ctx, hipMemsetAsync(ctx->chk_counts, 0, 2 * sizeof(unsigned long long), s));
    }
    if (!ctx->ev_chk_fork) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_chk_fork, hipEventDisableTiming));
    if (!ctx->ev_chk_join) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_chk_join, hipEventDisableTiming));
    u32 hog = 0;  // a serial wave of four MiMC chains beside other calls' heavy stages: fenced onto CUs of its own, as k_prepare_bids
    if ((rc = serial_lds_bytes(ctx, (const void*)k_witness_check, &hog))) return rc;
    const std::function<int32_t(hipStream_t)> open_hook = [&](hipStream_t os) -> int32_t {
        if (reuse) BBP_HIP_TRY(ctx, hipStreamWaitEvent(os, reuse, 0));
        if (draw) {  // the call's entropy, drawn on the device before the opening stage reads it
            const int32_t rc = (*draw)(os);
            if (rc) return rc;
        }
        ScopedEvent ev(ctx, TAG_WITNESS, os);
        hipLaunchKernelGGL(k_witness_check, dim3((B + 63) / 64), dim3(64), hog, os, B, N, in, ctx->mimc_c, mask);
        BBP_HIP_TRY(ctx, hipGetLastError());
        return BBP_OK;
    };
    if ((rc = prove_batch_dev(ctx, B, N, in, ent, out, s, &open_hook))) return rc;
    if ((rc = corrupt_hook(ctx, 0, B, N, out, s))) return rc;
    bbp_ctx::VLane& L = ctx->vl[ctx->chk_lane++ % (u32)bbp_ctx::VLANES];
    u8* rows = scratch;
    int32_t* vstatus = reinterpret_cast<int32_t*>(scratch + CheckRing(B, N).vstatus);
    BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_chk_fork, s));
    BBP_HIP_TRY(ctx, hipStreamWaitEvent(L.stream, ctx->ev_chk_fork, 0));
    if (reuse) BBP_HIP_TRY(ctx, hipStreamWaitEvent(L.stream, reuse, 0));
    {
        ScopedEvent ev(ctx, TAG_VERIFY_SCALARS, L.stream);
        const size_t n = verify_row_bytes(N) * B;
        hipLaunchKernelGGL(k_check_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.stream, B, N, in, (const u8*)out, rows);
        BBP_HIP_TRY(ctx, hipGetLastError());
    }
    const int last_par = ctx->last_par;  // (the verifier takes it over; bbp_debug_challenges means the prove call)
    rc = verify_batch_agg_dev(ctx, VerifyRows::uniform(B, N), BBP_AGG_GROUP_DEFAULT, rows, cent, vstatus, L.stream, nullptr);
    ctx->last_par = last_par;
    if (rc) return rc;
    BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_chk_join, L.stream));
    BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_chk_join, 0));
    {
        ScopedEvent ev(ctx, TAG_VERIFY_SCALARS, s);
        hipLaunchKernelGGL(k_check_merge, dim3((B + 63) / 64), dim3(64), 0, s, B, N, (const u32*)mask, (const int32_t*)vstatus, out, status,
                           ctx->chk_counts, fail_n, fail_idx, idx_base);
        BBP_HIP_TRY(ctx, hipGetLastError());
    }
    return BBP_OK;
}

// a proof with a satisfied witness failed its check twice: health bit 1, sticky like bit 0 (every later host-pointer call fails)
static int32_t raise_check_failure(bbp_ctx* ctx, u32 row) {
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipLaunchKernelGGL(k_health_or, dim3(1), dim3(64), 0, ctx->stream, ctx->health, 2u);
        BBP_HIP_TRY(ctx, hipGetLastError());
        BBP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->err = "checked proving: the record of row " + std::to_string(row) +
                   " (a satisfied witness) failed verification twice -- health bit 1; free this context and create a new one";
        return BBP_ERR_DEVICE;
    });
}

// last-error text of a row the witness check refused (host evaluation of the same relations: failure paths only)
static std::string refused_row_text(const bbp_ctx* ctx, const uint8_t* row, uint32_t N) {
    const bbp_ctx* c = is_pool(ctx) ? ctx->members[0] : ctx;
    std::vector<sc> mc(BBP_MIMC_ROUNDS);
    if (c->mimc_host.size() < sizeof(sc) * BBP_MIMC_ROUNDS) return "toggle >= N";
    memcpy(mc.data(), c->mimc_host.data(), sizeof(sc) * BBP_MIMC_ROUNDS);
    std::vector<u32> w(prove_in_words(N));
    memcpy(w.data(), row, 4 * w.size());
    return witness_check_text(witness_check_row(N, w.data(), mc.data()));
}

enum CheckMode { CHECK_AUTO, CHECK_OFF, CHECK_REPROVE };  // context's setting / never (bbp_reserve) / checked, no second prove

// The other input of prove_batch_host (bbp_prove_round): the round's table and the raw bids in host memory instead of expanded
// rows.  They are uploaded as they are and the device pass (round_bids.h) writes the prover's rows into the staging slot; its
// per-bid statuses stand in for the host screening, and `out` receives rows record || score || z_img.
struct RoundInput {
    const uint8_t* table;   // seed || pub_list
    const uint8_t* bids;    // B x (d || k)
    uint64_t* toggles_out;  // B entries, or NULL
};

// One host-pointer prove call on its way through the steps below: the arguments, where things lie in its staging slot
// (prove_io.h), the entropy decision, and what came back.
struct ProveCall {
    bbp_ctx* ctx;
    uint32_t B, N;
    const uint8_t* in;  // NULL for a round call
    const uint8_t* entropy;
    uint8_t* out;
    int32_t* status;
    CheckMode mode;
    const RoundInput* round;
    ProveStaging L;
    // screening: what is uploaded into the slot's `in` -- the rows (with stand-ins for refused ones), or bids and table
    std::vector<uint8_t> fixed;
    const uint8_t *src = nullptr, *src2 = nullptr;
    // entropy: the prover's rows in host memory (NULL: drawn on the device under `key`) and the one span that is uploaded
    ChachaKey key{};
    std::vector<uint8_t> ent_host, ent_all;
    const uint8_t* up_ent = nullptr;
    // the check's verdicts as read back
    std::vector<int32_t> dstatus;
    std::vector<u32> dmask, fail_rows;
    std::vector<uint8_t> fail_keys;  // hedged round call: the row keys of fail_rows, in that order (as read back)
    double t_lock = 0, t_h2d = 0;  // BBP_TRACE
};

// Step 1: host-side argument screening (the reference's typed API cannot express these states: SURVEY.md 8b).  A refused row is
// replaced by a neutral stand-in so the batch geometry is unchanged.  A round call's rows are screened by the device pass.
static void prove_screen(ProveCall& c) {
    const size_t in_stride = c.L.in_stride;
    for (uint32_t i = 0; i < c.B; i++) c.status[i] = BBP_OK;
    if (c.round) {
        c.src = c.round->bids, c.src2 = c.round->table;
        return;
    }
    for (uint32_t i = 0; i < c.B; i++) {
        const uint8_t* r = c.in + in_stride * i;
        uint64_t toggle;
        memcpy(&toggle, r + prove_in_toggle(c.N), 8);
        if (toggle >= c.N) c.status[i] = BBP_ERR_BAD_ARG;
        for (int k = 0; k < 7 && c.status[i] == BBP_OK; k++) {
            u32 w[8];
            memcpy(w, r + 32 * k, 32);
            if (!sc_is_canonical(w)) c.status[i] = BBP_ERR_FORMAT;  // serde Scalar deserialisation is canonical-only
        }
        if (c.status[i] != BBP_OK) {
            if (c.fixed.empty()) c.fixed.assign(c.in, c.in + in_stride * c.B);
            memset(&c.fixed[in_stride * i], 0, in_stride);
        }
    }
    c.src = c.fixed.empty() ? c.in : c.fixed.data();
}

// Step 2: the call's entropy -- the caller's, the OS's, or (source DEVICE) one key for the call, each chunk's rows drawn on its
// opening stream (k_draw_entropy): only the key leaves the OS.  Checked: the verifier's weights come from the OS like
// bbp_verify_batch's; they travel behind the prover's entropy.  The result is the one span up_ent that is uploaded.
static int32_t prove_entropy(ProveCall& c) {
    const uint32_t B = c.B, m = 4 + c.N;
    const size_t ent_stride = c.L.ent_stride;
    if (c.L.dev_draw) {
        if (int32_t rc = next_device_key(c.ctx, &c.key)) return rc;
    } else if (!c.entropy) {
        // thread_rng replacement: 64 OS bytes per blinding, wide-reduced like Scalar::random; 32 OS bytes for the rng seed
        std::vector<uint8_t> raw((size_t)B * (64 * m + 32));
        if (!os_random(raw.data(), raw.size())) return no_os_random(c.ctx);
        c.ent_host.resize(ent_stride * B);
        for (uint32_t i = 0; i < B; i++) {
            const uint8_t* rp = &raw[(size_t)i * (64 * m + 32)];
            for (uint32_t k = 0; k < m; k++) {
                u32 w[16];
                memcpy(w, rp + 64 * k, 64);
                sc s = sc_from_wide(w);
                sc_tobytes(&c.ent_host[ent_stride * i + 32 * k], s);
                if (wipe_on(c.ctx)) secure_zero(w, sizeof w), secure_zero(&s, sizeof s);
            }
            memcpy(&c.ent_host[ent_stride * i + 32 * m], rp + 64 * m, 32);
        }
        if (wipe_on(c.ctx)) secure_zero_vec(raw);
        c.entropy = c.ent_host.data();
    }
    c.up_ent = c.entropy;
    if (c.L.check) {
        const size_t own = c.L.ent_up_bytes - 32 * (size_t)B;  // the prover's rows, unless they are drawn
        c.ent_all.resize(c.L.ent_up_bytes);
        if (own) memcpy(c.ent_all.data(), c.entropy, own);
        if (!os_random(c.ent_all.data() + own, 32 * (size_t)B)) return no_os_random(c.ctx);
        c.up_ent = c.ent_all.data();
    }
    return BBP_OK;
}

// every buffer of a staging slot at what the layout says (the enqueue step; bbp_reserve, ahead of time)
static int32_t staging_reserve(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const ProveStaging& L) {
    int32_t rc;
    if ((rc = dev_reserve(ctx, sl.out, L.out_cap)) || (rc = pinned_reserve(ctx, sl.h_out, sl.h_cap, L.h_out_bytes)) ||
        (L.check && (rc = dev_reserve(ctx, sl.chk, L.chk_bytes))) || (rc = dev_reserve(ctx, sl.in, L.in_cap)) ||
        (rc = dev_reserve(ctx, sl.ent, L.ent_cap)))
        return rc;
    return pinned_reserve(ctx, sl.h_in, sl.h_in_cap, L.h_in_bytes);
}

// Step 3, under the context lock: reserve, upload, the chunk loop, a round call's output rows, the slot's event.
static int32_t prove_enqueue(ProveCall& c, bbp_ctx::IoSlot& sl) {
    bbp_ctx* const ctx = c.ctx;
    const ProveStaging& L = c.L;
    const uint32_t B = c.B, N = c.N;
    int32_t rc;
    BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // a round call's bids and table travel as they are; the slot's input buffer also holds the pass's scratch and the rows it writes
    if ((rc = staging_reserve(ctx, sl, L)) ||
        (rc = upload_inputs(ctx, sl, c.src, L.in_first_bytes, c.up_ent, L.ent_up_bytes, L.ent_up_off, c.src2, L.in_tab_bytes, L.in_tab)))
        return rc;
    if (L.round && !ctx->ev_round) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_round, hipEventDisableTiming));
    c.t_h2d = now_ms();
    u8 *const d_in = (u8*)sl.in.p, *const d_ent = (u8*)sl.ent.p, *const d_out = (u8*)sl.out.p;
    int32_t* st_dev = (int32_t*)(d_out + L.out_status);
    u32 *mask_dev = (u32*)(d_out + L.out_mask), *fail_n = (u32*)(d_out + L.out_fail_n), *fail_idx = (u32*)(d_out + L.out_fail_idx);
    if (L.check) BBP_HIP_TRY(ctx, hipMemsetAsync(fail_n, 0, sizeof(u32), ctx->stream));
    // Very large host batches go through the engine in equal chunks of at most host_chunk_prove proofs so that scratch stays
    // bounded (~1.3 MB per proof of the largest call, three buffers); consecutive calls pipeline -- chunk k+1's opening stage
    // under chunk k's MSMs.  One 16384-proof call was measured 5 % faster than four of 4096, hence the large default.
    const uint32_t n_chunks = (B + host_chunk_prove() - 1) / host_chunk_prove(), chunk = (B + n_chunks - 1) / n_chunks;
    for (uint32_t first = 0; first < B; first += chunk) {
        const uint32_t nb = B - first < chunk ? B - first : chunk;
        const u8 *cin = d_in + L.in_rows + L.in_stride * first, *cent = d_ent + L.ent_stride * first;
        u8* cout = d_out + L.out_recs + L.rec * first;
        // what runs on the chunk's opening stream ahead of the opening stage.  A round call: the device pass writes this chunk's
        // rows (the table is reduced by the first chunk; a later chunk may open on the other stream and waits for that).
        // (source DEVICE / HEDGED) this chunk's own rows of the call's key: no two chunks draw equal rows
        const std::function<int32_t(hipStream_t)> draw = [&](hipStream_t os) -> int32_t {
            if (L.round) {
                int32_t rc;
                if (first) BBP_HIP_TRY(ctx, hipStreamWaitEvent(os, ctx->ev_round, 0));
                if ((rc = round_prepare_enqueue(ctx, N, d_in + L.in_tab, d_in + L.in_scratch, L.rs, first == 0, first, nb,
                                                d_in + ROUND_BID_BYTES * first, (u32*)cin, nullptr, (u32*)(d_out + L.out_tog) + 2 * (size_t)first,
                                                (int32_t*)(d_out + L.out_pass_st) + first, os)))
                    return rc;
                if (!first && n_chunks > 1) BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_round, os));
            }
            if (L.hedged)  // the rows are complete on os (uploaded, or just written by the pass above): row keys, then the draw under them
                return hedged_draw_enqueue(ctx, nb, N, c.key, first, cin, d_ent + L.ent_keys + 32 * (size_t)first, (void*)cent, os);
            return L.dev_draw ? draw_enqueue(ctx, nb, N, BBP_ENTROPY_PROVE, c.key, first, (void*)cent, os) : (int32_t)BBP_OK;
        };
        const std::function<int32_t(hipStream_t)>* open = L.dev_draw || L.round ? &draw : nullptr;
        if (L.check) {
            u8* scratch = (u8*)sl.chk.p;  // chunks are stream-ordered on ctx->stream; each chunk's check joins back before the next starts
            if ((rc = prove_checked_enqueue(ctx, nb, N, cin, cent, d_ent + L.ent_check(first), cout, st_dev + first, mask_dev + first, scratch,
                                            fail_n, fail_idx, first, ctx->stream, nullptr, open)))
                return rc;
        } else {
            if ((rc = prove_batch_dev(ctx, nb, N, cin, cent, cout, ctx->stream, open))) return rc;
            if ((rc = corrupt_hook(ctx, first, nb, N, cout, ctx->stream))) return rc;
        }
    }
    if (L.round && (rc = round_rows_enqueue(ctx, B, N, d_out + L.out_recs, (const u32*)(d_in + L.in_scratch + L.rs.rb), d_out, ctx->stream))) return rc;
    ctx->debug_corrupt_proof = -1;  // armed for an index beyond this call: consumed all the same
    BBP_HIP_TRY(ctx, hipEventRecord(sl.ev, ctx->stream));
    return BBP_OK;
}

// Step 4, lock released (another thread may be enqueueing the next batch now): the results out of the slot's pinned mirror.  A
// round call: the device pass's verdicts stand where the host screening's would.  Checked: the info block behind the records --
// statuses, witness masks, the count and the rows of rejected records (k_check_merge).
static int32_t prove_collect(ProveCall& c, bbp_ctx::IoSlot& sl) {
    const ProveStaging& L = c.L;
    const size_t b = c.B;
    if (int32_t rc = fetch_results(c.ctx, sl, L.out_fetch)) return rc;
    const u8* h = (const u8*)sl.h_out;
    memcpy(c.out, h, L.res_stride * b);
    if (L.round) {
        memcpy(c.status, h + L.out_pass_st, 4 * b);
        if (c.round->toggles_out) memcpy(c.round->toggles_out, h + L.out_tog, 8 * b);
    }
    if (L.check) {
        c.dstatus.resize(b);
        c.dmask.resize(b);
        memcpy(c.dstatus.data(), h + L.out_status, 4 * b);
        memcpy(c.dmask.data(), h + L.out_mask, 4 * b);
        u32 n_fail = 0;
        memcpy(&n_fail, h + L.out_fail_n, 4);
        c.fail_rows.resize(std::min<u32>(n_fail, c.B));
        memcpy(c.fail_rows.data(), h + L.out_fail_idx, 4 * c.fail_rows.size());
        // hedged round call: the expanded rows exist on the device only, so the failed rows' keys are fetched (failure path only; the
        // slot is still this call's, and everything that wrote the keys finished before sl.ev)
        if (L.hedged && L.round && !c.fail_rows.empty() && c.mode != CHECK_REPROVE) {
            c.fail_keys.resize(32 * c.fail_rows.size());
            hipError_t e = hipSuccess;
            for (size_t j = 0; j < c.fail_rows.size() && e == hipSuccess; j++)
                e = hipMemcpyAsync(&c.fail_keys[32 * j], (const u8*)sl.ent.p + L.ent_keys + 32 * (size_t)c.fail_rows[j], 32, hipMemcpyDeviceToHost, c.ctx->copy);
            if (e == hipSuccess) e = hipEventRecord(sl.ev_in, c.ctx->copy);
            if (e == hipSuccess) e = wait_event_polling(sl.ev_in);
            if (e != hipSuccess) {
                api_guard(c.ctx, [&]() -> int32_t { return c.ctx->err = std::string("collecting row keys: ") + hipGetErrorString(e), BBP_ERR_DEVICE; });
                return BBP_ERR_DEVICE;
            }
        }
    }
    return BBP_OK;
}

static int32_t prove_batch_host(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out,
                                int32_t* status, CheckMode mode = CHECK_AUTO, const RoundInput* round = nullptr);

// Secret wiping, the staging slot of a host-pointer prove call: after its last reader -- the results are in the caller's memory and a
// hedged round call's failed row keys have been fetched (prove_collect); a second prove of failed rows takes a slot of its own and
// wipes that.  One launch on the copy stream for the three device buffers, waited for; then the pinned mirrors, on the host.
// enqueued == false (the enqueue step failed half-way, streams may still read the slot): this slot and whatever the call reserved and
// did not wipe, behind a device synchronise (wipe_failed_call); other calls' slots are left to them.
static int32_t slot_wipe(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const ProveStaging& L, bool enqueued) {
    int32_t rc = api_guard(ctx, [&]() -> int32_t {  // the lock for the enqueue only, as everywhere on the host path
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (!enqueued) return wipe_failed_call(ctx, sl);
        WipeList wl;
        wipe_take(wl, sl.in);
        wipe_take(wl, sl.ent);
        wipe_take(wl, sl.out);
        if (int32_t rc = wipe_enqueue(ctx, wl, ctx->copy)) return rc;
        BBP_HIP_TRY(ctx, hipEventRecord(sl.ev_in, ctx->copy));
        return BBP_OK;
    });
    if (rc || !enqueued) return rc;
    // the wait with the lock released (the copy stream may be queued behind another thread's upload); the slot is still this call's
    const hipError_t e = wait_event_polling(sl.ev_in);
    if (sl.h_in) secure_zero(sl.h_in, std::min(sl.h_in_cap, L.h_in_bytes));
    if (sl.h_out) secure_zero(sl.h_out, std::min(sl.h_cap, L.h_out_bytes));
    if (e != hipSuccess) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string("secret wipe of a staging slot: ") + hipGetErrorString(e), BBP_ERR_DEVICE; });
        return BBP_ERR_DEVICE;
    }
    return BBP_OK;
}
// ... and the call's own host copies (stand-in rows, drawn entropy, the call key, fetched row keys), on every way out
struct ProveCallWipe {
    ProveCall& c;
    ~ProveCallWipe() {
        if (!wipe_on(c.ctx)) return;
        secure_zero_vec(c.fixed), secure_zero_vec(c.ent_host), secure_zero_vec(c.ent_all), secure_zero_vec(c.fail_keys);
        secure_zero(&c.key, sizeof c.key);
    }
};

// Step 5 (checked calls): rows the screening let through take the device's verdict (their records are already zeroed unless OK),
// and a record that failed its check is proved once more with the same inputs and the same entropy (the drawn entropy when the
// caller gave none; source DEVICE: the row re-derived from the call's key), and checked again; a second failure is a device
// fault: the whole call fails and health bit 1 is raised.  Runs without a staging slot: the second prove takes one of its own.
static int32_t prove_merge(ProveCall& c) {
    bbp_ctx* const ctx = c.ctx;
    const ProveStaging& L = c.L;
    if (c.mode == CHECK_AUTO) ctx->chk_checked += c.B;
    int64_t first_refused = -1;
    for (uint32_t i = 0; i < c.B; i++) {
        if (c.status[i] != BBP_OK) continue;
        c.status[i] = c.dstatus[i];
        if (c.dstatus[i] != BBP_OK && c.dstatus[i] != BBP_ERR_VERIFY && first_refused < 0) first_refused = i;
    }
    if (first_refused >= 0) set_tls_error(ctx, std::string("row ") + std::to_string(first_refused) + ": " + witness_check_text(c.dmask[first_refused]));
    if (c.mode == CHECK_REPROVE || c.fail_rows.empty()) return BBP_OK;
    if (!c.fail_keys.empty()) {  // keys travel with their rows through the sort
        std::vector<std::pair<u32, size_t>> order(c.fail_rows.size());
        for (size_t j = 0; j < order.size(); j++) order[j] = {c.fail_rows[j], j};
        std::sort(order.begin(), order.end());
        std::vector<uint8_t> keys(c.fail_keys.size());
        for (size_t j = 0; j < order.size(); j++) memcpy(&keys[32 * j], &c.fail_keys[32 * order[j].second], 32);
        c.fail_keys.swap(keys);
        if (wipe_on(ctx)) secure_zero_vec(keys);  // the unsorted copy
    }
    std::sort(c.fail_rows.begin(), c.fail_rows.end());
    const uint32_t nr = (uint32_t)c.fail_rows.size();
    const size_t rin_stride = L.in_first_stride;  // a round call proves the failed bids again, as a round
    std::vector<uint8_t> rin(rin_stride * nr), rent(L.ent_stride * nr), rout(L.res_stride * nr);
    std::vector<int32_t> rst(nr);
    for (uint32_t j = 0; j < nr; j++) {
        memcpy(&rin[rin_stride * j], c.src + rin_stride * c.fail_rows[j], rin_stride);
        if (L.hedged) {  // the row's own key: a rows call re-derives it from the row as uploaded, a round call fetched it (prove_collect)
            ChachaKey rk = L.round ? chacha_key_from_bytes(&c.fail_keys[32 * j]) : hedge_row_key_bytes(c.key, c.N, c.src + L.in_stride * c.fail_rows[j]);
            hedge_prove_row_bytes(rk, c.N, c.fail_rows[j], &rent[L.ent_stride * j]);
            if (wipe_on(ctx)) secure_zero(&rk, sizeof rk);
        } else if (L.dev_draw)
            entropy_prove_row_bytes(c.key, c.N, c.fail_rows[j], &rent[L.ent_stride * j]);
        else
            memcpy(&rent[L.ent_stride * j], c.entropy + L.ent_stride * c.fail_rows[j], L.ent_stride);
    }
    ctx->chk_reproved += nr;
    const RoundInput again{c.src2, rin.data(), nullptr};
    const int32_t rc2 = prove_batch_host(ctx, nr, c.N, L.round ? nullptr : rin.data(), rent.data(), rout.data(), rst.data(), CHECK_REPROVE, L.round ? &again : nullptr);
    if (wipe_on(ctx)) secure_zero_vec(rin), secure_zero_vec(rent);  // the failed rows and their re-derived entropy
    if (rc2) return rc2;
    for (uint32_t j = 0; j < nr; j++) {
        if (rst[j] != BBP_OK) return raise_check_failure(ctx, c.fail_rows[j]);
        memcpy(c.out + L.res_stride * c.fail_rows[j], &rout[L.res_stride * j], L.res_stride);
        c.status[c.fail_rows[j]] = BBP_OK;
    }
    return BBP_OK;
}

// body of bbp_prove_batch and, with `round`, of bbp_prove_round (in == NULL then); the combiner's runner and bbp_reserve's warm-up
// call it too.  Takes the context lock itself, for the enqueue step only.
static int32_t prove_batch_host(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out, int32_t* status,
                                CheckMode mode, const RoundInput* round) {
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc) return rc;
    if (B == 0) return BBP_OK;
    fault_injected("prove_batch");
    const bool check = mode == CHECK_REPROVE || (mode == CHECK_AUTO && ctx->prove_check.load());
    const int source = ctx->entropy_source.load();
    const bool hedged = !entropy && source == BBP_ENTROPY_SOURCE_HEDGED, dev_draw = hedged || (!entropy && source == BBP_ENTROPY_SOURCE_DEVICE);
    ProveCall c{ctx, B, N, in, entropy, out, status, mode, round, ProveStaging(B, N, round != nullptr, check, dev_draw, hedged)};
    const ProveCallWipe host_wipe{c};
    prove_screen(c);
    if ((rc = prove_entropy(c))) return rc;
    static const bool trace = getenv("BBP_TRACE") != nullptr;
    const double t_enter = now_ms();
    {  // the staging slot is held for this block only: a second prove of rejected rows (prove_merge) takes a slot of its own
        SlotLease lease(ctx);  // may wait for the call two back to collect its results; the context lock is NOT held here
        bbp_ctx::IoSlot& sl = *lease.sl;
        const double t_slot = now_ms();
        if ((rc = api_guard(ctx, [&]() -> int32_t { return c.t_lock = now_ms(), prove_enqueue(c, sl); }))) {
            if (wipe_on(ctx)) (void)slot_wipe(ctx, sl, c.L, false);
            return rc;
        }
        const double t_enq = now_ms();
        rc = prove_collect(c, sl);
        if (wipe_on(ctx)) {
            const int32_t wrc = slot_wipe(ctx, sl, c.L, true);
            if (rc == BBP_OK) rc = wrc;
        }
        if (rc) return rc;
        if (trace)
            fprintf(stderr, "[bbp trace] prove_batch B=%u slot=%d: enter %.1f, slot +%.1f, lock +%.1f, h2d +%.1f, enqueued +%.1f, done +%.1f\n", B,
                    (int)(&sl - ctx->io), t_enter, t_slot - t_enter, c.t_lock - t_enter, c.t_h2d - t_enter, t_enq - t_enter, now_ms() - t_enter);
    }
    for (uint32_t i = 0; i < B; i++)
        if (status[i] != BBP_OK) memset(out + c.L.res_stride * i, 0, c.L.res_stride);
    return check ? prove_merge(c) : (int32_t)BBP_OK;
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

extern "C" int32_t bbp_prove_batch(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out,
                                   int32_t* status) {
    if (!ctx || !in || !out || !status) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) {  // block split over the members, records in request order (pool.cpp)
        const int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
        if (rc || B == 0) return rc;
        return no_throw_ctx(ctx, [&]() -> int32_t { return pool_prove_batch(ctx, B, N, in, entropy, out, status); });
    }
    return no_throw_ctx(ctx, [&]() -> int32_t { return prove_batch_host(ctx, B, N, in, entropy, out, status); });
}

extern "C" int32_t bbp_prove_batch_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev, void* out_dev,
                                       void* stream) {
    if (!ctx || !in_dev || !entropy_dev || !out_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_prove_batch_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc = check_n(ctx, N);
        if (rc) return rc;
        if (B == 0) return BBP_OK;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        if ((rc = prove_batch_dev(ctx, B, N, (const u8*)in_dev, (const u8*)entropy_dev, (u8*)out_dev, s))) return rc;
        rc = corrupt_hook(ctx, 0, B, N, (u8*)out_dev, s);
        ctx->debug_corrupt_proof = -1;
        return rc;
    });
}

extern "C" int32_t bbp_prove_batch_checked_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const void* in_dev, const void* entropy_dev,
                                               const void* check_entropy_dev, void* out_dev, void* status_dev, void* stream) {
    if (!ctx || !in_dev || !entropy_dev || !check_entropy_dev || !out_dev || !status_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_prove_batch_checked_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc = check_n(ctx, N);
        if (rc) return rc;
        if (B == 0) return BBP_OK;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        // scratch in rotation: verify rows + verifier statuses, then the witness masks; a ring entry waits for the status kernel of
        // the call that used it last (several calls in flight, no host synchronisation)
        bbp_ctx::CheckBuf& cb = ctx->chk[ctx->chk_next++ % (u32)bbp_ctx::CHECK_RING];
        const CheckRing ring(B, N);
        if ((rc = dev_reserve(ctx, cb.buf, ring.bytes))) return rc;
        if (!cb.ev) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&cb.ev, hipEventDisableTiming));
        u8* base = (u8*)cb.buf.p;
        rc = prove_checked_enqueue(ctx, B, N, (const u8*)in_dev, (const u8*)entropy_dev, (const u8*)check_entropy_dev, (u8*)out_dev,
                                   (int32_t*)status_dev, (u32*)(base + ring.mask), base, nullptr, nullptr, 0, s, cb.ev_valid ? cb.ev : nullptr);
        ctx->debug_corrupt_proof = -1;
        if (rc) return rc;
        BBP_HIP_TRY(ctx, hipEventRecord(cb.ev, s));
        cb.ev_valid = true;
        ctx->chk_checked += B;
        return BBP_OK;
    });
}

// ---- proving a round from raw bids (include/bbp.h; the device pass is round_bids.h) -----------------------------------------------
extern "C" int32_t bbp_prove_round(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* bids, const uint8_t* entropy,
                                   uint8_t* rows_out, uint64_t* toggles_out, int32_t* status) {
    if (!ctx || !round || !bids || !rows_out || !status) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) {  // bids block-split over the members, every member receives the table (pool.cpp)
        const int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
        if (rc || B == 0) return rc;
        return no_throw_ctx(ctx, [&]() -> int32_t { return pool_prove_round(ctx, N, round, B, bids, entropy, rows_out, toggles_out, status); });
    }
    const RoundInput r{round, bids, toggles_out};
    return no_throw_ctx(ctx, [&]() -> int32_t { return prove_batch_host(ctx, B, N, nullptr, entropy, rows_out, status, CHECK_AUTO, &r); });
}

// Both _dev forms (context lock held).  entropy_dev == NULL: the pass alone, rows into prove_in.  Else the pass into the ring entry,
// the prover, and the output rows into rows_out, all ordered on s; the prover's opening stage waits for the pass through ev_prep.
static int32_t round_dev_enqueue(bbp_ctx* ctx, u32 N, const u8* table, u32 B, const u8* bids, u32* prove_in, u32* tails, u32* toggles,
                                 int32_t* status, const u8* entropy_dev, u8* rows_out, hipStream_t s) {
    int32_t rc;
    const bool prove = entropy_dev != nullptr;
    const RoundRing ring(B, N, prove);
    const RoundScratch& rs = ring.rs;
    // scratch in rotation: an entry waits for the last kernel of the call that used it last (several calls in flight, no host synchronisation)
    bbp_ctx::CheckBuf& cb = ctx->rnd[ctx->rnd_next++ % (u32)bbp_ctx::CHECK_RING];
    if ((rc = dev_reserve(ctx, cb.buf, ring.bytes))) return rc;
    if (!cb.ev) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&cb.ev, hipEventDisableTiming));
    if (cb.ev_valid) BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, cb.ev, 0));
    u8* base = (u8*)cb.buf.p;
    u8 *in_rows = base + ring.rows, *recs = base + ring.recs;
    if (prove) prove_in = (u32*)in_rows;
    if ((rc = round_prepare_enqueue(ctx, N, table, base, rs, true, 0, B, bids, prove_in, tails, toggles, status, s))) return rc;
    // the prover's opening stage does not wait for the caller's stream (bbp.h); it does wait for this event
    BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_prep, s));
    ctx->ev_prep_valid = true;
    if (prove) {
        if ((rc = prove_batch_dev(ctx, B, N, in_rows, entropy_dev, recs, s))) return rc;
        rc = corrupt_hook(ctx, 0, B, N, recs, s);
        ctx->debug_corrupt_proof = -1;
        if (rc || (rc = round_rows_enqueue(ctx, B, N, recs, (const u32*)(base + rs.rb), rows_out, s))) return rc;
    }
    if (wipe_on(ctx)) {  // secret wiping: the ring entry (bids' results, expanded rows), ahead of its event -- the entry's reuse rule covers the wipe
        WipeList wl;
        wipe_take(wl, cb.buf);
        if ((rc = wipe_enqueue(ctx, wl, s))) return rc;
    }
    BBP_HIP_TRY(ctx, hipEventRecord(cb.ev, s));
    cb.ev_valid = true;
    return BBP_OK;
}

extern "C" int32_t bbp_prepare_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, void* prove_in_dev,
                                         void* tails_dev, void* toggles_dev, void* status_dev, void* stream) {
    if (!ctx || !round_dev || !bids_dev || !prove_in_dev || !status_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_prepare_round_dev");
    return api_guard(ctx, [&]() -> int32_t {
        const int32_t rc = check_n(ctx, N);
        if (rc || B == 0) return rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        return round_dev_enqueue(ctx, N, (const u8*)round_dev, B, (const u8*)bids_dev, (u32*)prove_in_dev, (u32*)tails_dev, (u32*)toggles_dev,
                                 (int32_t*)status_dev, nullptr, nullptr, pick_stream(ctx, stream));
    });
}

extern "C" int32_t bbp_prove_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, const void* entropy_dev,
                                       void* rows_out_dev, void* toggles_out_dev, void* status_dev, void* stream) {
    if (!ctx || !round_dev || !bids_dev || !entropy_dev || !rows_out_dev || !status_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_prove_round_dev");
    return api_guard(ctx, [&]() -> int32_t {
        const int32_t rc = check_n(ctx, N);
        if (rc || B == 0) return rc;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        return round_dev_enqueue(ctx, N, (const u8*)round_dev, B, (const u8*)bids_dev, nullptr, nullptr, (u32*)toggles_out_dev, (int32_t*)status_dev,
                                 (const u8*)entropy_dev, (u8*)rows_out_dev, pick_stream(ctx, stream));
    });
}

// ---- selecting a round's bids (include/bbp.h; rules and kernels: round_select.h) ---------------------------------------------------
// The selection launches on s (round_select.h): the state zeroed, one launch per key byte, the counts, the ordered compaction
static int32_t select_kernels_enqueue(bbp_ctx* ctx, u32 B, const u32* recs, const RsFloor& floor, u32 K, u32 cap, u32* sel, u32* counts, u8* state,
                                      hipStream_t s) {
    const RsGeom g = rs_geom(B);
    RsState* st = (RsState*)state;
    ScopedEvent ev(ctx, TAG_SELECT, s);
    BBP_HIP_TRY(ctx, hipMemsetAsync(st, 0, sizeof(RsState), s));
    for (u32 pass = 0; pass < 32; pass++) hipLaunchKernelGGL(k_round_select_pass, dim3(g.G), dim3(RS_SEL_T), 0, s, B, g.span, recs, floor, K, pass, st);
    hipLaunchKernelGGL(k_round_select_count, dim3(g.G), dim3(RS_SEL_T), 0, s, B, g.span, recs, floor, counts, st);
    hipLaunchKernelGGL(k_round_select_write, dim3(g.G), dim3(RS_SEL_T), 0, s, B, g.span, recs, floor, cap, sel, (const RsState*)st);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

// Scoring and selection on s: the table reduced into the scratch at `base` (its RoundScratch header), one record per bid, then sel and
// counts.  Device pointers throughout; cap <= B entries of sel.
static int32_t select_enqueue(bbp_ctx* ctx, u32 N, const u8* table, u32 B, const u8* bids, const RsFloor& floor, u32 K, u32 cap, u32* sel, u32* counts,
                              int32_t* status, u32* scores, u8* base, const SelectScratch& ss, hipStream_t s) {
    int32_t rc;
    if ((rc = round_reduce_enqueue(ctx, N, table, base, ss.rs, s))) return rc;
    u32* recs = (u32*)(base + ss.recs);
    {  // a throughput launch: no LDS reservation, the waves of many workgroups share each SIMD
        ScopedEvent ev(ctx, TAG_WITNESS, s);
        hipLaunchKernelGGL(k_round_scores, dim3((B + RS_SCORE_T - 1) / RS_SCORE_T), dim3(RS_SCORE_T), 0, s, B, N, bids, (const sc*)(base + ss.rs.rblk),
                           (const int32_t*)(base + ss.rs.rflag), ctx->mimc_c, recs, status, scores);
        BBP_HIP_TRY(ctx, hipGetLastError());
    }
    return select_kernels_enqueue(ctx, B, recs, floor, K, cap, sel, counts, base + ss.state, s);
}

extern "C" int32_t bbp_select_round_dev(bbp_ctx* ctx, uint32_t N, const void* round_dev, uint32_t B, const void* bids_dev, const uint8_t floor32[32],
                                        uint32_t K, uint32_t cap, void* sel_dev, void* counts_dev, void* status_dev, void* scores_dev, void* prove_in_dev,
                                        void* tails_dev, void* toggles_dev, void* stream) {
    if (!ctx || !round_dev || !bids_dev || !floor32 || !counts_dev || !status_dev || (cap && !sel_dev)) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_select_round_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc = check_n(ctx, N);
        if (rc) return rc;
        if (B > BBP_SELECT_MAX_BIDS) return ctx->err = "bbp_select_round_dev: more than BBP_SELECT_MAX_BIDS bids", BBP_ERR_BAD_ARG;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        if (B == 0) {  // nothing qualifies: the counts say so, in stream order
            BBP_HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 8, s));
            return BBP_OK;
        }
        if (cap > B) cap = B;  // no more than B bids can be selected
        const bool expand = cap && (prove_in_dev || tails_dev || toggles_dev);
        if (expand && (rc = round_lanes_ok(ctx, N, cap))) return rc;
        const SelectScratch ss = select_scratch(B, expand ? cap : 0, N);
        // scratch in rotation, under the rule of round_dev_enqueue
        bbp_ctx::CheckBuf& cb = ctx->rnd[ctx->rnd_next++ % (u32)bbp_ctx::CHECK_RING];
        if ((rc = dev_reserve(ctx, cb.buf, ss.end))) return rc;
        if (!cb.ev) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&cb.ev, hipEventDisableTiming));
        if (cb.ev_valid) BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, cb.ev, 0));
        u8* base = (u8*)cb.buf.p;
        const u32* counts = (const u32*)counts_dev;
        if ((rc = select_enqueue(ctx, N, (const u8*)round_dev, B, (const u8*)bids_dev, rs_floor_load(floor32), K, cap, (u32*)sel_dev, (u32*)counts_dev,
                                 (int32_t*)status_dev, (u32*)scores_dev, base, ss, s)))
            return rc;
        if (expand) {  // the selected bids, gathered, through the existing pass: launches sized by cap, lanes at or beyond counts[0] leave at once
            u8* gb = base + ss.gbids;
            u32* rb = (u32*)(base + ss.rs.rb);
            ScopedEvent ev(ctx, TAG_WITNESS, s);
            hipLaunchKernelGGL(k_round_gather, dim3((unsigned)(((u64)cap * BBP_ROUND_BID_BYTES + 255) / 256)), dim3(256), 0, s, cap, (const u32*)sel_dev, counts,
                               (const u8*)bids_dev, gb);
            BBP_HIP_TRY(ctx, hipGetLastError());
            if ((rc = round_bids_enqueue(ctx, N, base, ss.rs, cap, gb, rb, counts, s)) ||
                (rc = round_expand_enqueue(ctx, N, (const u8*)round_dev, cap, gb, rb, (u32*)prove_in_dev, (u32*)tails_dev, (u32*)toggles_dev, nullptr, counts, s)))
                return rc;
            // the rows are announced as bbp_prepare_round_dev's are: the next prove call's opening stage waits for them by itself
            BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_prep, s));
            ctx->ev_prep_valid = true;
        }
        if (wipe_on(ctx)) {  // secret wiping: the ring entry (score records, gathered bids, their results), ahead of its event
            WipeList wl;
            wipe_take(wl, cb.buf);
            if ((rc = wipe_enqueue(ctx, wl, s))) return rc;
        }
        BBP_HIP_TRY(ctx, hipEventRecord(cb.ev, s));
        cb.ev_valid = true;
        return BBP_OK;
    });
}

// Phase A of bbp_prove_round_select on ONE device's context: table and bids up, scoring and selection, counts / sel / statuses (/ scores)
// down -- the one synchronisation of the call, waited for with the context lock released.  cap <= B: entries of sel_out.  recs_host
// (the debug hook): B records that stand where the scoring's would, nothing is scored then.
static int32_t select_phase_a(bbp_ctx* ctx, u32 N, const u8* round, u32 B, const u8* bids, const u32* recs_host, const uint8_t* floor32, u32 K, u32 cap,
                              u32* sel_out, u32 counts_out[2], int32_t* status, u8* scores_out) {
    std::lock_guard<std::mutex> phase(ctx->sel_mu);
    const SelectStaging L(B, cap, N, scores_out != nullptr);
    const size_t up = recs_host ? 0 : L.up_bytes;
    int32_t rc = api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        auto body = [&]() -> int32_t {
            int32_t rc;
            if ((rc = dev_reserve(ctx, ctx->sel_dev, L.bytes)) || (rc = pinned_reserve(ctx, ctx->sel_h, ctx->sel_h_cap, L.h_bytes))) return rc;
            if (!ctx->ev_sel) BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_sel, hipEventDisableTiming));
            hipStream_t s = ctx->stream;
            u8 *d = (u8*)ctx->sel_dev.p, *h = (u8*)ctx->sel_h;
            u32* recs = (u32*)(d + L.scratch + L.ss.recs);
            if (recs_host) {
                BBP_HIP_TRY(ctx, hipMemcpyAsync(recs, recs_host, 4 * (size_t)RS_WORDS * B, hipMemcpyHostToDevice, s));
                if ((rc = select_kernels_enqueue(ctx, B, recs, rs_floor_load(floor32), K, cap, (u32*)(d + L.sel), (u32*)(d + L.counts),
                                                 d + L.scratch + L.ss.state, s)))
                    return rc;
            } else {
                memcpy(h + L.bids, bids, ROUND_BID_BYTES * (size_t)B);
                memcpy(h + L.tab, round, round_table_bytes(N));
                BBP_HIP_TRY(ctx, hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, s));
                if ((rc = select_enqueue(ctx, N, d + L.tab, B, d + L.bids, rs_floor_load(floor32), K, cap, (u32*)(d + L.sel), (u32*)(d + L.counts),
                                         (int32_t*)(d + L.status), scores_out ? (u32*)(d + L.scores) : nullptr, d + L.scratch, L.ss, s)))
                    return rc;
            }
            BBP_HIP_TRY(ctx, hipMemcpyAsync(h + up, d + L.counts, L.down_bytes, hipMemcpyDeviceToHost, s));
            if (wipe_on(ctx)) {  // secret wiping: bids, records, selection, behind the copy that hands the results out
                WipeList wl;
                wipe_take(wl, ctx->sel_dev);
                if ((rc = wipe_enqueue(ctx, wl, s))) return rc;
            }
            BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_sel, s));
            return BBP_OK;
        };
        const int32_t rc = body();
        if (rc && wipe_on(ctx)) {  // a half-enqueued phase: everything SECRET, behind a device synchronise; the message stays this failure's
            const std::string why = ctx->err;
            (void)wipe_all(ctx);
            ctx->err = why;
        }
        return rc;
    });
    if (rc) return rc;
    const hipError_t e = wait_event_polling(ctx->ev_sel);
    if (e == hipSuccess) {
        const u8* down = (const u8*)ctx->sel_h + up;  // the fetched region starts at L.counts on the device
        memcpy(counts_out, down, 8);
        const u32 n = counts_out[0] < cap ? counts_out[0] : cap;
        if (n) memcpy(sel_out, down + (L.sel - L.counts), 4 * (size_t)n);
        if (!recs_host) memcpy(status, down + (L.status - L.counts), 4 * (size_t)B);
        if (scores_out) memcpy(scores_out, down + (L.scores - L.counts), 32 * (size_t)B);
    }
    if (wipe_on(ctx)) secure_zero(ctx->sel_h, std::min(ctx->sel_h_cap, L.h_bytes));
    if (e != hipSuccess) {
        api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string("collecting the selection: ") + hipGetErrorString(e), BBP_ERR_DEVICE; });
        return BBP_ERR_DEVICE;
    }
    return BBP_OK;
}

extern "C" int32_t bbp_prove_round_select(bbp_ctx* ctx, uint32_t N, const uint8_t* round, uint32_t B, const uint8_t* bids, const uint8_t floor32[32],
                                          uint32_t K, uint32_t cap, const uint8_t* entropy, uint8_t* rows_out, uint32_t* sel_out, uint32_t* n_sel,
                                          uint32_t* n_qualified, uint64_t* toggles_out, uint8_t* scores_out, int32_t* status) {
    if (!ctx || !round || !bids || !floor32 || !n_sel || !status || (cap && (!rows_out || !sel_out))) return BBP_ERR_BAD_ARG;
    bool done;
    const int32_t screened = round_select_screen(N, B, &done);
    if (screened || done) {
        *n_sel = 0;
        if (n_qualified) *n_qualified = 0;
        return api_guard(ctx, [&]() -> int32_t {
            if (int32_t rc = check_n(ctx, N)) return rc;  // (names the list length)
            if (screened) ctx->err = "bbp_prove_round_select: more than BBP_SELECT_MAX_BIDS bids";
            return screened;
        });
    }
    return no_throw_ctx(ctx, [&]() -> int32_t {
        bbp_ctx* const dev = is_pool(ctx) ? ctx->members[0] : ctx;  // phase A: one member scores, as bbp_witness_batch
        auto fail = [&](int32_t rc, const std::string& why) {
            api_guard(ctx, [&]() -> int32_t { return ctx->err = why, rc; });
            return rc;
        };
        const u32 cap_sel = cap < B ? cap : B;
        std::vector<u32> sel(cap_sel);
        u32 counts[2] = {0, 0};
        int32_t rc = select_phase_a(dev, N, round, B, bids, nullptr, floor32, K, cap_sel, sel.data(), counts, status, scores_out);
        if (rc) return dev == ctx ? rc : fail(rc, bbp_last_error(dev));
        *n_sel = counts[0];
        if (n_qualified) *n_qualified = counts[1];
        if (counts[0] > cap)
            return fail(BBP_ERR_BAD_ARG, "bbp_prove_round_select: " + std::to_string(counts[0]) + " bids selected, room for " + std::to_string(cap) +
                                             " (cap): nothing proved");
        const u32 n = counts[0];
        if (n == 0) return BBP_OK;
        // phase B: the selected bids from the CALLER's memory through bbp_prove_round's own path; entropy row j goes to sel[j]
        std::vector<uint8_t> picked(ROUND_BID_BYTES * (size_t)n);
        for (u32 j = 0; j < n; j++) memcpy(&picked[ROUND_BID_BYTES * (size_t)j], bids + ROUND_BID_BYTES * (size_t)sel[j], ROUND_BID_BYTES);
        std::vector<int32_t> st(n, BBP_ERR_INTERNAL);
        rc = bbp_prove_round(ctx, N, round, n, picked.data(), entropy, rows_out, toggles_out, st.data());
        secure_zero(picked.data(), picked.size());
        if (rc) return rc;
        memcpy(sel_out, sel.data(), 4 * (size_t)n);
        for (u32 j = 0; j < n; j++)
            if (st[j] != BBP_OK)
                return fail(BBP_ERR_INTERNAL, "bbp_prove_round_select: scoring accepted bid " + std::to_string(sel[j]) + ", proving refused it (status " +
                                                  std::to_string(st[j]) + ")");
        return BBP_OK;
    });
}

// Test hook: the shipped selection kernel on caller-made scores and statuses.  Synchronises.
extern "C" int32_t bbp_debug_round_select(bbp_ctx* ctx, uint32_t B, const uint8_t* scores, const int32_t* statuses, const uint8_t floor32[32], uint32_t K,
                                          uint32_t cap, uint32_t* sel_out, uint32_t* n_sel, uint32_t* n_qualified) {
    if (!ctx || !scores || !statuses || !floor32 || !n_sel || !n_qualified || (cap && !sel_out)) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_round_select");
    return no_throw_ctx(ctx, [&]() -> int32_t {
        auto refuse = [&](const char* why) {
            api_guard(ctx, [&]() -> int32_t { return ctx->err = why, BBP_ERR_BAD_ARG; });
            return (int32_t)BBP_ERR_BAD_ARG;
        };
        if (B == 0 || B > BBP_SELECT_MAX_BIDS) return refuse("bbp_debug_round_select: B is 0 or above BBP_SELECT_MAX_BIDS");
        std::vector<u32> recs((size_t)RS_WORDS * B, 0);
        for (u32 i = 0; i < B; i++) {
            u32* r = &recs[(size_t)RS_WORDS * i];
            for (int w = 0; w < 8; w++) r[RS_Q + w] = rb_le32(scores + 32 * (size_t)i + 4 * w);
            r[RS_STATUS] = (u32)statuses[i];
            if (!sc_is_canonical(r + RS_Q)) return refuse("bbp_debug_round_select: a score is not below l");
            if (statuses[i] != BBP_OK && statuses[i] != BBP_ERR_FORMAT && statuses[i] != BBP_ERR_BAD_ARG)
                return refuse("bbp_debug_round_select: a status is none of BBP_OK, BBP_ERR_FORMAT, BBP_ERR_BAD_ARG");
        }
        u32 counts[2] = {0, 0};
        const u32 cap_sel = cap < B ? cap : B;
        const int32_t rc = select_phase_a(ctx, 1, nullptr, B, nullptr, recs.data(), floor32, K, cap_sel, sel_out, counts, nullptr, nullptr);
        *n_sel = counts[0], *n_qualified = counts[1];
        return rc;
    });
}

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
// where a call's results go (n_duplicates: the one-per-bidder calls, otherwise null)
struct BestOut {
    u32 cap;
    u32 *best, *n_best, *n_candidates, *n_examined, *n_duplicates;
    u32* n_tranches = nullptr;  // the tranches that held at least one row (the many-rounds calls with one round report them)
};

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

// the K best winners (K == 0: all): selection, pairs, and everything the host reads into the mirror.  *room: pairs fetched at most.
static int32_t best_finish_enqueue(const BestCall& c, const int32_t* status_to_fetch, u32* room) {
    bbp_ctx* ctx = c.ctx;
    const u32 n = c.K && c.K < c.B ? c.K : c.B;
    *room = n;
    if (int32_t rc = select_kernels_enqueue(ctx, c.B, c.at(c.L.win), BEST_NO_FLOOR, c.K, n, c.at(c.L.sel), c.at(c.L.counts), c.d + c.L.state, c.s)) return rc;
    {
        ScopedEvent ev(ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_best_pairs, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, n, (const u32*)c.at(c.L.sel), (const u32*)c.at(c.L.counts),
                           (const u32*)c.at(c.L.win), c.at(c.L.pairs));
        BBP_HIP_TRY(ctx, hipGetLastError());
    }
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
static void stand_committed(const BestCall& c) {
    const StandCall& S = *c.stand;
    const u32* whdr = (const u32*)(c.h + S.W.h_whdr);
    bbp_ctx::Standing& m = *S.meta;
    m.count = whdr[STAND_H_COUNT];
    memcpy(m.bar, whdr + STAND_H_BAR, 32);
    m.offered += S.rows;
    m.trip = 0;
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
static int32_t best_public_host(bbp_ctx* ctx, u32 N, const uint8_t* round, u32 B, const uint8_t* rows, const uint8_t* floor32, u32 K, u32 tranche,
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
static int32_t best_hook_refuse(bbp_ctx* ctx, const std::string& why) {
    return api_guard(ctx, [&]() -> int32_t { return ctx->err = why, BBP_ERR_BAD_ARG; });
}
static int32_t best_hook_screen(bbp_ctx* ctx, const char* what, u32 B, const int32_t* verdicts, u32* n_ok) {
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
        auto fill = [&](u8* dst) { memcpy(dst, keys, 32 * (size_t)B); };
        BestCall c(ctx, B, K, ctx->stream, true, false);
        return best_run_host(c, fill, best_hook_read(verdicts), floor32, tranche, BestOut{cap, best_out, n_best, n_candidates, n_examined, nullptr}, status);
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
        BestCall c(ctx, B, K, pick_stream(ctx, stream), false, false);
        return best_run_dev(c, N, (const u8*)round_dev, (const u8*)rows_dev, (const u8*)entropy_dev, floor32, tranche,
                            BestOut{cap, best_out, n_best, n_candidates, n_examined, nullptr}, (int32_t*)status_dev);
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
        auto fill = [&](u8* dst) {
            for (u32 i = 0; i < B; i++) memcpy(dst + 64 * (size_t)i, keys + 32 * (size_t)i, 32), memcpy(dst + 64 * (size_t)i + 32, ids + 32 * (size_t)i, 32);
        };
        BestCall c(ctx, B, K, ctx->stream, true, true, table_log2);
        return best_run_host(c, fill, best_hook_read(verdicts), floor32, tranche, BestOut{cap, best_out, n_best, n_candidates, n_examined, n_duplicates},
                             status);
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
        BestCall c(ctx, B, K, pick_stream(ctx, stream), false, true);
        return best_run_dev(c, N, (const u8*)round_dev, (const u8*)rows_dev, (const u8*)entropy_dev, floor32, tranche,
                            BestOut{cap, best_out, n_best, n_candidates, n_examined, n_duplicates}, (int32_t*)status_dev);
    });
}

// ---- standing of a round (include/bbp.h; rules and kernels: round_standing.h) ---------------------------------------------------------
// An offer is a one-per-bidder host call over K + B working rows with a StandCall: the same driver.  The standings of a handle live on
// ONE device's context (a pool: member 0), found and changed under its best_mu.
static bbp_ctx* stand_dev(bbp_ctx* ctx) { return is_pool(ctx) ? ctx->members[0] : ctx; }
static int32_t stand_refuse(bbp_ctx* ctx, const std::string& why) {
    return api_guard(ctx, [&]() -> int32_t { return ctx->err = why, BBP_ERR_BAD_ARG; });
}
// the open standing behind a handle, or null (caller holds dev->best_mu)
static bbp_ctx::Standing* stand_find(bbp_ctx* dev, u32 handle) {
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
        return stand_offer(ctx, "bbp_standing_offer", standing, B,
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
                               return best_run_host(c, fill, verdicts, nullptr, tranche,
                                                    BestOut{cap, entered_out, n_entered, n_candidates, n_examined, n_duplicates}, status);
                           });
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
        return stand_offer(ctx, "bbp_debug_standing_offer", standing, B,
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
                               return best_run_host(c, fill, read, nullptr, tranche, BestOut{cap, entered_out, n_entered, n_candidates, n_examined, n_duplicates},
                                                    status);
                           });
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
struct BestsCall {
    bbp_ctx* ctx;
    u32 R, B, K, tranche;
    hipStream_t s;
    BestsLayout L;
    std::optional<BestsDistinctLayout> D;  // one per bidder only (rounds_best_distinct.h)
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
    size_t bytes() const { return D ? D->bytes : L.bytes; }
    size_t h_bytes() const { return D ? D->h_bytes : L.h_bytes; }
    size_t staged_row() const { return D ? 64 : 32; }
    size_t staged() const { return D ? D->kid : L.keys; }
    size_t h_staged() const { return D ? D->h_kid : L.h_keys; }
    const char* family() const { return D ? "best proofs of many rounds, one per bidder: " : "best valid proofs of many rounds: "; }
    unsigned long long* offb() const { return (unsigned long long*)(d + L.offb); }
};
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
    hipLaunchKernelGGL(k_bests_ids, dim3((c.B + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, c.B, base, dev_rows ? (const unsigned long long*)rowoff : nullptr,
                       (const u32*)c.at(L.rb), (const u32*)c.at(L.round_of), c.at(c.D->ids), dev_rows ? nullptr : rowoff);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// keys at base (the _dev form: the rows; else the staged keys {rows}) -> records, statuses, candidate counts, segments
static int32_t bests_segment_enqueue(const BestsCall& c, const u8* base, bool dev_rows, int32_t* status) {
    const BestsLayout& L = c.L;
    const dim3 grid((c.B + BEST_T - 1) / BEST_T), block(BEST_T);
    {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_bests_keys, grid, block, 0, c.s, c.B, base, dev_rows ? (const unsigned long long*)(c.d + L.rowoff) : nullptr,
                           (const u32*)c.at(L.rb), (const u32*)c.at(L.round_of), (const u32*)c.at(L.floors), c.at(L.recs), c.at(L.win), status, c.ctr(L.c_ncand));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
    }
    if (int32_t rc = bests_scan_enqueue(c, L.c_ncand, L.c_seg, false)) return rc;
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_place, grid, block, 0, c.s, c.B, (const u32*)c.at(L.recs), (const u32*)c.ctr(L.c_seg), c.ctr(L.c_fill), c.at(L.cand));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
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
    {
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
    return BBP_OK;
}

static int32_t bests_mark_enqueue(const BestsCall& c, u32 n, const int32_t* tstat, int32_t* status) {
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    hipLaunchKernelGGL(k_bests_mark, dim3((n + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, n, (const u32*)c.at(c.L.sel), tstat, status, c.at(c.L.recs),
                       c.at(c.L.win), c.ctr(c.L.c_examined), c.ctr(c.L.c_ok));
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// {one per bidder} behind the mark of a step of n rows: identities settled, holders' winner records opened, duplicates of running
// rounds dropped
static int32_t bests_settle_enqueue(const BestsCall& c, u32 n, const int32_t* tstat, int32_t* status) {
    const BestsLayout& L = c.L;
    const BestsDistinctLayout& D = *c.D;
    const u32 *sel = c.at(L.sel), *ids = c.at(D.ids), *round_of = c.at(L.round_of), mask = D.slots - 1;
    u32 *table = c.at(D.table), *flag = c.dctr(D.d_flag);
    ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
    const dim3 grid((n + BEST_T - 1) / BEST_T), block(BEST_T);
    hipLaunchKernelGGL(k_bests_settle, grid, block, 0, c.s, n, c.B, sel, tstat, (const u32*)c.at(L.recs), ids, round_of, table, mask, c.dctr(D.d_settled), flag);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bests_holders, grid, block, 0, c.s, n, c.B, sel, tstat, ids, round_of, (const u32*)table, mask, c.at(L.win), flag);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bests_drop, dim3((c.B + BEST_T - 1) / BEST_T), block, 0, c.s, c.B, c.K, c.at(L.recs), ids, round_of, (const u32*)table, mask, status,
                       (const u32*)c.dctr(D.d_settled), c.dctr(D.d_dups), flag);
    BBP_HIP_TRY(c.ctx, hipGetLastError());
    return BBP_OK;
}

// the winners' pairs (nw of them, grouped by round as off says) and everything the host reads, into the mirror
static int32_t bests_pairs_enqueue(const BestsCall& c, u32 nw, const int32_t* status_to_fetch) {
    const BestsLayout& L = c.L;
    if (nw) {
        ScopedEvent ev(c.ctx, TAG_SELECT, c.s);
        hipLaunchKernelGGL(k_best_pairs, dim3((nw + BEST_T - 1) / BEST_T), dim3(BEST_T), 0, c.s, nw, (const u32*)c.at(L.sel), (const u32*)c.ctr(L.c_off + c.R),
                           (const u32*)c.at(L.win), c.at(L.pairs));
        BBP_HIP_TRY(c.ctx, hipGetLastError());
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
    std::vector<char> running;  // round r contributed to the step planned last (all of them before step 0); a round that stopped stays stopped
    u32 n = 0;                  // the rows of the step planned last
    explicit BestsTally(const BestsCall& c)
        : R(c.R), K(c.K), tranche(c.tranche), distinct(c.D.has_value()), nc(R), examined(R), ok(R), take(R), settled(distinct ? R : 0),
          dups(settled.size()), running(settled.size(), 1) {}
    // the rows round r contributes to step t (finish: the winners it reports), from what the call holds of the device's counters
    u32 rows_of(u32 r, u32 t, bool finish) const {
        if (distinct) return finish ? bests_winners(K, settled[r]) : bests_take_distinct(K, tranche, t, nc[r], examined[r], dups[r], settled[r]);
        return finish ? bests_winners(K, ok[r]) : bests_take(K, tranche, t, nc[r], examined[r], ok[r]);
    }
    // the first counters: the candidate counts are the device's; B bounds them
    bool adopt_candidates(const BestsCall& c, std::string* why) {
        unsigned long long total = 0;
        for (u32 r = 0; r < R; r++) total += nc[r] = c.mirror(c.L.c_ncand)[r];
        if (total <= c.B && c.mirror(c.L.c_seg)[R] == total) return true;
        return *why = std::string(c.family()) + "the device counted " + std::to_string(total) + " candidates among " + std::to_string(c.B) + " rows", false;
    }
    // The most rows step t can hold, from what a host form knows before the device has planned it.  It has counted the valid rows, so
    // this is the step's size.  {A bound only, before the device has counted the last step's identities: a valid row settles at least
    // one identity, the mirrored dups are a lower bound.  0: every round has stopped for sure.}
    u32 bound(u32 t) const {
        unsigned long long sum = 0;
        for (u32 r = 0; r < R; r++) {
            if (!distinct)
                sum += rows_of(r, t, false);
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
                if (good) settled[r] = ds, dups[r] = dd;
            }
            if (good) ok[r] = dok;
        }
        if (good) {
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
        fill(c.h + c.h_staged());
        BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + c.staged(), c.h + c.h_staged(), c.staged_row() * c.B, hipMemcpyHostToDevice, c.s));
        if (c.D && (r = bests_ids_enqueue(c, c.d + c.staged(), false))) return r;  // (which says where each staged row starts)
        if ((r = bests_segment_enqueue(c, c.d + c.staged(), c.D.has_value(), (int32_t*)c.at(L.status)))) return r;
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
        const u32 nw = finish ? std::min(ty.winners_bound(), c.B) : 0;
        rc = submit([&]() -> int32_t {
            int32_t r;
            if (pending) {
                const int32_t* tstat = (const int32_t*)c.at(L.tstat);
                memcpy(c.h + L.h_tstat, st.data(), 4 * (size_t)pending);
                BBP_HIP_TRY(dev, hipMemcpyAsync(c.d + L.tstat, c.h + L.h_tstat, 4 * (size_t)pending, hipMemcpyHostToDevice, c.s));
                if ((r = bests_mark_enqueue(c, pending, tstat, (int32_t*)c.at(L.status)))) return r;
                if (c.D && (r = bests_settle_enqueue(c, pending, tstat, (int32_t*)c.at(L.status)))) return r;
            }
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
    if ((rc = bests_deliver(c, ty, round_of, steps, out, &why))) return fail(why, rc);
    memcpy(status, c.h + L.h_status, 4 * (size_t)c.B);
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
    int32_t verify(u32 n, const u32* sel, const u32* take, int32_t* st) {
        bests_step_rounds(R, take, step_round_of);
        picked.clear();
        for (u32 j = 0; j < n; j++) {
            if (sel[j] >= B || round_of[sel[j]] != step_round_of[j])
                return api_guard(ctx, [&]() -> int32_t { return ctx->err = std::string(family) + "a selected row is no row of its round", BBP_ERR_INTERNAL; });
            picked.insert(picked.end(), rows + rowoff[sel[j]], rows + rowoff[sel[j] + 1]);
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
        const size_t w = ids ? 64 : 32;
        auto fill = [&](u8* dst) {
            for (u32 i = 0; i < B; i++) {
                memcpy(dst + w * i, keys + 32 * (size_t)i, 32);
                if (ids) memcpy(dst + w * i + 32, ids + 32 * (size_t)i, 32);
            }
        };
        if (R == 1) {
            BestCall c(ctx, B, K, ctx->stream, true, ids != nullptr, table_log2);
            return best_run_host(c, fill, best_hook_read(verdicts), floors ? floors : BESTS_ZERO_FLOOR, tranche, out.one_round(), status);
        }
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
        if (R == 1) {
            BestCall c(ctx, B, K, pick_stream(ctx, stream), false, distinct);
            return best_run_dev(c, round_Ns[0], (const u8*)rounds_dev, (const u8*)rows_dev, (const u8*)entropy_dev, floors ? floors : BESTS_ZERO_FLOOR, tranche,
                                out.one_round(), (int32_t*)status_dev);
        }
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

extern "C" int32_t bbp_set_prove_check(bbp_ctx* ctx, int32_t on) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    for (bbp_ctx* m : ctx->members) bbp_set_prove_check(m, on);
    ctx->prove_check = on != 0;
    return BBP_OK;
}

extern "C" int32_t bbp_prove_check_stats(bbp_ctx* ctx, uint64_t* n_checked, uint64_t* n_unsatisfied, uint64_t* n_reproved, uint64_t* n_failed) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    uint64_t v[4] = {0, 0, 0, 0};
    std::vector<bbp_ctx*> ctxs = is_pool(ctx) ? ctx->members : std::vector<bbp_ctx*>{ctx};
    for (bbp_ctx* c : ctxs) {
        unsigned long long dc[2] = {0, 0};
        const int32_t rc = api_guard(c, [&]() -> int32_t {  // the device counters are final once the device is idle
            if (!c->chk_counts) return BBP_OK;
            BBP_HIP_TRY(c, hipSetDevice(c->device));
            BBP_HIP_TRY(c, hipDeviceSynchronize());
            BBP_HIP_TRY(c, hipMemcpy(dc, c->chk_counts, sizeof dc, hipMemcpyDeviceToHost));
            return BBP_OK;
        });
        if (rc) return rc;
        v[0] += c->chk_checked.load();
        v[1] += dc[0];
        v[2] += c->chk_reproved.load();
        v[3] += dc[1];
    }
    if (n_checked) *n_checked = v[0];
    if (n_unsatisfied) *n_unsatisfied = v[1];
    if (n_reproved) *n_reproved = v[2];
    if (n_failed) *n_failed = v[3];
    return BBP_OK;
}

extern "C" int32_t bbp_debug_corrupt_next_proof(bbp_ctx* ctx, uint32_t index) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_corrupt_next_proof");
    return api_guard(ctx, [&]() -> int32_t {
        ctx->debug_corrupt_proof = index;
        return BBP_OK;
    });
}

// the key of a device draw in host memory, as bytes and as words
struct DrawKey {
    bbp_ctx* ctx;
    uint8_t k[32] = {};
    ChachaKey ck{};
    ~DrawKey() {
        if (wipe_on(ctx)) secure_zero(k, sizeof k), secure_zero(&ck, sizeof ck);
    }
};

extern "C" int32_t bbp_draw_entropy_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, uint32_t kind, const uint8_t* key32, void* out_dev, void* stream) {
    if (!ctx || !out_dev || (kind != BBP_ENTROPY_PROVE && kind != BBP_ENTROPY_VERIFY)) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_draw_entropy_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc;
        if (kind == BBP_ENTROPY_PROVE && (rc = check_n(ctx, N))) return rc;
        if (B == 0) return BBP_OK;
        DrawKey dk{ctx};  // erased on every way out while secret wiping is on
        uint8_t* const k = dk.k;
        if (key32)
            memcpy(k, key32, sizeof dk.k);
        else if (!os_random(k, sizeof dk.k))
            return ctx->err = "cannot read /dev/urandom", BBP_ERR_DEVICE;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        dk.ck = chacha_key_from_bytes(k);
        if ((rc = draw_enqueue(ctx, B, N, kind, dk.ck, 0, out_dev, s))) return rc;  // (the launch takes the key by value)
        if (kind == BBP_ENTROPY_PROVE) {  // the next prove call's opening stage waits for these rows (not ev_prep: see context.h)
            BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_draw, s));
            ctx->ev_draw_valid = true;
        }
        return BBP_OK;
    });
}

extern "C" int32_t bbp_draw_entropy_hedged_dev(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* key32, const void* in_dev, void* out_dev, void* stream) {
    if (!ctx || !in_dev || !out_dev) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_draw_entropy_hedged_dev");
    return api_guard(ctx, [&]() -> int32_t {
        int32_t rc;
        if ((rc = check_n(ctx, N))) return rc;
        if (((uintptr_t)in_dev | (uintptr_t)out_dev) & 3) return ctx->err = "hedged entropy draw: rows must be 4-byte aligned", BBP_ERR_BAD_ARG;
        if (B == 0) return BBP_OK;
        DrawKey dk{ctx};  // erased on every way out while secret wiping is on
        uint8_t* const k = dk.k;
        if (key32)
            memcpy(k, key32, sizeof dk.k);
        else if (!os_random(k, sizeof dk.k))
            return ctx->err = "cannot read /dev/urandom", BBP_ERR_DEVICE;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        // the draw reads the rows: a pending prepare is waited for here, and stays pending for the next prove call (which reads them too)
        if (ctx->ev_prep_valid) BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_prep, 0));
        dk.ck = chacha_key_from_bytes(k);
        if ((rc = hedged_draw_enqueue(ctx, B, N, dk.ck, 0, in_dev, nullptr, out_dev, s))) return rc;  // (the launch takes the key by value)
        BBP_HIP_TRY(ctx, hipEventRecord(ctx->ev_draw, s));
        ctx->ev_draw_valid = true;
        return BBP_OK;
    });
}

extern "C" int32_t bbp_set_entropy_source(bbp_ctx* ctx, int32_t source) {
    if (!ctx || (source != BBP_ENTROPY_SOURCE_OS && source != BBP_ENTROPY_SOURCE_DEVICE && source != BBP_ENTROPY_SOURCE_HEDGED)) return BBP_ERR_BAD_ARG;
    for (bbp_ctx* m : ctx->members) bbp_set_entropy_source(m, source);
    ctx->entropy_source = source;
    return BBP_OK;
}

extern "C" int32_t bbp_debug_next_entropy_key(bbp_ctx* ctx, const uint8_t key32[32]) {
    if (!ctx || !key32) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_next_entropy_key");
    return api_guard(ctx, [&]() -> int32_t {
        memcpy(ctx->debug_key, key32, sizeof ctx->debug_key);
        ctx->debug_key_armed = true;
        return BBP_OK;
    });
}

// what the call combiner runs for a group of concurrent bbp_prove callers (submit.cpp)
int32_t bbp::prove_batch_locked(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out,
                                int32_t* status, std::string* err) {
    const int32_t rc = no_throw_ctx(ctx, [&]() -> int32_t { return prove_batch_host(ctx, B, N, in, entropy, out, status); });
    if (rc && err) *err = tls_error();
    return rc;
}

// completion hook of the asynchronous entry points (runs on a combiner thread): the request's message becomes that thread's
// bbp_last_error text for the duration of the callback, then the request is gone
static void async_done(Request* r) {
    try {
        set_tls_error(r->origin, r->status == BBP_OK ? std::string() : !r->err.empty() ? r->err
                                 : r->status == BBP_ERR_BAD_ARG ? (r->kind == 0 && static_cast<const bbp_ctx*>(r->origin)->prove_check
                                                                      ? refused_row_text(static_cast<const bbp_ctx*>(r->origin), r->in, r->N) : "toggle >= N")
                                     : r->status == BBP_ERR_FORMAT && r->kind == 0 ? "non-canonical scalar input"
                                                                                    : status_text(r->status));
    } catch (...) {
    }
    void (*fn)(void*, int32_t) = r->user_fn;
    void* user = r->user;
    const int32_t st = r->status;
    if (r->origin && wipe_on(static_cast<const bbp_ctx*>(r->origin))) secure_zero_vec(r->own_in), secure_zero_vec(r->own_entropy);
    delete r;
    fn(user, st);
}

static void fill_prove_input(std::vector<uint8_t>& in, const uint8_t scalars7[7 * 32], const uint8_t* pub_list, uint32_t N, uint64_t toggle) {
    in.resize(prove_in_bytes(N));
    memcpy(&in[0], scalars7, PROVE_IN_LIST);
    memcpy(&in[PROVE_IN_LIST], pub_list, (size_t)N * 32);
    memcpy(&in[prove_in_toggle(N)], &toggle, 8);
}

extern "C" int32_t bbp_prove(bbp_ctx* ctx, const uint8_t scalars7[7 * 32], const uint8_t* pub_list, uint32_t N, uint64_t toggle,
                             const uint8_t* entropy, uint8_t* proof_out, uint32_t* proof_len) {
    if (!ctx || !scalars7 || !proof_out) return BBP_ERR_BAD_ARG;
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc) return rc;
    if (!pub_list) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        std::vector<uint8_t> in;
        fill_prove_input(in, scalars7, pub_list, N, toggle);
        Request r;
        r.kind = 0;
        r.N = N;
        r.in = in.data();
        r.in_len = in.size();
        r.entropy = entropy;
        r.out = proof_out;
        const int32_t st = static_cast<Combiner*>(ctx->combiner)->submit(ctx, r);
        if (st != BBP_OK) {
            set_tls_error(ctx, !r.err.empty() ? r.err : st == BBP_ERR_BAD_ARG ? (ctx->prove_check ? refused_row_text(ctx, in.data(), N) : "toggle >= N")
                                                                             : "non-canonical scalar input");
            if (wipe_on(ctx)) secure_zero_vec(in);
            return st;
        }
        if (wipe_on(ctx)) secure_zero_vec(in);
        if (proof_len) *proof_len = BBP_R1CS_PROOF_BYTES;
        return BBP_OK;
    }, ctx);
}

extern "C" int32_t bbp_prove_async(bbp_ctx* ctx, const uint8_t scalars7[7 * 32], const uint8_t* pub_list, uint32_t N, uint64_t toggle,
                                   const uint8_t* entropy, uint8_t* proof_out, bbp_done_fn done, void* user) {
    if (!ctx || !scalars7 || !proof_out || !done) return BBP_ERR_BAD_ARG;
    int32_t rc = api_guard(ctx, [&]() -> int32_t { return check_n(ctx, N); });
    if (rc) return rc;
    if (!pub_list) return BBP_ERR_BAD_ARG;
    return no_throw([&]() -> int32_t {
        Request* r = new Request();
        r->kind = 0;
        r->N = N;
        fill_prove_input(r->own_in, scalars7, pub_list, N, toggle);  // inputs are copied: the caller's buffers are free on return
        r->in = r->own_in.data();
        r->in_len = r->own_in.size();
        if (entropy) {
            r->own_entropy.assign(entropy, entropy + bbp_entropy_size(N));
            r->entropy = r->own_entropy.data();
        }
        r->out = proof_out;
        r->on_done = async_done;
        r->origin = ctx;
        r->user_fn = done;
        r->user = user;
        if (!static_cast<Combiner*>(ctx->combiner)->submit_async(ctx, r)) {
            if (wipe_on(ctx)) secure_zero_vec(r->own_in), secure_zero_vec(r->own_entropy);
            delete r;
            set_tls_error(ctx, "call combiner: cannot start a batch thread");
            return BBP_ERR_INTERNAL;
        }
        return BBP_OK;
    }, ctx);
}

// The host-pointer verify path of one context; `rows` says what `in` holds (verify_rows.h; a rounds call: its table in host memory,
// uploaded behind the rows in the same staging slot).  Takes the context lock itself, for the enqueue phase only.
static int32_t verify_batch_host(bbp_ctx* ctx, const VerifyRows& rows, const uint8_t* in, int32_t* status, uint32_t group = 0,
                                 uint32_t* n_fallback = nullptr) {
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
                }
                return rc;
            });
        return rc;
    });
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
