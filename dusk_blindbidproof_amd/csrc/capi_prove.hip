// C-ABI, the calls that prove: witness and bid preparation, on-device entropy, checked proving, the host and device prove calls, proving a
// round from raw bids, selection -- see include/bbp.h for the reference interface each replaces.  The other call families and what this
// unit defines for them: capi.h.
#define BBP_ROUND_BIDS_KERNELS  // the kernels of round_bids.h and round_select.h are compiled here (capi.h)
#define BBP_ROUND_SELECT_KERNELS
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <functional>

#include "capi.h"
#include "hedge.h"
#include "round_bids.h"
#include "secret_map.h"
#include "witness_check.h"

namespace bbp {
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

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool os_random(uint8_t* buf, size_t n) {
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) return false;
    size_t got = fread(buf, 1, n, f);
    fclose(f);
    return got == n;
}

// B rows of `kind` (rows row_base.. of the key's streams) into out on s
int32_t draw_enqueue(bbp_ctx* ctx, u32 B, u32 N, u32 kind, const ChachaKey& key, u32 row_base, void* out, hipStream_t s) {
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

int32_t bbp::check_n(bbp_ctx* ctx, uint32_t N) {
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
// Waiting for a slot's event with the context lock released.  hipEventSynchronize by default; BBP_WAIT_POLL_US=n polls
// hipEventQuery every n microseconds instead (no measurable difference on MI355X / ROCm 7.2 once the copies were kept out of
// the DMA queues' way -- see fetch_results -- 18.7 k vs 18.6 k proofs/s from two threads; kept as a knob for runtimes where a
// thread parked in the runtime gets in the way of other threads' launches).
hipError_t wait_event_polling(hipEvent_t ev) {
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

int32_t pinned_reserve(bbp_ctx* ctx, void*& p, size_t& cap, size_t bytes) {
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
int32_t upload_inputs(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const uint8_t* a, size_t na, const uint8_t* b, size_t nb, size_t ent_off, const uint8_t* a2,
                      size_t na2, size_t a2_off) {
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
int32_t fetch_results(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, size_t bytes) {
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

int32_t bbp::no_os_random(bbp_ctx* ctx) {
    api_guard(ctx, [&]() -> int32_t { return ctx->err = "cannot read /dev/urandom", BBP_ERR_DEVICE; });
    return BBP_ERR_DEVICE;
}

// key of a host-pointer call that draws on the device: the armed test key (bbp_debug_next_entropy_key), else 32 OS bytes
int32_t bbp::next_device_key(bbp_ctx* ctx, ChachaKey* key) {
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

// (the check modes of a host prove call, CHECK_AUTO / CHECK_OFF / CHECK_REPROVE: capi.h)
// The other input of prove_batch_host (bbp_prove_round): the round's table and the raw bids in host memory instead of expanded
// rows.  They are uploaded as they are and the device pass (round_bids.h) writes the prover's rows into the staging slot; its
// per-bid statuses stand in for the host screening, and `out` receives rows record || score || z_img.
struct bbp::RoundInput {
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
int32_t bbp::staging_reserve(bbp_ctx* ctx, bbp_ctx::IoSlot& sl, const ProveStaging& L) {
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
int32_t bbp::prove_batch_host(bbp_ctx* ctx, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* entropy, uint8_t* out, int32_t* status,
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
int32_t bbp::select_kernels_enqueue(bbp_ctx* ctx, u32 B, const u32* recs, const RsFloor& floor, u32 K, u32 cap, u32* sel, u32* counts, u8* state,
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
void bbp::async_done(Request* r) {
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
