// Secret wiping (include/bbp.h "Secret wiping"; the classes are secret_map.h's, the placement rules DESIGN.md's): the wipe kernel and
// how a call hands it its spans, the wipe-everything pass, and the two test hooks that look at what is left.
#include <string.h>

#include "context.h"
#include "secret_map.h"
#include "submit.h"

namespace bbp {

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
struct WipeArgs {
    WipeSpan s[WIPE_SPANS];
};
constexpr u32 WIPE_BLK = 256;
constexpr u32 WIPE_PER_LANE = 8;    // 16-byte stores a lane makes when the grid is not capped
constexpr u32 WIPE_GRID_MAX = 2048;  // sized from the bytes, capped: beyond this a lane just makes more stores

// One launch erases every span of a call on one stream: blockIdx.y names the span, the blocks of a row walk it grid-stride with
// 16-byte stores.  Plain stores; spans are 16-aligned multiples of 16 bytes inside their buffers (wipe_enqueue checks).
__global__ void __launch_bounds__(WIPE_BLK) k_wipe_spans(WipeArgs a) {
    const WipeSpan sp = a.s[blockIdx.y];
    uint4* const p = static_cast<uint4*>(sp.p);
    const u64 n = sp.bytes >> 4, step = (u64)gridDim.x * WIPE_BLK;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (u64 i = (u64)blockIdx.x * WIPE_BLK + threadIdx.x; i < n; i += step) p[i] = z;
}

__device__ __forceinline__ u32 nonzero_bytes(u32 w) { return ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0); }

// Test hook: non-zero bytes of p[0 .. bytes) added to *out (block reduction, one atomic per block); the ragged tail behind the last
// whole 16 bytes is lane 0's of block 0.
__global__ void __launch_bounds__(WIPE_BLK) k_residue_count(const u8* __restrict__ p, u64 bytes, unsigned long long* __restrict__ out) {
    __shared__ u32 part[WIPE_BLK];
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const u64 n = bytes >> 4, step = (u64)gridDim.x * WIPE_BLK;
    u32 c = 0;
    for (u64 i = (u64)blockIdx.x * WIPE_BLK + threadIdx.x; i < n; i += step) {
        const uint4 v = q[i];
        c += nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (u64 i = n << 4; i < bytes; i++) c += p[i] != 0;
    part[threadIdx.x] = c;
    __syncthreads();
    for (u32 d = WIPE_BLK / 2; d >= 1; d >>= 1) {
        if (threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(out, (unsigned long long)part[0]);
}

struct ScanPattern {
    u32 w[16];
};
// Test hook: exact matches of the pattern's `len` words at every 4-byte offset of p[0 .. n_words) added to *out.
__global__ void __launch_bounds__(WIPE_BLK) k_pattern_scan(const u32* __restrict__ p, u64 n_words, ScanPattern pat, u32 len, unsigned long long* __restrict__ out) {
    if (n_words < len) return;
    const u64 last = n_words - len, step = (u64)gridDim.x * WIPE_BLK;
    u32 c = 0;
    for (u64 i = (u64)blockIdx.x * WIPE_BLK + threadIdx.x; i <= last; i += step) {
        if (p[i] != pat.w[0]) continue;
        bool eq = true;
        for (u32 k = 1; k < len; k++) eq = eq && p[i + k] == pat.w[k];
        c += eq;
    }
    if (c) atomicAdd(out, (unsigned long long)c);
}

// ---- what a call hands the wipe ------------------------------------------------------------------------------------------------------
void wipe_take(WipeList& l, DevBuf& b) {
    size_t bytes = wipe_round(b.dirty);
    if (bytes > b.cap) bytes = b.cap / WIPE_GRAIN * WIPE_GRAIN;  // (never: a buffer is allocated 4096 bytes beyond what was asked of it)
    b.dirty = 0;
    if (!b.p || !bytes) return;
    if (l.n < WIPE_SPANS) l.s[l.n] = WipeSpan{b.p, bytes}, l.buf[l.n] = &b;
    l.n++;  // a list that overflows is refused by wipe_enqueue
}

static int32_t wipe_launch(bbp_ctx* ctx, const WipeSpan* spans, int n, hipStream_t s) {
    WipeArgs a{};
    u64 widest = 0;
    for (int i = 0; i < n; i++) {
        if (((uintptr_t)spans[i].p | spans[i].bytes) & (WIPE_GRAIN - 1)) return ctx->err = "secret wipe: a span is not 16-byte aligned", BBP_ERR_INTERNAL;
        a.s[i] = spans[i];
        if (spans[i].bytes > widest) widest = spans[i].bytes;
    }
    const u64 blocks = (widest / WIPE_GRAIN + WIPE_BLK * WIPE_PER_LANE - 1) / (WIPE_BLK * WIPE_PER_LANE);
    const u32 gx = blocks < 1 ? 1u : blocks > WIPE_GRID_MAX ? WIPE_GRID_MAX : (u32)blocks;
    ScopedEvent ev(ctx, TAG_WIPE, s);
    hipLaunchKernelGGL(k_wipe_spans, dim3(gx, (u32)n), dim3(WIPE_BLK), 0, s, a);
    BBP_HIP_TRY(ctx, hipGetLastError());
    return BBP_OK;
}

int32_t wipe_enqueue(bbp_ctx* ctx, const WipeList& l, hipStream_t s) {
    if (l.n == 0) return BBP_OK;
    if (l.n > WIPE_SPANS) return ctx->err = "secret wipe: too many spans for one launch", BBP_ERR_INTERNAL;
    // what bbp_debug_wipe_cost reports: the spans of every wipe since the log was last cleared, by buffer
    bbp_ctx::WipeLog& log = ctx->wipe_log;
    log.launches++;
    for (int i = 0; i < l.n; i++) {
        log.bytes += l.s[i].bytes;
        // n saturates one past CAP ("more than one launch replays"): a context that wipes for months never walks it out of range
        if (log.n < bbp_ctx::WipeLog::CAP) log.buf[log.n] = l.buf[i], log.span_bytes[log.n] = l.s[i].bytes;
        if (log.n <= bbp_ctx::WipeLog::CAP) log.n++;
    }
    return wipe_launch(ctx, l.s, l.n, s);
}

// ---- every buffer of the context, classed (secret_map.h) ---------------------------------------------------------------------------------
struct MemRef {
    const char* name;
    void* p;
    size_t cap;
    int cls;
    DevBuf* buf;  // device: the DevBuf behind it, if it is one
};
static void device_buffers(bbp_ctx* c, std::vector<MemRef>& v) {
    // the one table (secret_map.h)
#define X(name, field, count, secret)                                                                       \
    for (int i = 0; i < (int)(count); i++) {                                                                \
        DevBuf& b = field;                                                                                  \
        if (b.p) v.push_back(MemRef{name, b.p, b.cap, (secret) ? SC_SECRET : SC_PUBLIC, &b});              \
    }
    BBP_CTX_DEVICE_BUFFERS(X, bbp_ctx::PROVE_BUFS, bbp_ctx::VERIFY_SLOT, bbp_ctx::IO_SLOTS)
#undef X
    // ... and what is not a DevBuf: the resident tables, PUBLIC, for the scan
    auto raw = [&](const char* name, void* p, size_t bytes) {
        if (p) v.push_back(MemRef{name, p, bytes, SC_PUBLIC, nullptr});
    };
    raw("gens", c->gens, sizeof(ge) * (size_t)TAB_BASES);
    raw("ptable", c->ptable, sizeof(niels_row) * (size_t)TAB_BASES * MSM_POS);
    raw("btab", c->btab, tail_btab_bytes());
    raw("comb", c->comb, sizeof(niels_packed) * 2 * 64 * 8);
    raw("mimc_c", c->mimc_c, sizeof(sc) * BBP_MIMC_ROUNDS);
}
static void pinned_buffers(bbp_ctx* c, std::vector<MemRef>& v) {
#define X(name, ptr, cap, count, secret)                                                                    \
    for (int i = 0; i < (int)(count); i++)                                                                  \
        if (ptr) v.push_back(MemRef{name, ptr, cap, (secret) ? SC_SECRET : SC_PUBLIC, nullptr});
    BBP_CTX_PINNED_BUFFERS(X, bbp_ctx::IO_SLOTS)
#undef X
    for (auto& L : c->vl)
        for (auto& e : L.ns_ring)
            if (e.h) v.push_back(MemRef{"vl.ns_ring", e.h, e.cap, SC_PUBLIC, nullptr});
}

int32_t wipe_all(bbp_ctx* ctx) {
    BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BBP_HIP_TRY(ctx, hipDeviceSynchronize());  // nothing of this context reads or writes a buffer while it is erased
    std::vector<MemRef> dev, host;
    device_buffers(ctx, dev);
    pinned_buffers(ctx, host);
    for (const MemRef& m : dev) {
        if (m.cls != SC_SECRET) continue;
        BBP_HIP_TRY(ctx, hipMemsetAsync(m.p, 0, m.cap, ctx->stream));  // the whole capacity, ragged end included: the rare pass
        if (m.buf) m.buf->dirty = 0;
    }
    ctx->wipe_log = bbp_ctx::WipeLog{};
    BBP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const MemRef& m : host)
        if (m.cls == SC_SECRET) secure_zero(m.p, m.cap);
    return BBP_OK;
}

// Test hook (bbp_debug_poison_scratch): wipe_all with another fill value and over both classes.  Every DevBuf of the table over its whole
// capacity and every pinned mirror, except what secret_map.h exempts (state that outlives a call); the resident tables, the compiled
// circuits and the counter words are not in the walk.  `dirty` stays: what a wiping call owes is not changed by a fill.
static void fill_words(void* p, size_t bytes, uint32_t word) {  // host memory: whole words, then the ragged end from the word's low bytes
    uint8_t* q = static_cast<uint8_t*>(p);
    size_t i = 0;
    for (; i + 4 <= bytes; i += 4) memcpy(q + i, &word, 4);
    if (i < bytes) memcpy(q + i, &word, bytes - i);
}
int32_t poison_all(bbp_ctx* ctx, uint32_t word, uint64_t* dev_bytes, uint64_t* host_bytes, uint32_t* n_buffers) {
    BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BBP_HIP_TRY(ctx, hipDeviceSynchronize());
    std::vector<MemRef> dev, host;
    device_buffers(ctx, dev);
    pinned_buffers(ctx, host);
    *dev_bytes = 0, *host_bytes = 0, *n_buffers = 0;
    for (const MemRef& m : dev) {
        if (!m.buf || poison_exempt(m.name)) continue;  // (no DevBuf behind it: a resident table)
        BBP_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)m.p, (int)word, m.cap / 4, ctx->stream));
        if (m.cap % 4) BBP_HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(m.p) + m.cap / 4 * 4, &word, m.cap % 4, hipMemcpyHostToDevice, ctx->stream));
        *dev_bytes += m.cap, ++*n_buffers;
    }
    BBP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const MemRef& m : host) {
        if (poison_exempt(m.name)) continue;
        fill_words(m.p, m.cap, word);
        *host_bytes += m.cap;
    }
    return BBP_OK;
}

// A host-pointer prove call whose enqueue step failed half-way: what it reserved and did not get to wipe -- every SECRET buffer that is
// still `dirty` (a call that was enqueued whole has reset its own) and its staging slot with the slot's mirrors -- behind a device
// synchronise, since streams may still read them.  Other calls' staging slots are theirs: a caller that is collecting its results with
// the lock released keeps them.
int32_t wipe_failed_call(bbp_ctx* ctx, bbp_ctx::IoSlot& sl) {
    BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BBP_HIP_TRY(ctx, hipDeviceSynchronize());
    std::vector<MemRef> dev;
    device_buffers(ctx, dev);
    const char *io0 = reinterpret_cast<const char*>(&ctx->io[0]), *io1 = reinterpret_cast<const char*>(&ctx->io[bbp_ctx::IO_SLOTS + bbp_ctx::IO_VSLOTS]);
    const char *s0 = reinterpret_cast<const char*>(&sl), *s1 = reinterpret_cast<const char*>(&sl + 1);
    for (const MemRef& m : dev) {
        const char* at = reinterpret_cast<const char*>(m.buf);
        if (m.cls != SC_SECRET || !m.buf || !m.buf->dirty) continue;
        if (at >= io0 && at < io1 && !(at >= s0 && at < s1)) continue;  // another call's slot
        const size_t bytes = m.buf->dirty < m.cap ? m.buf->dirty : m.cap;
        BBP_HIP_TRY(ctx, hipMemsetAsync(m.p, 0, bytes, ctx->stream));
        m.buf->dirty = 0;
    }
    BBP_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sl.h_in) secure_zero(sl.h_in, sl.h_in_cap);
    if (sl.h_out) secure_zero(sl.h_out, sl.h_cap);
    return BBP_OK;
}

static u32 scan_grid(u64 items) {
    const u64 blocks = (items + WIPE_BLK * WIPE_PER_LANE - 1) / (WIPE_BLK * WIPE_PER_LANE);
    return blocks < 1 ? 1u : blocks > WIPE_GRID_MAX ? WIPE_GRID_MAX : (u32)blocks;
}

}  // namespace bbp

using namespace bbp;

extern "C" int32_t bbp_set_secret_wipe(bbp_ctx* ctx, int32_t on) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (ctx->combiner) static_cast<Combiner*>(ctx->combiner)->set_secret_wipe(on != 0);
    if (is_pool(ctx)) {
        ctx->secret_wipe = on != 0;
        for (bbp_ctx* m : ctx->members)
            if (int32_t rc = bbp_set_secret_wipe(m, on)) return rc;
        return BBP_OK;
    }
    return api_guard(ctx, [&]() -> int32_t {
        ctx->secret_wipe = on != 0;
        return on ? wipe_all(ctx) : (int32_t)BBP_OK;  // the invariant holds from here: everything is zero, and every call erases what it writes
    });
}

extern "C" int32_t bbp_wipe_secrets(bbp_ctx* ctx) {
    if (!ctx) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) {
        for (bbp_ctx* m : ctx->members)
            if (int32_t rc = bbp_wipe_secrets(m)) return rc;
        return BBP_OK;
    }
    return api_guard(ctx, [&]() -> int32_t { return wipe_all(ctx); });
}

extern "C" int32_t bbp_debug_secret_residue(bbp_ctx* ctx, uint64_t* dev_bytes, uint64_t* host_bytes, char* where, uint32_t cap) {
    if (!ctx || !dev_bytes || !host_bytes || (cap && !where)) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_secret_residue");
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BBP_HIP_TRY(ctx, hipDeviceSynchronize());
        std::vector<MemRef> dev, host;
        device_buffers(ctx, dev);
        pinned_buffers(ctx, host);
        std::vector<unsigned long long> counts(dev.size() + 1, 0);
        unsigned long long* d_counts = nullptr;
        BBP_HIP_TRY(ctx, hipMalloc(&d_counts, counts.size() * sizeof(unsigned long long)));
        hipError_t e = hipMemsetAsync(d_counts, 0, counts.size() * sizeof(unsigned long long), ctx->stream);
        for (size_t i = 0; i < dev.size() && e == hipSuccess; i++) {
            if (dev[i].cls != SC_SECRET) continue;
            hipLaunchKernelGGL(k_residue_count, dim3(scan_grid(dev[i].cap / 16)), dim3(WIPE_BLK), 0, ctx->stream, (const u8*)dev[i].p, (u64)dev[i].cap, d_counts + i);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_counts);
        if (e != hipSuccess) return ctx->err = std::string("secret residue: ") + hipGetErrorString(e), BBP_ERR_DEVICE;
        const char* first = nullptr;
        *dev_bytes = 0, *host_bytes = 0;
        for (size_t i = 0; i < dev.size(); i++) {
            *dev_bytes += counts[i];
            if (counts[i] && !first) first = dev[i].name;
        }
        for (const MemRef& m : host) {
            if (m.cls != SC_SECRET) continue;
            uint64_t c = 0;
            const uint8_t* q = static_cast<const uint8_t*>(m.p);
            for (size_t i = 0; i < m.cap; i++) c += q[i] != 0;
            *host_bytes += c;
            if (c && !first) first = m.name;
        }
        if (cap) snprintf(where, cap, "%s", first ? first : "");
        return BBP_OK;
    });
}

extern "C" int32_t bbp_debug_secret_scan(bbp_ctx* ctx, const uint8_t* pattern, uint32_t len, uint64_t* dev_hits, uint64_t* host_hits) {
    if (!ctx || !pattern || !dev_hits || !host_hits) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_secret_scan");
    return api_guard(ctx, [&]() -> int32_t {
        if (len < 4 || len > 64 || len % 4) return ctx->err = "bbp_debug_secret_scan: len is a multiple of 4 from 4 to 64", BBP_ERR_BAD_ARG;
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BBP_HIP_TRY(ctx, hipDeviceSynchronize());
        ScanPattern pat{};
        memcpy(pat.w, pattern, len);
        std::vector<MemRef> dev, host;
        device_buffers(ctx, dev);  // SECRET and PUBLIC alike: the scan is what finds a buffer the table classed wrongly
        pinned_buffers(ctx, host);
        unsigned long long* d_count = nullptr;
        unsigned long long hits = 0;
        BBP_HIP_TRY(ctx, hipMalloc(&d_count, sizeof(unsigned long long)));
        hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream);
        for (size_t i = 0; i < dev.size() && e == hipSuccess; i++) {
            const u64 n_words = dev[i].cap / 4;
            if (n_words < len / 4) continue;
            hipLaunchKernelGGL(k_pattern_scan, dim3(scan_grid(n_words)), dim3(WIPE_BLK), 0, ctx->stream, (const u32*)dev[i].p, n_words, pat, len / 4, d_count);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&hits, d_count, sizeof hits, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_count);
        if (e != hipSuccess) return ctx->err = std::string("secret scan: ") + hipGetErrorString(e), BBP_ERR_DEVICE;
        *dev_hits = hits;
        *host_hits = 0;
        for (const MemRef& m : host) {
            const uint8_t* q = static_cast<const uint8_t*>(m.p);
            for (size_t i = 0; i + len <= m.cap; i += 4)
                if (!memcmp(q + i, pattern, len)) ++*host_hits;
        }
        return BBP_OK;
    });
}

extern "C" int32_t bbp_debug_poison_scratch(bbp_ctx* ctx, uint32_t word, int32_t sticky, uint64_t* dev_bytes, uint64_t* host_bytes, uint32_t* n_buffers) {
    if (!ctx || !dev_bytes || !host_bytes || !n_buffers) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_poison_scratch");
    return api_guard(ctx, [&]() -> int32_t {
        ctx->poison_word = word;
        ctx->poison_sticky.store(sticky != 0, std::memory_order_relaxed);
        return poison_all(ctx, word, dev_bytes, host_bytes, n_buffers);
    });
}

extern "C" int32_t bbp_debug_wipe_cost(bbp_ctx* ctx, int32_t clear, uint64_t* bytes, uint32_t* launches, float* lone_us) {
    if (!ctx || !bytes || !launches || !lone_us) return BBP_ERR_BAD_ARG;
    if (is_pool(ctx)) return pool_reject(ctx, "bbp_debug_wipe_cost");
    return api_guard(ctx, [&]() -> int32_t {
        BBP_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BBP_HIP_TRY(ctx, hipDeviceSynchronize());  // idle device: the logged wipes have run, the spans read zero already
        bbp_ctx::WipeLog& log = ctx->wipe_log;
        *bytes = log.bytes, *launches = log.launches, *lone_us = 0.f;
        if (log.n > bbp_ctx::WipeLog::CAP) return ctx->err = "bbp_debug_wipe_cost: more spans logged than one launch takes; clear the log before the call to measure", BBP_ERR_BAD_ARG;
        if (log.n) {
            WipeSpan spans[bbp_ctx::WipeLog::CAP];
            for (int i = 0; i < log.n; i++) {  // the buffers as they are now: one that grew since keeps the logged length, which it still holds
                if (!log.buf[i]->p || log.span_bytes[i] > log.buf[i]->cap) return ctx->err = "bbp_debug_wipe_cost: a logged buffer shrank", BBP_ERR_INTERNAL;
                spans[i] = WipeSpan{log.buf[i]->p, log.span_bytes[i]};
            }
            hipEvent_t a = nullptr, b = nullptr;
            BBP_HIP_TRY(ctx, hipEventCreate(&a));
            BBP_HIP_TRY(ctx, hipEventCreate(&b));
            hipError_t e = hipEventRecord(a, ctx->stream);
            int32_t rc = e == hipSuccess ? wipe_launch(ctx, spans, log.n, ctx->stream) : (int32_t)BBP_ERR_DEVICE;
            if (rc == BBP_OK && (e = hipEventRecord(b, ctx->stream)) == hipSuccess && (e = hipEventSynchronize(b)) == hipSuccess) {
                float ms = 0.f;
                e = hipEventElapsedTime(&ms, a, b);
                *lone_us = ms * 1000.f;
            }
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
            if (rc) return rc;
            if (e != hipSuccess) return ctx->err = std::string("bbp_debug_wipe_cost: ") + hipGetErrorString(e), BBP_ERR_DEVICE;
        }
        if (clear) log = bbp_ctx::WipeLog{};
        return BBP_OK;
    });
}
