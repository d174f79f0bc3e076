// TEST INFRASTRUCTURE: the host side of secret wiping (include/bbp.h "Secret wiping") as a stand-alone program under AddressSanitizer +
// UBSan: the erase helpers of csrc/secure_zero.h, and the call combiner (csrc/submit.cpp, the product's own code)
// behind a stand-in engine.  The combiner gathers the rows and entropy of a prove batch into vectors of its own; with wiping on they
// must read zero when their memory is released.  This program replaces the global operator delete: the stand-in engine notes where the
// batch's rows and entropy lie, and the block that is released there is read before it goes back -- all zero, or not.
// Prints one line per scenario; exit code 0 = all of them passed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/secure_zero.h"
#include "../dusk_blindbidproof_amd/csrc/submit.h"

// ---- the watched blocks ----------------------------------------------------------------------------------------------------------
struct Watch {
    std::atomic<const void*> p{nullptr};
    std::atomic<size_t> n{0};
};
static Watch g_watch[2];  // the batch's rows, its entropy
static std::atomic<int> g_zero{0}, g_dirty{0};

static void released(void* p) {
    if (!p) return;
    for (Watch& w : g_watch) {
        if (w.p.load() != p) continue;
        const unsigned char* q = static_cast<const unsigned char*>(p);
        size_t nz = 0;
        for (size_t i = 0; i < w.n.load(); i++) nz += q[i] != 0;
        (nz ? g_dirty : g_zero)++;
        w.p = nullptr;
    }
}
void* operator new(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void operator delete(void* p) noexcept {
    released(p);
    free(p);
}
void operator delete(void* p, size_t) noexcept {
    released(p);
    free(p);
}

// ---- the stand-in engine ---------------------------------------------------------------------------------------------------------
struct bbp_ctx {
    std::atomic<int> calls{0}, bad{0};
};
static size_t prow_len(uint32_t N) { return 7 * 32 + 32 * (size_t)N + 8; }
static size_t ent_len(uint32_t N) { return 32 * (4 + (size_t)N) + 32; }
static size_t rec_len(uint32_t N) { return 1121 + 32 * (4 + (size_t)N); }

namespace bbp {
int32_t prove_batch_locked(bbp_ctx* c, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t* ent, uint8_t* out, int32_t* status, std::string*) {
    g_watch[0].n = prow_len(N) * B, g_watch[0].p = in;
    g_watch[1].n = ent ? ent_len(N) * B : 0, g_watch[1].p = ent;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + prow_len(N) * i;
        if (row[0] == 0 || (ent && ent[ent_len(N) * i] == 0)) c->bad++;  // the gathered copies are intact while the engine reads them
        status[i] = 0;
        memset(out + rec_len(N) * i, row[0], rec_len(N));
    }
    c->calls++;
    return 0;
}
int32_t verify_batch_locked(bbp_ctx*, uint32_t B, uint32_t, uint32_t, const uint8_t*, int32_t* status, std::string*) {
    for (uint32_t i = 0; i < B; i++) status[i] = 0;
    return 0;
}
}  // namespace bbp

static int g_fail = 0;
static void expect(bool ok, const char* what) {
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) g_fail++;
}

// four blocking callers with entropy through one combiner; every record must come back whatever the setting
static bool run_callers(bool wipe) {
    bbp_ctx eng;
    bool good = true;
    {
        bbp::Combiner comb;
        comb.set_secret_wipe(wipe);
        const uint32_t N = 3;
        std::vector<std::thread> th;
        std::atomic<int> wrong{0};
        for (int t = 0; t < 4; t++)
            th.emplace_back([&, t] {
                std::vector<uint8_t> in(prow_len(N), (uint8_t)(0x11 * (t + 1))), ent(ent_len(N), (uint8_t)(0xA0 + t)), out(rec_len(N), 0);
                bbp::Request r;
                r.kind = 0, r.N = N, r.in = in.data(), r.in_len = in.size(), r.entropy = ent.data(), r.out = out.data();
                const int32_t st = comb.submit(&eng, r);
                if (st != 0 || out[0] != in[0] || out[rec_len(N) - 1] != in[0]) wrong++;
                if (in[5] != (uint8_t)(0x11 * (t + 1)) || ent[5] != (uint8_t)(0xA0 + t)) wrong++;  // the caller's own buffers stay the caller's
            });
        for (auto& t : th) t.join();
        good = wrong == 0 && eng.bad == 0 && eng.calls > 0;
    }
    return good;
}

int main() {
    // 1. the helpers: a buffer and a vector over its whole capacity (what a shrink left behind included)
    {
        uint8_t key[32];
        memset(key, 0x5A, sizeof key);
        bbp::secure_zero(key, sizeof key);
        size_t nz = 0;
        for (uint8_t b : key) nz += b != 0;
        std::vector<uint8_t> v(4096, 0xC3);
        v.resize(100);
        bbp::secure_zero_vec(v);
        bool kept = v.size() == 100;
        v.resize(v.capacity());
        for (uint8_t b : v) nz += b != 0;
        std::vector<uint8_t> w(513, 0x77);
        bbp::secure_zero_vec(w);
        for (uint8_t b : w) nz += b != 0;
        std::vector<uint8_t> none;
        bbp::secure_zero_vec(none);
        expect(nz == 0 && kept, "erase helpers: a key, a shrunk vector over its capacity, an odd length, an empty vector");
    }
    // 2. a request's own copies (what an asynchronous request holds until its callback has fired)
    {
        bbp::Request r;
        r.own_in.assign(prow_len(8), 0xEE), r.own_entropy.assign(ent_len(8), 0xDD);
        bbp::secure_zero_vec(r.own_in), bbp::secure_zero_vec(r.own_entropy);
        size_t nz = 0;
        for (uint8_t b : r.own_in) nz += b != 0;
        for (uint8_t b : r.own_entropy) nz += b != 0;
        expect(nz == 0 && r.own_in.size() == prow_len(8), "request copies read zero before the request is deleted");
    }
    // 3. the combiner's batch vectors.  Off first: the watch sees what a release without an erase looks like.
    g_zero = 0, g_dirty = 0;
    const bool off_ok = run_callers(false);
    const int off_zero = g_zero, off_dirty = g_dirty;
    expect(off_ok && off_dirty >= 2 && off_zero == 0, "wiping off: records right, the batch's rows and entropy are released as they are (the watch can see)");
    g_zero = 0, g_dirty = 0;
    const bool on_ok = run_callers(true);
    const int on_zero = g_zero, on_dirty = g_dirty;
    expect(on_ok && on_dirty == 0 && on_zero >= 2, "wiping on: records right, the batch's rows and entropy read zero when they are released");
    printf("released blocks: off %d zero / %d dirty, on %d zero / %d dirty\n", off_zero, off_dirty, on_zero, on_dirty);
    if (g_fail) return 1;
    printf("secret_wipe_san ok\n");
    return 0;
}
