// TEST INFRASTRUCTURE: csrc/secret_map.h (the classes and spans of secret wiping) compiled for the host, as a stand-alone program under
// AddressSanitizer + UBSan (CPU build only).  For the real circuits of N = 1, 8, 202:
//   - every name of BBP_BATCH_ARRAYS is classed exactly once, and the two class lists name nothing else;
//   - the alignment assertions of batch_spans hold (256-aligned arrays, 8-byte strides, spans inside their carve slots);
//   - for (B, N) = (3, 1), (64, 8), (2, 202) the secret spans cover the B rows of every secret array without a gap, overlap nothing
//     (neither each other nor a public array's rows) and end inside the reservation; secret + public spans cover every array.
// Prints one line per check; exit code 0 = all of them passed.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/circuit.h"
#include "../dusk_blindbidproof_amd/csrc/secret_map.h"

using namespace bbp;

static int g_fail = 0;
static void expect(bool ok, const std::string& what) {
    printf("%s: %s\n", ok ? "ok" : "FAILED", what.c_str());
    if (!ok) g_fail++;
}

static BatchDims dims_of(uint32_t N) {
    const circuit::Compiled c = circuit::compile(N);
    return BatchDims{c.m, c.n_mul, c.n_cons, circuit::cst_count(N)};
}

struct Row {
    std::string name;
    size_t off, bytes;  // the exact B rows of the array in the carve
};
static std::vector<Row> arrays_of(uint32_t B, const BatchDims& d) {
    const BatchOffsets o = batch_offsets(B, d);
    std::vector<Row> v;
#define X(name, T, count) v.push_back(Row{#name, o.name, (size_t)(count) * sizeof(T) * B});
    BBP_BATCH_ARRAYS(X)
#undef X
    return v;
}

int main() {
    // classes
    {
        const BatchDims d = dims_of(8);
        bool once = true;
        int n_secret = 0, n_public = 0, n_all = 0;
        for (const Row& r : arrays_of(1, d)) {
            int cls = -1;
            if (batch_class_count(r.name.c_str(), &cls) != 1) once = false, printf("  %s is classed %d times\n", r.name.c_str(), batch_class_count(r.name.c_str(), &cls));
            n_all++;
        }
#define X(name, T, count) n_secret++;
        BBP_BATCH_SECRET(X)
#undef X
#define X(name, T, count) n_public++;
        BBP_BATCH_PUBLIC(X)
#undef X
        int cls = -1;
        expect(once && n_secret + n_public == n_all && batch_class_count("nosuch", &cls) == 0,
               "every batch array is classed exactly once (" + std::to_string(n_secret) + " secret, " + std::to_string(n_public) + " public)");
        // the counts of the class lists are the layout's own
        bool same = true;
        const BatchStrides st = batch_strides(d);
#define X(name, T, count) if ((u32)(count) != st.name) same = false;
        BBP_BATCH_SECRET(X)
        BBP_BATCH_PUBLIC(X)
#undef X
        expect(same, "the class lists restate the layout's element counts");
    }
    // alignment and tiling
    const uint32_t align_ns[] = {1, 8, 202};
    for (uint32_t N : align_ns) {
        const BatchDims d = dims_of(N);
        bool ok = true;
        for (uint32_t B : {1u, 2u, 3u, 63u, 64u, 65u, 130u, 1024u}) {
            BatchSpans s;
            ok = ok && batch_spans(B, d, -1, s);
            for (int i = 0; i < s.n; i++) ok = ok && s.s[i].off % 256 == 0 && s.s[i].bytes % WIPE_GRAIN == 0;
        }
        expect(ok, "alignment assertions hold for N = " + std::to_string(N));
    }
    const uint32_t cases[][2] = {{3, 1}, {64, 8}, {2, 202}};
    for (auto& c : cases) {
        const uint32_t B = c[0], N = c[1];
        const BatchDims d = dims_of(N);
        const std::vector<Row> arr = arrays_of(B, d);
        const size_t total = batch_offsets(B, d).bytes;
        BatchSpans sec, all;
        bool ok = batch_spans(B, d, SC_SECRET, sec) && batch_spans(B, d, -1, all);
        std::vector<char> secret_byte(total, 0), covered(total, 0), any(total, 0);
        for (const Row& r : arr) {
            int cls = -1;
            batch_class_count(r.name.c_str(), &cls);
            for (size_t i = 0; i < r.bytes; i++) secret_byte[r.off + i] = cls == SC_SECRET ? 1 : 2;
        }
        size_t overlap = 0, outside = 0, on_public = 0;
        for (int i = 0; i < sec.n; i++)
            for (size_t k = 0; k < sec.s[i].bytes; k++) {
                const size_t b = sec.s[i].off + k;
                if (b >= total) {
                    outside++;
                    continue;
                }
                overlap += covered[b];
                covered[b] = 1;
                on_public += secret_byte[b] == 2;
            }
        size_t gap = 0;
        for (size_t b = 0; b < total; b++) gap += secret_byte[b] == 1 && !covered[b];
        for (int i = 0; i < all.n; i++)
            for (size_t k = 0; k < all.s[i].bytes && all.s[i].off + k < total; k++) any[all.s[i].off + k] = 1;
        size_t any_gap = 0;
        for (size_t b = 0; b < total; b++) any_gap += secret_byte[b] != 0 && !any[b];
        ok = ok && !overlap && !outside && !on_public && !gap && !any_gap;
        char buf[200];
        snprintf(buf, sizeof buf, "B = %u, N = %u: %d secret spans tile the secret arrays' rows (gap %zu, overlap %zu, outside %zu, on public rows %zu; all arrays: gap %zu)",
                 B, N, sec.n, gap, overlap, outside, on_public, any_gap);
        expect(ok, buf);
    }
    // scratch discipline: what bbp_debug_poison_scratch leaves alone.  Every exempt name is a buffer of the context, named exactly once
    // in the two buffer lists, with a reason; the list itself is printed for the Python tier to hold against its literal.
    {
        std::vector<std::string> buffers, exempt;
#define X(name, field, count, secret) buffers.push_back(name);
        BBP_CTX_DEVICE_BUFFERS(X, 0, 0, 0)
#undef X
#define X(name, ptr, cap, count, secret) buffers.push_back(name);
        BBP_CTX_PINNED_BUFFERS(X, 0)
#undef X
        bool ok = true, reasons = true;
        std::string list;
#define X(name, reason) exempt.push_back(name), reasons = reasons && strlen(reason) >= 20;
        BBP_POISON_EXEMPT(X)
#undef X
        for (const std::string& e : exempt) {
            const long n = std::count(buffers.begin(), buffers.end(), e);
            if (n != 1) ok = false, printf("  exempt buffer %s is named %ld times in the buffer lists\n", e.c_str(), n);
            if (std::count(exempt.begin(), exempt.end(), e) != 1) ok = false, printf("  %s is exempted more than once\n", e.c_str());
            if (!poison_exempt(e.c_str())) ok = false;
            list += (list.empty() ? "" : " ") + e;
        }
        size_t n_poisoned = 0;
        for (const std::string& b : buffers) n_poisoned += !poison_exempt(b.c_str());
        ok = ok && !poison_exempt("nosuch") && !poison_exempt("") && !poison_exempt("stan") && n_poisoned + exempt.size() == buffers.size();
        expect(ok && reasons, "every poison-exempt buffer is one buffer of the context, exempted once, with a reason (" + std::to_string(n_poisoned) + " of " +
                                  std::to_string(buffers.size()) + " buffers are poisoned)");
        printf("poison exempt: [%s]\n", list.c_str());
    }
    if (g_fail) return 1;
    printf("secret_map_check ok\n");
    return 0;
}
