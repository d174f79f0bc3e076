// Test-only stand-alone program: hc_batch_layout, hc_batch_view, hc_enc_slots and hc_index_lists (tests/host_check.cpp,
// csrc/batch_layout.h, csrc/msm_index.h) over the case grids of tests/test_batch_layout_host.py and tests/test_msm_index_host.py, with
// batches up to 32768, built with -fsanitize=address,undefined (CPU build; __graft_entry__.build_batch_layout_san).  The header's
// offsets end up as pointers into device memory, so its arithmetic is run once where a bad index or an overflow is reported; the totals
// are held against a sum taken in 64 bits throughout (at 32768 proofs an array passes 4 GiB: a 32-bit product would wrap).
#include <stdio.h>

#include "host_check.cpp"

static int fails = 0;
static void expect(bool ok, const char* what, uint32_t B, uint32_t N) {
    if (!ok) {
        fails++;
        printf("FAIL %s B=%u N=%u\n", what, B, N);
    }
}

int main() {
    const uint32_t Ns[] = {1, 8, 202, 0 /* the three widened into one */}, Bs[] = {1, 3, 7, 8, 9, 64, 640, 4095, 4096, 4097, 32768};
    long carves = 0;
    uint32_t wide[4] = {0, 0, 0, 0};
    for (uint32_t N : Ns) {
        uint32_t dims[4];
        if (N) {
            hc_circuit_dims(N, dims);
            for (int i = 0; i < 4; i++) wide[i] = wide[i] > dims[i] ? wide[i] : dims[i];
        } else
            memcpy(dims, wide, sizeof dims);
        const uint64_t m = dims[0], n1 = dims[1], S = sizeof(sc), G = sizeof(ge), T = sizeof(merlin_transcript);
        // bytes per proof of every array, in the order of the carve
        const uint64_t per[30] = {dims[3] * S, m * S, m * S, (1 + 2 * n1) * S, (1 + n1) * S, (1 + 2 * n1) * S, T, T, 32 * S, ((uint64_t)dims[2] + 1) * S, 2049 * S,
                                  2048 * S, 2048 * S, 2048 * S, 2048 * S, m * S, n1 * S, n1 * S, n1 * S, n1 * S, 2048 * S, 2048 * S, 2048 * S, 2048 * S,
                                  2 * 2049 * S, (m + 8) * G, 2 * G, 64 * G, (m + 30) * 32, 32 * m + 32};
        for (uint32_t B : Bs) {
            uint64_t off[64], stride[64], elem[64], total = 0, delta[64];
            char names[512];
            const int n = hc_batch_layout(B, dims, off, stride, elem, &total, names, sizeof names);
            expect(n == 30, "array count", B, N);
            uint64_t end = 0;
            for (int i = 0; i < n && i < 30; i++) {
                expect(off[i] == end && stride[i] * elem[i] == per[i], "offset", B, N);
                end += (per[i] * B + 255) / 256 * 256;
            }
            expect(total == end, "total", B, N);
            for (uint32_t slices = 1; slices <= 4; slices++)
                for (uint32_t i = 0; i <= slices; i++) {
                    const uint32_t first = hc_slice_first(B, slices, i);
                    expect(hc_batch_view(B, dims, first, delta) == n, "view count", B, N);
                    for (int k = 0; k < n && k < 30; k++) expect(delta[k] == off[k] + per[k] * first && delta[k] <= total, "view", B, N);
                }
            carves++;
        }
        uint64_t slots[18];
        hc_enc_slots((uint32_t)m, slots);
        expect(slots[0] * 4 == per[28] && slots[15] + 16 == slots[0] && slots[16] * G == per[25], "encoding slots", 0, N);
    }
    long entries = 0;
    for (uint32_t N : {1u, 8u, 202u}) {
        uint32_t dims[4], n_ai = 0;
        hc_circuit_dims(N, dims);
        const uint32_t want[5] = {1 + 2 * dims[1], 1 + 2 * dims[1], 1 + dims[1], 11 * 2 * 2049, 4098};
        for (int which = 0; which < 5; which++) {
            std::vector<uint32_t> idx(want[which]);
            expect(hc_index_lists(N, which, idx.data(), want[which], &n_ai) == (int)want[which], "list length", (uint32_t)which, N);
            for (uint32_t e : idx) expect(e < TAB_BASES || (which == 0 && e == MSM_SKIP_BASE), "entry inside the tables", (uint32_t)which, N);
            entries += want[which];
        }
        expect(n_ai > 0 && n_ai <= want[0], "n_ai_terms", 0, N);
        std::vector<uint32_t> w(1u << 16);
        for (int which = 0; which < 3; which++) expect(hc_circuit_wires(N, which, w.data(), (uint32_t)w.size()) > 0, "gadget program", (uint32_t)which, N);
    }
    printf("%ld carves, %ld list entries, %d failures\n", carves, entries, fails);
    return fails ? 1 : 0;
}
