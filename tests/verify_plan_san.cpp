// Test-only stand-alone program: hc_verify_plan and hc_verify_staging (tests/host_check.cpp, csrc/verify_plan.h) over the case grid of
// tests/test_verify_plan_host.py, built with -fsanitize=address,undefined (CPU build; __graft_entry__.build_verify_plan_san).  The
// header's offsets end up as pointers into device scratch, so its arithmetic is run once where a bad index or an overflow is reported.
#include <stdio.h>

#include "host_check.cpp"

static int fails = 0;
static void expect(bool ok, const char* what, uint32_t B, uint32_t G) {
    if (!ok) {
        fails++;
        printf("FAIL %s B=%u G=%u\n", what, B, G);
    }
}

int main() {
    const uint32_t Bs[] = {1, 2, 32, 33, 64, 65, 4095, 4096, 4097, 32768}, Gs[] = {0, 2, 8, 64}, mix[] = {1, 8, 202};
    const uint32_t round_sets[][3] = {{8, 0, 0}, {8, 8, 0}, {1, 202, 0}, {8, 8, 8}, {1, 8, 202}};
    const uint32_t n_rounds[] = {1, 2, 2, 3, 3};
    long plans = 0;
    for (uint32_t B : Bs) {
        std::vector<uint32_t> ns(B), of(B);
        std::vector<uint8_t> vers(B, 0);
        vers[B - 1] = 1;
        for (uint32_t i = 0; i < B; i++) ns[i] = mix[i % 3];
        uint32_t dims[12];
        for (int i = 0; i < 3; i++) {
            const uint32_t N = mix[i], n_mul = 1442 + 3 * N;
            dims[4 * i] = 4 + N, dims[4 * i + 1] = n_mul, dims[4 * i + 2] = 2 * n_mul + 3 + 3 * N, dims[4 * i + 3] = 100 + N;
        }
        for (uint32_t G : Gs) {
            int64_t geo[54];
            uint64_t lay[39], st[13];
            uint32_t rd_off[4];
            const char* knobs[] = {"BBP_VARBASE_V1", "1", "BBP_VARBASE_LANES", "1000"};
            for (int kn = 0; kn <= 2; kn++) {
                for (int ver = 0; ver < 2; ver++) {
                    expect(hc_verify_plan(knobs, kn, 0, B, 8, ver, nullptr, nullptr, 0, nullptr, nullptr, dims + 4, 1, ver ? 0 : G, 32, geo, lay, rd_off) == 0, "uniform", B, G);
                    expect(hc_verify_plan(knobs, kn, 1, B, 0, 0, ns.data(), ver ? vers.data() : nullptr, 0, nullptr, nullptr, dims, 3, ver ? 0 : G, 32, geo, lay, rd_off) == 0,
                           "mixed", B, G);
                    expect(lay[24] >= lay[12] + lay[13], "misc total", B, G);
                    plans += 2;
                }
                for (int r = 0; r < 5; r++) {
                    for (uint32_t i = 0; i < B; i++) of[i] = i % n_rounds[r];
                    for (int with_of = (n_rounds[r] == 1 ? 0 : 1); with_of < 2; with_of++) {
                        expect(hc_verify_plan(knobs, kn, 2, B, 0, 0, nullptr, nullptr, n_rounds[r], round_sets[r], with_of ? of.data() : nullptr, dims, 3, G, 32, geo, lay,
                                              rd_off) == 0, "rounds", B, G);
                        expect(geo[17] == 0 && (uint32_t)geo[15] == rd_off[n_rounds[r]], "round offsets", B, G);
                        plans++;
                    }
                    hc_verify_staging(2, B, 0, 0, nullptr, nullptr, n_rounds[r], round_sets[r], of.data(), G, 32, r & 1, 32768, st);
                    expect(st[1] >= st[0] && st[5] == 4 * ((uint64_t)B + 1), "rounds staging", B, G);
                }
            }
            for (uint32_t chunk : {1u, 14u, 16u, 32768u}) {
                if (chunk == 1 && B > 4097) continue;
                hc_verify_staging(1, B, 0, 0, ns.data(), vers.data(), 0, nullptr, nullptr, G, 2, 1, chunk, st);
                expect(st[7] == 0 && st[8] * st[9] >= B && st[9] <= chunk, "mixed two-phase staging", B, G);
                hc_verify_staging(0, B, 202, 0, nullptr, nullptr, 0, nullptr, nullptr, G, 2, 0, chunk, st);
                expect(st[7] == (G ? G : B >= 4 ? 2u : 0u), "uniform staging group", B, G);
            }
        }
    }
    // the round-table limit on synthetic round lengths: nothing is allocated from a plan
    const uint32_t big[][3] = {{0x7ffffffeu, 0, 0}, {0x7fffffffu, 0, 0}, {0x3fffffffu, 0x3fffffffu, 0}, {0xfffffffeu, 0xfffffffeu, 0xfffffffeu}};
    const uint32_t big_n[] = {1, 1, 2, 3}, want[] = {0, 1, 1, 1}, of2[] = {0, 0}, d8[] = {12, 1466, 2959, 108};
    for (int i = 0; i < 4; i++) {
        int64_t geo[54];
        uint64_t lay[39];
        uint32_t rd_off[4];
        expect(hc_verify_plan(nullptr, 0, 2, 2, 0, 0, nullptr, nullptr, big_n[i], big[i], of2, d8, 1, 0, 32, geo, lay, rd_off) == 0 && geo[17] == want[i], "round table limit",
               (uint32_t)i, 0);
    }
    printf("%ld plans, %d failures\n", plans, fails);
    return fails ? 1 : 0;
}
