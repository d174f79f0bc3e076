// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): csrc/round_best.h -- the rules of bbp_verify_round_best
// (round_best_host), the key screening, the tranche sizes, the ranking of (key, index) pairs and the staging layouts -- driven by a
// command file that tests/test_round_best_host.py writes, one command per line, every value in hex as the bytes travel (little-endian):
//   best B K tranche cap floor32   then B lines "verdict key32"   -> "best n_best n_candidates n_examined | best... | status..."
//   key key32 floor32                                             -> "key status"   (0: a candidate)
//   rank n cap                     then n lines "index key32"     -> "rank i0 i1 ..."
//   screen N B                                                    -> "screen rc done"
// and, with no command at all, self-checks of the helpers and of the layouts.  Ends with "round_best_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/round_best.h"

using namespace bbp;

static int failures = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            failures++;                                          \
        }                                                        \
    } while (0)

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return v;
}
static void load_key(const std::string& h, u32* w) {
    const std::vector<uint8_t> b = unhex(h);
    for (int i = 0; i < 8; i++) w[i] = rb_le32(b.data() + 4 * i);
}

static void self_checks() {
    CHECK(BBP_ROW_SKIPPED == -1 && BBP_ROW_SKIPPED != BBP_OK && BBP_ROW_SKIPPED != BBP_ERR_VERIFY && BBP_ROW_SKIPPED != BBP_ERR_FORMAT);
    // tranche sizes: T_0 = max(tranche, K), the default for 0, every candidate for K == 0; T_t doubles and is clamped to what is left
    CHECK(best_tranche0(1, 0, 9) == BBP_BEST_TRANCHE_DEFAULT && best_tranche0(3, 1, 9) == 3 && best_tranche0(3, 8, 9) == 8 && best_tranche0(0, 8, 9) == 9);
    CHECK(best_tranche_rows(4, 0, 100) == 4 && best_tranche_rows(4, 3, 100) == 32 && best_tranche_rows(4, 5, 100) == 100);
    CHECK(best_tranche_rows(1u << 20, 30, 0xffffffffu) == 0xffffffffu && best_tranche_rows(1u << 20, 40, 7) == 7);
    // the bound: the least t with T_0 (2^t - 1) >= n
    for (u32 T0 : {1u, 3u, 4u, 64u, 1000u})
        for (u32 n : {0u, 1u, 2u, 3u, 4u, 5u, 63u, 64u, 65u, 1025u, 5000u, 1u << 20}) {
            u32 t = 0;
            while ((unsigned long long)T0 * ((1ull << t) - 1) < n) t++;
            CHECK(best_max_tranches(n, T0) == t);
        }
    // a record that has left its array does not qualify, under any floor
    u32 rec[RS_WORDS] = {}, zero[8] = {};
    rec[RS_STATUS] = BEST_OUT;
    CHECK(!rs_qualifies(rec, zero));
    rec[RS_STATUS] = (u32)BBP_OK;
    CHECK(rs_qualifies(rec, zero));
    // layouts: regions in order, none overlapping, 256-aligned; counts and sel keep their distance in the mirror (one copy fetches both)
    for (u32 B : {1u, 63u, 70u, 5000u, 1u << 20})
        for (bool hk : {false, true}) {
            const BestLayout L(B, hk);
            const size_t b = B;
            CHECK(L.ctr == 0 && L.counts >= L.ctr + 16 && L.sel >= L.counts + 8 && L.state >= L.sel + 4 * b && L.keys >= L.state + sizeof(RsState));
            CHECK(L.recs >= L.keys + (hk ? 32 * b : 0) && L.win >= L.recs + 4 * (size_t)RS_WORDS * b && L.status >= L.win + 4 * (size_t)RS_WORDS * b);
            CHECK(L.tstat >= L.status + 4 * b && L.pairs >= L.tstat + 4 * b && L.bytes >= L.pairs + 4 * (size_t)BEST_PAIR_WORDS * b);
            for (size_t o : {L.counts, L.sel, L.state, L.keys, L.recs, L.win, L.status, L.tstat, L.pairs, L.h_tstat, L.h_ctr, L.h_counts, L.h_sel, L.h_pairs, L.h_status})
                CHECK(o % 256 == 0);
            CHECK(L.h_tstat >= L.h_keys + (hk ? 32 * b : 0) && L.h_ctr >= L.h_tstat + 4 * b && L.h_counts >= L.h_ctr + 8);
            CHECK(L.h_sel - L.h_counts == L.sel - L.counts && L.h_pairs >= L.h_sel + 4 * b && L.h_status >= L.h_pairs + 4 * (size_t)BEST_PAIR_WORDS * b);
            CHECK(L.h_bytes >= L.h_status + 4 * b);
        }
    for (u32 N : {1u, 8u, 202u})
        for (u32 n : {1u, 5u, 64u, 8192u}) {
            const BestRows R(n, N);
            CHECK(round_row_bytes(N) == 1313 + 32 * (size_t)N && proof_record_bytes(N) + 64 == round_row_bytes(N));  // the key: 32 bytes at the record's end
            CHECK(R.rows == 0 && R.ent >= round_row_bytes(N) * n && R.ent % 256 == 0 && R.bytes >= R.ent + 32 * (size_t)n);
        }
}

int main(int argc, char** argv) {
    self_checks();
    std::ifstream in;
    if (argc > 1) in.open(argv[1]);
    std::string line;
    while (argc > 1 && std::getline(in, line)) {
        std::istringstream ls(line);
        std::string cmd;
        ls >> cmd;
        if (cmd == "best") {
            u32 B, K, tranche, cap;
            std::string fh;
            ls >> B >> K >> tranche >> cap >> fh;
            u32 floor[8];
            load_key(fh, floor);
            std::vector<u32> keys(8 * (size_t)B + 8), best(cap);  // (exactly cap entries: ASan sees a write beyond them)
            std::vector<int32_t> verdicts(B), status(B, 77);
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh;
                rs_ >> verdicts[i] >> kh;
                load_key(kh, &keys[8 * (size_t)i]);
            }
            u32 nb = 0, nc = 0, ne = 0;
            round_best_host(B, keys.data(), verdicts.data(), floor, K, tranche, cap, best.data(), &nb, &nc, &ne, status.data());
            printf("best %u %u %u |", nb, nc, ne);
            for (u32 j = 0; j < nb && j < cap; j++) printf(" %u", best[j]);
            printf(" |");
            for (u32 i = 0; i < B; i++) printf(" %d", status[i]);
            printf("\n");
            // ... and the bound on the tranches, through n_examined: no more rows than the bound's tranches hold
            const u32 T0 = best_tranche0(K, tranche, nc);
            unsigned long long most = 0;
            for (u32 t = 0; t < best_max_tranches(nc, T0); t++) most += best_tranche_rows(T0, t, 0xffffffffu);
            CHECK(ne <= nc && (nc == 0 || most >= nc));
        } else if (cmd == "key") {
            std::string kh, fh;
            ls >> kh >> fh;
            u32 k[8], f[8];
            load_key(kh, k), load_key(fh, f);
            printf("key %d\n", best_screen_key(k, f));
        } else if (cmd == "rank") {
            u32 n, cap;
            ls >> n >> cap;
            std::vector<u32> pairs((size_t)BEST_PAIR_WORDS * n + 1), out(cap);
            for (u32 j = 0; j < n; j++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh;
                rs_ >> pairs[(size_t)BEST_PAIR_WORDS * j + 8] >> kh;
                load_key(kh, &pairs[(size_t)BEST_PAIR_WORDS * j]);
            }
            best_rank_pairs(n, pairs.data(), cap, out.data());
            printf("rank");
            for (u32 j = 0; j < n && j < cap; j++) printf(" %u", out[j]);
            printf("\n");
        } else if (cmd == "screen") {
            u32 N, B;
            ls >> N >> B;
            bool done = false;
            const int32_t rc = round_select_screen(N, B, &done);
            printf("screen %d %d\n", rc, done ? 1 : 0);
        } else if (!cmd.empty()) {
            printf("FAILED unknown command %s\n", cmd.c_str());
            failures++;
        }
    }
    if (failures) return 1;
    printf("round_best_check ok\n");
    return 0;
}
