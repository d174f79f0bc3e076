// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): csrc/standings.h on the host -- the rule of one offer to many
// standings (standings_offer_host over S StandingStates), the per-step plan and the layout -- driven by a command file that
// tests/test_standings_host.py writes, one command per line, every 32-byte value in hex as the bytes travel (little-endian):
//   standings S                 then S lines "K floor32": S fresh standings replace the current ones
//   offer B tranche cap         then one line of S table_log2 values, then B lines "standing verdict key32 id32": one offer
//        -> "offer rc n_steps", then per standing "s n_entered n_candidates n_examined n_duplicates offered | entered... | serial:key32:id32 ..."
//           (the entries after the offer), then "status ..."
// and, with no command at all, self-checks of the helpers and of the layout.  Ends with "standings_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/standings.h"

using namespace bbp;

static int failures = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            failures++;                                          \
        }                                                        \
    } while (0)

static void load_key(const std::string& h, u32* w) {
    uint8_t b[32] = {};
    for (size_t i = 0; i < 32 && 2 * i + 1 < h.size(); i++) b[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    for (int i = 0; i < 8; i++) w[i] = rb_le32(b + 4 * i);
}
static std::string hex_key(const u32* w) {
    char s[65];
    for (int b = 0; b < 32; b++) snprintf(s + 2 * b, 3, "%02x", (unsigned)((w[b >> 2] >> (8 * (b & 3))) & 0xffu));
    return s;
}
static bool same(const StandingState& a, const StandingState& b) {
    return a.K == b.K && a.offered == b.offered && a.keys == b.keys && a.ids == b.ids && a.serials == b.serials && memcmp(a.floor, b.floor, 32) == 0;
}

static void self_checks() {
    // the per-step plan: tranche t of the live candidates, T_0 = max(tranche, K), no stop at K, nothing once none is live
    CHECK(stands_take(3, 0, 0, 100, 0, 0, 0) == BBP_BEST_TRANCHE_DEFAULT && stands_take(3, 1, 0, 100, 0, 0, 0) == 3 && stands_take(3, 1, 2, 100, 9, 0, 0) == 12);
    CHECK(stands_take(1024, 1, 0, 5000, 0, 0, 0) == 1024 && stands_take(1, 1, 3, 10, 7, 1, 1) == 1 && stands_take(1, 1, 3, 10, 7, 2, 1) == 0);
    CHECK(stands_take(1, 1, 40, 0xffffffffu, 0, 0, 0) == 0xffffffffu && stands_take(2, 5, 0, 3, 1, 1, 2) == 0);
    CHECK(STANDS_H_STRIDE >= STAND_H_WORDS && STANDS_P_WORDS > STANDS_P_SERIALS);
    // the layout: every span 256-aligned, in order, none overlapping, behind the one-per-bidder state of the working rows
    for (u32 S : {2u, 3u, 64u})
        for (u32 K : {1u, 3u, 1024u})
            for (u32 B : {1u, 130u, 1u << 20}) {
                const u32 sumK = S * K, W = sumK + B;
                const BestsLayout L(W, S, false);
                const BestsDistinctLayout D(L, W, S, 0, true);
                const StandingsLayout X(D, S, sumK, B);
                const size_t dev[] = {X.sctr, X.par, X.whdr, X.wserial, X.order, X.local, X.bytes};
                const size_t dev_need[] = {4 * (size_t)S, 4 * (size_t)STANDS_P_WORDS * S, 4 * (size_t)STANDS_H_STRIDE * S, 8 * (size_t)sumK, 4 * (size_t)sumK, 4 * (size_t)B};
                CHECK(dev[0] >= D.bytes);
                for (int k = 0; k < 6; k++) CHECK(dev[k] % 256 == 0 && dev[k + 1] >= dev[k] + dev_need[k]);
                const size_t pin[] = {X.h_sctr, X.h_par, X.h_local, X.h_whdr, X.h_order, X.h_bytes};
                const size_t pin_need[] = {4 * (size_t)S, 4 * (size_t)STANDS_P_WORDS * S, 4 * (size_t)B, 4 * (size_t)STANDS_H_STRIDE * S, 4 * (size_t)sumK};
                CHECK(pin[0] >= D.h_bytes);
                for (int k = 0; k < 5; k++) CHECK(pin[k] % 256 == 0 && pin[k + 1] >= pin[k] + pin_need[k]);
                CHECK(D.slots > W || D.log2 == BEST_TABLE_LOG2_MAX);  // a slot more than there are working rows ...
            }
    CHECK((1ull << BEST_TABLE_LOG2_MAX) > (unsigned long long)BBP_STANDING_MAX_OPEN * BBP_STANDING_MAX_K + BBP_SELECT_MAX_BIDS);  // ... at the largest call too
    // an offer of no rows changes nothing and reports zeros, for every standing
    std::vector<StandingState> st(3);
    for (u32 s = 0; s < 3; s++) st[s].K = 2 + s;
    u32 ne[3] = {9, 9, 9}, nc[3] = {9, 9, 9}, nx[3] = {9, 9, 9}, nd[3] = {9, 9, 9}, steps = 9;
    CHECK(standings_offer_host(3, st.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, ne, nc, nx, nd, &steps, nullptr) == BBP_OK);
    for (u32 s = 0; s < 3; s++) CHECK(ne[s] == 0 && nc[s] == 0 && nx[s] == 0 && nd[s] == 0 && st[s].count() == 0 && st[s].offered == 0);
    CHECK(steps == 0);
}

int main(int argc, char** argv) {
    self_checks();
    std::ifstream in;
    if (argc > 1) in.open(argv[1]);
    std::string line;
    std::vector<StandingState> st;
    while (argc > 1 && std::getline(in, line)) {
        std::istringstream ls(line);
        std::string cmd;
        ls >> cmd;
        if (cmd == "standings") {
            u32 S;
            ls >> S;
            st.assign(S, StandingState{});
            for (u32 s = 0; s < S; s++) {
                std::getline(in, line);
                std::istringstream ss(line);
                std::string fh;
                ss >> st[s].K >> fh;
                load_key(fh, st[s].floor);
            }
        } else if (cmd == "offer") {
            const u32 S = (u32)st.size();
            u32 B, tranche, cap;
            ls >> B >> tranche >> cap;
            std::vector<u32> log2(S), of(B), keys(8 * (size_t)B), ids(8 * (size_t)B), entered((size_t)S * cap, 0xabababab);  // (exactly S x cap entries: ASan sees a write beyond)
            std::vector<int32_t> verdicts(B), status(B, 77);
            std::getline(in, line);
            std::istringstream lg(line);
            for (u32 s = 0; s < S; s++) lg >> log2[s];
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh, ih;
                rs_ >> of[i] >> verdicts[i] >> kh >> ih;
                load_key(kh, &keys[8 * (size_t)i]), load_key(ih, &ids[8 * (size_t)i]);
            }
            std::vector<u32> ne(S), nc(S), nx(S), nd(S);
            u32 steps = 0;
            const std::vector<StandingState> before = st;
            const int32_t rc = standings_offer_host(S, st.data(), B, of.data(), keys.data(), ids.data(), verdicts.data(), tranche, cap, entered.data(), ne.data(), nc.data(),
                                                    nx.data(), nd.data(), &steps, status.data(), log2.data());
            if (rc)
                for (u32 s = 0; s < S; s++) CHECK(same(st[s], before[s]));  // BBP_ERR_INTERNAL in any standing: no state changes
            printf("offer %d %u\n", rc, steps);
            for (u32 s = 0; s < S; s++) {
                printf("%u %u %u %u %u %llu |", s, ne[s], nc[s], nx[s], nd[s], st[s].offered);
                for (u32 j = 0; !rc && j < ne[s] && j < cap; j++) printf(" %u", entered[(size_t)s * cap + j]);
                for (u32 j = rc ? 0 : ne[s]; j < cap; j++) CHECK(rc || entered[(size_t)s * cap + j] == 0xabababab);  // entries beyond are not written
                printf(" |");
                for (u32 e = 0; e < st[s].count(); e++)
                    printf(" %llu:%s:%s", st[s].serials[e], hex_key(&st[s].keys[8 * (size_t)e]).c_str(), hex_key(&st[s].ids[8 * (size_t)e]).c_str());
                printf("\n");
                CHECK(rc || ((unsigned long long)nx[s] + nd[s] <= nc[s] && st[s].count() <= st[s].K));
            }
            printf("status");
            for (u32 i = 0; i < B; i++) printf(" %d", status[i]);
            printf("\n");
        } else if (!cmd.empty()) {
            printf("FAILED unknown command %s\n", cmd.c_str());
            failures++;
        }
    }
    if (failures) return 1;
    printf("standings_check ok\n");
    return 0;
}
