// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): csrc/round_select.h -- the selection rules, the compare helpers,
// the screening and the per-bid score record -- driven by a command file that tests/test_round_select_host.py writes, one command per
// line, every value in hex as the bytes travel (little-endian):
//   select B K floor32          then B lines "status score32"      -> "sel n_sel n_qualified i0 i1 ..."
//   score N B table bids mimc90                                    -> B lines "rec status toggle q32"; every record is also held against
//                                                                     round_bid_eval's (same status, toggle and q)
//   screen N B                                                     -> "screen rc done"
// and, with no command at all, self-checks of the helpers and of the staging layouts.  Ends with "round_select_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/round_select.h"

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
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}

static void self_checks() {
    u32 a[8] = {0, 0, 0, 0, 0, 0, 0, 1}, b[8] = {0xffffffffu, 0, 0, 0, 0, 0, 0, 0};
    CHECK(rs_ge256(a, b) && !rs_ge256(b, a) && rs_ge256(a, a));  // the most significant word decides
    CHECK(rs_cmp_top(a, b, 32) == 1 && rs_cmp_top(b, a, 32) == -1 && rs_cmp_top(a, a, 32) == 0);
    CHECK(rs_cmp_top(a, b, 0) == 0 && rs_cmp_top(a, b, 3) == 0 && rs_cmp_top(a, b, 4) == 1);  // byte 3 is word 7's lowest
    u32 c[8] = {0x04030201u, 0, 0, 0, 0, 0, 0, 0xa0b0c0d0u};
    CHECK(rs_key_byte(c, 0) == 0xa0 && rs_key_byte(c, 3) == 0xd0 && rs_key_byte(c, 28) == 0x04 && rs_key_byte(c, 31) == 0x01);
    u32 lo1[8] = {5, 0, 0, 0, 0, 0, 0, 7}, lo2[8] = {6, 0, 0, 0, 0, 0, 0, 7};
    for (u32 nb = 0; nb <= 32; nb++) CHECK(rs_cmp_top(lo1, lo2, nb) == (nb == 32 ? -1 : 0));
    uint8_t f[32] = {};
    f[0] = 0x11, f[31] = 0x80;
    const RsFloor fl = rs_floor_load(f);
    CHECK(fl.w[0] == 0x11 && fl.w[7] == 0x80000000u);
    for (u32 B : {1u, 255u, 256u, 1024u, 1025u, 1100u, 65536u, 262143u, 262145u, 1u << 20}) {  // every bid belongs to exactly one workgroup
        const RsGeom g = rs_geom(B);
        CHECK(g.G >= 1 && g.G <= RS_SEL_G_MAX && g.span % RS_SEL_T == 0 && (unsigned long long)g.G * g.span >= B);
        CHECK(B <= 4 * RS_SEL_T ? g.G == 1 : g.G > 1);
    }
    // layouts: regions in order, inside the buffer, 256-aligned
    for (u32 N : {1u, 8u, 202u})
        for (u32 B : {1u, 70u, 1u << 20})
            for (u32 cap : {0u, 1u, 64u}) {
                const u32 cp = cap < B ? cap : B;
                const SelectScratch s = select_scratch(B, cp, N);
                CHECK(s.rs.rb >= s.rs.rblk + round_table_bytes(N) && s.state >= s.rs.rb + 4 * (size_t)RB_WORDS * cp && s.recs >= s.state + sizeof(RsState));
                CHECK(s.gbids >= s.recs + 4 * (size_t)RS_WORDS * B && s.end >= s.gbids + ROUND_BID_BYTES * cp && s.recs % 256 == 0 && s.gbids % 256 == 0);
                for (bool sc_ : {false, true}) {
                    const SelectStaging L(B, cp, N, sc_);
                    CHECK(L.tab >= ROUND_BID_BYTES * B && L.up_bytes == L.tab + round_table_bytes(N) && L.counts >= L.up_bytes);
                    CHECK(L.sel >= L.counts + 8 && L.status >= L.sel + 4 * (size_t)cp && L.scores >= L.status + 4 * (size_t)B);
                    CHECK(L.counts + L.down_bytes == L.scores + (sc_ ? 32 * (size_t)B : 0) && L.scratch >= L.counts + L.down_bytes);
                    CHECK(L.bytes == L.scratch + L.ss.end && L.h_bytes == L.up_bytes + L.down_bytes && L.scratch % 256 == 0);
                }
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
        if (cmd == "select") {
            u32 B, K;
            std::string fh;
            ls >> B >> K >> fh;
            const RsFloor floor = rs_floor_load(unhex(fh).data());
            std::vector<u32> recs((size_t)RS_WORDS * B, 0), sel(B ? B : 1);
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                u32 st;
                std::string sh;
                rs_ >> st >> sh;
                const std::vector<uint8_t> sb = unhex(sh);
                for (int w = 0; w < 8; w++) recs[(size_t)RS_WORDS * i + RS_Q + w] = rb_le32(sb.data() + 4 * w);
                recs[(size_t)RS_WORDS * i + RS_STATUS] = st;
            }
            u32 n_sel = 0, n_q = 0;
            round_select_host(B, recs.data(), floor.w, K, sel.data(), &n_sel, &n_q);
            printf("sel %u %u", n_sel, n_q);
            for (u32 j = 0; j < n_sel; j++) printf(" %u", sel[j]);
            printf("\n");
        } else if (cmd == "score") {
            u32 N, B;
            std::string th, bh, mh;
            ls >> N >> B >> th >> bh >> mh;
            const std::vector<uint8_t> table = unhex(th), bids = unhex(bh), mimc = unhex(mh);
            std::vector<sc> c(BBP_MIMC_ROUNDS), rblk(1 + (size_t)N);
            memcpy(c.data(), mimc.data(), 32 * BBP_MIMC_ROUNDS);
            u32 w[8];
            memcpy(w, table.data(), 32);
            const int32_t flag = sc_is_canonical(w) ? BBP_OK : BBP_ERR_FORMAT;
            rblk[0] = sc_reduce256(w);
            for (u32 i = 0; i < N; i++) {
                memcpy(w, table.data() + 32 * (1 + (size_t)i), 32);
                rblk[1 + i] = sc_from_bits(w);
            }
            for (u32 p = 0; p < B; p++) {
                u32 r[RS_WORDS], full[RB_WORDS];
                round_score_eval(N, bids.data() + BBP_ROUND_BID_BYTES * (size_t)p, rblk.data(), flag, c.data(), r);
                round_bid_eval(N, bids.data() + BBP_ROUND_BID_BYTES * (size_t)p, rblk.data(), flag, c.data(), full);
                CHECK(r[RS_STATUS] == full[RB_STATUS] && r[RS_TOGGLE] == full[RB_TOGGLE] && !memcmp(r + RS_Q, full + RB_Q, 32));
                uint8_t q[32];
                for (int i = 0; i < 32; i++) q[i] = (uint8_t)(r[RS_Q + i / 4] >> (8 * (i & 3)));
                printf("rec %u %u %s\n", r[RS_STATUS], r[RS_TOGGLE], hex(q, 32).c_str());
            }
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
    printf("round_select_check ok\n");
    return 0;
}
