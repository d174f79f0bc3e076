// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): csrc/rounds_best.h -- the rules of bbp_verify_rounds_best
// (rounds_best_host), the extended-key comparison, the radix select as the kernel runs it pass by pass (bests_select_host), the
// per-step plan, the state layout and the screening order -- driven by a command file that tests/test_rounds_best_host.py writes, one
// command per line, every key in hex as the bytes travel (little-endian):
//   bests R B K tranche cap has_floors   then (has_floors) R lines "floor32", then B lines "round verdict key32"
//                                        -> "bests n_steps|nb nc ne best...|... (R parts)|#|status..."
//   screen R B ns,.. ro,..|-             -> "screen rc done"
// and, with no command at all, self-checks of the helpers, the select and the layout.  Ends with "rounds_best_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/rounds_best.h"

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
static std::vector<u32> split_u32(const std::string& s) {
    std::vector<u32> v;
    std::istringstream ss(s);
    std::string part;
    while (std::getline(ss, part, ',')) v.push_back((u32)strtoul(part.c_str(), nullptr, 10));
    return v;
}

// the extended key byte by byte against the comparison the rules use
static void check_ext(const u32* qa, u32 ia, const u32* qb, u32 ib) {
    int c = 0;
    for (u32 pos = 0; pos < BESTS_EXT_BYTES && !c; pos++) {
        const u32 x = bests_ext_byte(qa, ia, pos), y = bests_ext_byte(qb, ib, pos);
        CHECK(x < 256 && y < 256);
        c = x > y ? 1 : x < y ? -1 : 0;
    }
    u32 keys[16];
    memcpy(keys, qa, 32), memcpy(keys + 8, qb, 32);
    const bool before = rs_cmp_top(qa, qb, 32) ? rs_cmp_top(qa, qb, 32) > 0 : ia < ib;  // key descending, index ascending
    CHECK((c > 0) == before || (ia == ib && c == 0));
    CHECK(bests_ext_before(qa, ia, qb, ib) == (c > 0));
    // a pivot built byte by byte from b: a >= pivot exactly when a is not behind b; every prefix of b matches it
    u32 piv[BESTS_PIV_WORDS] = {};
    for (u32 pos = 0; pos < BESTS_EXT_BYTES; pos++) {
        CHECK(bests_prefix_eq(qb, ib, piv, pos));
        bests_piv_set(piv, pos, bests_ext_byte(qb, ib, pos));
    }
    CHECK(bests_prefix_eq(qb, ib, piv, BESTS_EXT_BYTES) && bests_ext_ge(qb, ib, piv));
    CHECK(bests_ext_ge(qa, ia, piv) == (c >= 0));
    u32 same = 0;
    while (same < BESTS_EXT_BYTES && bests_ext_byte(qa, ia, same) == bests_ext_byte(qb, ib, same)) same++;
    for (u32 p = 0; p <= BESTS_EXT_BYTES; p++) CHECK(bests_prefix_eq(qa, ia, piv, p) == (p <= same));
}

static void self_checks() {
    std::mt19937 rnd(11);
    // extended keys: random, equal keys (the index alone decides), keys that differ in one byte only, indices at the ends of the range
    for (int n = 0; n < 400; n++) {
        u32 a[8], b[8];
        for (int w = 0; w < 8; w++) a[w] = rnd(), b[w] = n % 3 ? a[w] : rnd();
        if (n % 3 == 2) b[rnd() % 8] ^= 1u << (rnd() % 32);
        const u32 ends[] = {0, 1, 255, 256, 65535, 65536, BBP_SELECT_MAX_BIDS - 1, 0xffffffffu};
        const u32 ia = n % 2 ? rnd() : ends[rnd() % 8], ib = n % 5 ? rnd() : ia;
        check_ext(a, ia, b, ib);
    }
    // the bin of a pass: from the top, the first bin at which `want` members are reached
    {
        u32 hist[256] = {}, bin = 7, left = 0;
        hist[200] = 3, hist[17] = 2, hist[0] = 1;
        CHECK(bests_pick_bin(hist, 1, &bin, &left) && bin == 200 && left == 1);
        CHECK(bests_pick_bin(hist, 3, &bin, &left) && bin == 200 && left == 3);
        CHECK(bests_pick_bin(hist, 4, &bin, &left) && bin == 17 && left == 1);
        CHECK(bests_pick_bin(hist, 6, &bin, &left) && bin == 0 && left == 1);
        CHECK(!bests_pick_bin(hist, 7, &bin, &left));
    }
    // the select, as the kernel runs it, over segments in shuffled order: members of several rounds share the record array; closed
    // records are no members; equal keys, keys equal on 31 bytes
    for (int n = 0; n < 60; n++) {
        const u32 B = 1 + rnd() % 300;
        std::vector<u32> recs((size_t)RS_WORDS * B), seg;
        for (u32 i = 0; i < B; i++) {
            u32* r = &recs[(size_t)RS_WORDS * i];
            for (int w = 0; w < 8; w++) r[RS_Q + w] = n % 4 == 0 ? 5u : n % 4 == 1 ? (w ? 9u : rnd() % 256) : rnd();
            r[RS_STATUS] = rnd() % 4 ? (u32)BBP_OK : BEST_OUT;
            r[RS_TOGGLE] = 0;
            if (rnd() % 3) seg.push_back(i);  // (the others: rows of another round)
        }
        std::shuffle(seg.begin(), seg.end(), rnd);
        std::vector<u32> open;
        for (u32 i : seg)
            if (recs[(size_t)RS_WORDS * i + RS_STATUS] == (u32)BBP_OK) open.push_back(i);
        std::sort(open.begin(), open.end(), [&](u32 a, u32 b) { return bests_ext_before(&recs[(size_t)RS_WORDS * a], a, &recs[(size_t)RS_WORDS * b], b); });
        for (u32 take : {0u, 1u, 2u, (u32)open.size() / 2, (u32)open.size(), (u32)open.size() + 3}) {
            std::vector<u32> out(take, 0xeeeeeeeeu);  // exactly take entries: ASan sees a write beyond them
            const u32 got = bests_select_host((u32)seg.size(), seg.data(), recs.data(), take, out.data());
            const u32 want = take < open.size() ? take : (u32)open.size();
            CHECK(got == want);
            std::vector<u32> a(out.begin(), out.begin() + got), b(open.begin(), open.begin() + want);
            std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
            CHECK(a == b);
        }
    }
    // the plan of a step: nothing once K rows hold or no candidate is left, else the single-round tranche
    CHECK(bests_take(1, 4, 0, 10, 0, 0) == 4 && bests_take(1, 4, 1, 10, 4, 0) == 6 && bests_take(1, 4, 1, 10, 4, 1) == 0 && bests_take(1, 4, 2, 10, 10, 0) == 0);
    CHECK(bests_take(0, 4, 0, 10, 0, 0) == 10 && bests_take(0, 4, 1, 10, 10, 10) == 0 && bests_take(3, 1, 0, 2, 0, 0) == 2 && bests_take(1, 0, 0, 100, 0, 0) == 16);
    CHECK(bests_take(1, 1, 0, 0, 0, 0) == 0);
    CHECK(bests_winners(0, 7) == 7 && bests_winners(3, 7) == 3 && bests_winners(3, 2) == 2 && bests_winners(3, 0) == 0);
    // the layout: regions in order, 256-aligned, non-overlapping, monotonic in B and R; the counter block holds its eight parts
    size_t last_bytes = 0, last_h = 0;
    for (u32 R : {1u, 2u, 64u, 257u, 1000u, BBP_BEST_MAX_ROUNDS})
        for (u32 B : {1u, 63u, 1000u, 5000u, 1u << 20})
            for (bool hk : {false, true}) {
                const BestsLayout L(B, R, hk);
                const size_t b = B, r = R;
                const size_t dev[] = {L.ctr, L.offb, L.floors, L.rb, L.round_of, L.rowoff, L.cand, L.sel, L.keys, L.recs, L.win, L.status, L.tstat, L.pairs, L.bytes};
                const size_t need[] = {4 * (8 * r + 2), 8 * (r + 1), 32 * r, 4 * r, 4 * b, hk ? 0 : 8 * b, 4 * b, 4 * b, hk ? 32 * b : 0, 4 * (size_t)RS_WORDS * b,
                                       4 * (size_t)RS_WORDS * b, 4 * b, 4 * b, 4 * (size_t)BEST_PAIR_WORDS * b};
                for (int k = 0; k < 14; k++) CHECK(dev[k] % 256 == 0 && dev[k + 1] >= dev[k] + need[k]);
                const size_t pin[] = {L.h_floors, L.h_rb, L.h_round_of, L.h_rowoff, L.h_keys, L.h_tstat, L.h_ctr, L.h_sel, L.h_pairs, L.h_status, L.h_bytes};
                const size_t hneed[] = {32 * r, 4 * r, 4 * b, hk ? 0 : 8 * b, hk ? 32 * b : 0, 4 * b, 4 * (8 * r + 2), 4 * b, 4 * (size_t)BEST_PAIR_WORDS * b, 4 * b};
                for (int k = 0; k < 10; k++) CHECK(pin[k] % 256 == 0 && pin[k + 1] >= pin[k] + hneed[k]);
                CHECK(L.c_ncand == 0 && L.c_examined == R && L.c_ok == 2 * R && L.c_take == 3 * R && L.c_tranches == 4 * R && L.c_fill == 5 * R);
                CHECK(L.c_off == 6 * R && L.c_seg == L.c_off + R + 1 && L.c_words == L.c_seg + R + 1);
                const BestsLayout Lb(B + 1, R, hk), Lr(B, R + 1, hk);
                CHECK(Lb.bytes >= L.bytes && Lr.bytes >= L.bytes && Lb.h_bytes >= L.h_bytes && Lr.h_bytes >= L.h_bytes);
                (void)last_bytes, (void)last_h;
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
        if (cmd == "bests") {
            u32 R, B, K, tranche, cap, has_floors;
            ls >> R >> B >> K >> tranche >> cap >> has_floors;
            std::vector<u32> floors(8 * (size_t)R, 0), keys(8 * (size_t)B + 8), round_of(B), best((size_t)R * cap, 0xeeeeeeeeu), nb(R, 77), nc(R, 77), ne(R, 77);
            std::vector<int32_t> verdicts(B), status(B, 77);
            for (u32 r = 0; has_floors && r < R; r++) {
                std::getline(in, line);
                load_key(line, &floors[8 * (size_t)r]);
            }
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh;
                rs_ >> round_of[i] >> verdicts[i] >> kh;
                load_key(kh, &keys[8 * (size_t)i]);
            }
            u32 steps = 77;
            rounds_best_host(R, B, round_of.data(), keys.data(), verdicts.data(), floors.data(), K, tranche, cap, best.data(), nb.data(), nc.data(), ne.data(),
                             &steps, status.data());
            printf("bests %u", steps);
            for (u32 r = 0; r < R; r++) {
                printf("|%u %u %u", nb[r], nc[r], ne[r]);
                for (u32 j = 0; j < cap; j++) {
                    if (j < nb[r])
                        printf(" %u", best[(size_t)r * cap + j]);
                    else
                        CHECK(best[(size_t)r * cap + j] == 0xeeeeeeeeu);  // entries beyond min(n_best, cap) are not written
                }
                // ... and the bound on the steps: no round runs more tranches than B rows allow
                CHECK(ne[r] <= nc[r] && steps <= best_max_tranches(B, best_tranche0(K, tranche, B)) + 1);
            }
            printf("|#|");
            for (u32 i = 0; i < B; i++) printf(" %d", status[i]);
            printf("\n");
        } else if (cmd == "screen") {
            u32 R, B;
            std::string ns_s, ro_s;
            ls >> R >> B >> ns_s >> ro_s;
            const std::vector<u32> ns = split_u32(ns_s), ro = ro_s == "-" ? std::vector<u32>() : split_u32(ro_s);
            bool done = false;
            const int32_t rc = rounds_best_screen(R, ns.data(), B, ro_s == "-" ? nullptr : ro.data(), &done);
            printf("screen %d %d\n", rc, done ? 1 : 0);
        } else if (!cmd.empty()) {
            printf("FAILED unknown command %s\n", cmd.c_str());
            failures++;
        }
    }
    if (failures) return 1;
    printf("rounds_best_check ok\n");
    return 0;
}
