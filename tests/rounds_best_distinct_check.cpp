// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): csrc/rounds_best_distinct.h -- the rules of
// bbp_verify_rounds_best_distinct (rounds_best_distinct_host), the identity table with identities that belong to a round (hash, insert
// and lookup as the kernels run them, here one row after the other), the per-step plan and the extra layout -- driven by a command file
// that tests/test_rounds_best_distinct_host.py writes, one command per line, every value in hex as the bytes travel (little-endian):
//   bestsd R B K tranche cap has_floors   then (has_floors) R lines "floor32", then B lines "round verdict key32 id32"
//                                         -> "bestsd n_steps|nb nc ne nd best...|... (R parts)|#|status..."
//   table log2 n                          then n lines "insert round key32 id32" (insert: 0 / 1), rows 0..n-1; the rows with insert = 1 enter
//                                         the table in the order given
//                                         -> "table flag claimed | the occupied slots' rows, ascending | find of every row's identity (-1: none)"
// and, with no command at all, self-checks of the helpers and of the layout.  Ends with "rounds_best_distinct_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/rounds_best_distinct.h"

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

// a table of 2^log2 slots with exactly one empty slot, placed so that row 0's probe is the longest there is and wraps; every row
// carries the SAME 32 bytes, in a round of its own: the round alone tells the identities apart
static void one_empty_slot(u32 log2) {
    const u32 slots = 1u << log2, mask = slots - 1;
    std::vector<u32> ids(8 * (size_t)(slots + 1), 0x5a5a5a5au), keys(8 * (size_t)(slots + 1), 0), round_of(slots + 1), table(slots, BEST_EMPTY);
    for (u32 i = 0; i <= slots; i++) round_of[i] = 3 * i + 1, keys[8 * (size_t)i] = slots - i + 1;  // row 0 first in candidate order
    const u32 h = bests_id_hash(round_of[0], &ids[0]) & mask, gap = (h + mask) & mask;              // the slot just before row 0's
    u32 row = 1;
    for (u32 p = h; p != gap; p = best_probe_next(p, mask)) table[p] = row++;  // slots - 1 slots, rows 1..slots-1, each of another round
    CHECK(row == slots);
    u32 flag = 0;
    CHECK(bests_table_find(table.data(), mask, ids.data(), round_of.data(), round_of[0], &ids[0], &flag) == BEST_EMPTY && flag == 0);
    CHECK(bests_table_insert(table.data(), mask, ids.data(), round_of.data(), keys.data(), 8, 0, slots, &flag) == 1 && flag == 0);
    CHECK(table[gap] == 0 && bests_table_find(table.data(), mask, ids.data(), round_of.data(), round_of[0], &ids[0], &flag) == 0 && flag == 0);
    for (u32 i = 1; i < slots; i++) CHECK(bests_table_find(table.data(), mask, ids.data(), round_of.data(), round_of[i], &ids[8 * (size_t)i], &flag) == i);
    CHECK(flag == 0);
    // the table is full now: an identity it does not hold raises the flag, in lookup and in insert, and neither loops nor writes
    const std::vector<u32> before = table;
    CHECK(bests_table_find(table.data(), mask, ids.data(), round_of.data(), round_of[slots], &ids[8 * (size_t)slots], &flag) == BEST_EMPTY && flag == BEST_FLAG_PROBE);
    flag = 0;
    CHECK(bests_table_insert(table.data(), mask, ids.data(), round_of.data(), keys.data(), 8, slots, slots, &flag) == 0 && flag == BEST_FLAG_PROBE);
    CHECK(table == before);
}

static void self_checks() {
    // the round moves the hash, as every word of the identity does; equality reads the round and all 32 bytes
    u32 a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8];
    for (u32 bit : {0u, 7u, 15u, 31u}) CHECK(bests_id_hash(5, a) != bests_id_hash(5 ^ (1u << bit), a));
    for (int w = 0; w < 8; w++)
        for (u32 bit : {0u, 7u, 31u}) {
            memcpy(b, a, sizeof a);
            b[w] ^= 1u << bit;
            CHECK(bests_id_hash(9, a) != bests_id_hash(9, b));
        }
    {
        u32 ids[16], ro[2] = {4, 4};
        memcpy(ids, a, 32), memcpy(ids + 8, a, 32);
        CHECK(bests_id_equal(ids, ro, 0, 4, ids + 8) && !bests_id_equal(ids, ro, 0, 5, ids + 8));
        ids[8 + 7] ^= 0x80000000u;
        CHECK(!bests_id_equal(ids, ro, 0, 4, ids + 8));
    }
    // one z_img resent in every round: the rounds spread it over the table -- in a table of 2 R slots the R identities start on many
    // chains, not one (the round enters the hash, not the equality test only)
    {
        const u32 R = 1024, mask = 2 * R - 1;
        std::set<u32> starts;
        for (u32 r = 0; r < R; r++) starts.insert(bests_id_hash(r, a) & mask);
        CHECK(starts.size() > R / 2);
    }
    for (u32 log2 : {1u, 2u, 3u, 6u}) one_empty_slot(log2);
    // one identity, three rows of one round: a row that comes later in candidate order does not displace the holder, one that comes earlier
    // does; the same bytes in another round claim a slot of their own
    {
        u32 ids[32] = {}, keys[32] = {}, ro[4] = {7, 7, 7, 8}, table[4] = {BEST_EMPTY, BEST_EMPTY, BEST_EMPTY, BEST_EMPTY}, flag = 0;
        keys[0] = 1, keys[8] = 2, keys[16] = 3, keys[24] = 9;  // row 2 first in candidate order among round 7's
        CHECK(bests_table_insert(table, 3, ids, ro, keys, 8, 0, 4, &flag) == 1 && bests_table_insert(table, 3, ids, ro, keys, 8, 1, 4, &flag) == 0 && flag == 0);
        CHECK(bests_table_find(table, 3, ids, ro, 7, ids, &flag) == 1 && bests_table_find(table, 3, ids, ro, 8, ids, &flag) == BEST_EMPTY);
        CHECK(bests_table_insert(table, 3, ids, ro, keys, 8, 3, 4, &flag) == 1 && bests_table_find(table, 3, ids, ro, 8, ids, &flag) == 3);
        CHECK(bests_table_insert(table, 3, ids, ro, keys, 8, 2, 0, &flag) == 0 && flag == 0 && bests_table_find(table, 3, ids, ro, 7, ids, &flag) == 2);
        CHECK(bests_table_find(table, 3, ids, ro, 8, ids, &flag) == 3 && flag == 0);
    }
    // the plan of a step: live = candidates - examined - dropped; nothing once K identities are settled or no live candidate is left
    CHECK(bests_take_distinct(1, 4, 0, 10, 0, 0, 0) == 4 && bests_take_distinct(1, 4, 1, 10, 4, 0, 0) == 6 && bests_take_distinct(1, 4, 1, 10, 4, 0, 1) == 0);
    CHECK(bests_take_distinct(2, 1, 1, 10, 2, 5, 1) == 3 && bests_take_distinct(2, 1, 1, 10, 2, 8, 1) == 0 && bests_take_distinct(2, 1, 1, 10, 2, 9, 1) == 0);
    CHECK(bests_take_distinct(0, 4, 0, 10, 0, 0, 0) == 10 && bests_take_distinct(0, 4, 1, 10, 10, 0, 3) == 0 && bests_take_distinct(3, 1, 2, 100, 9, 1, 2) == 12);
    CHECK(bests_take_distinct(1, 1, 0, 0, 0, 0, 0) == 0 && bests_take_distinct(1, 0, 0, 100, 0, 0, 0) == 16);
    for (u32 t = 0; t < 4; t++) CHECK(bests_take_distinct(3, 2, t, 50, 7, 0, 1) == bests_take(3, 2, t, 50, 7, 1));  // no drops: the plain plan
    // the extra layout: behind BestsLayout(B, R, false), regions in order, none overlapping, 256-aligned; BestsLayout itself is untouched
    for (u32 R : {1u, 2u, 64u, 257u, 1000u, BBP_BEST_MAX_ROUNDS})
        for (u32 B : {1u, 63u, 70u, 5000u, 1u << 20})
            for (bool host : {false, true})
                for (u32 log2 : {0u, 5u, 21u}) {
                    const BestsLayout L(B, R, false);
                    const BestsDistinctLayout D(L, B, R, log2, host);
                    const size_t n = B, words = 2 * (size_t)R + 1;
                    CHECK(D.log2 == (log2 ? log2 : best_table_log2(B)) && D.slots == 1u << D.log2);
                    CHECK(D.d_settled == 0 && D.d_dups == R && D.d_flag == 2 * R && D.d_words == words);
                    CHECK(D.dctr >= L.bytes && D.ids >= D.dctr + 4 * words && D.table >= D.ids + 32 * n && D.kid >= D.table + 4 * (size_t)D.slots);
                    CHECK(D.bytes >= D.kid + (host ? 64 * n : 0));
                    CHECK(D.h_dctr >= L.h_bytes && D.h_kid >= D.h_dctr + 4 * words && D.h_bytes >= D.h_kid + (host ? 64 * n : 0));
                    for (size_t o : {D.dctr, D.ids, D.table, D.kid, D.h_dctr, D.h_kid}) CHECK(o % 256 == 0);
                    CHECK(L.rowoff + 8 * n <= L.cand);  // where the staged rows start: the host forms use the _dev form's row offsets
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
        if (cmd == "bestsd") {
            u32 R, B, K, tranche, cap, has_floors;
            ls >> R >> B >> K >> tranche >> cap >> has_floors;
            std::vector<u32> floors(8 * (size_t)R, 0), keys(8 * (size_t)B + 8), ids(8 * (size_t)B + 8), round_of(B), best((size_t)R * cap, 0xeeeeeeeeu), nb(R, 77),
                nc(R, 77), ne(R, 77), nd(R, 77);
            std::vector<int32_t> verdicts(B), status(B, 77);
            for (u32 r = 0; has_floors && r < R; r++) {
                std::getline(in, line);
                load_key(line, &floors[8 * (size_t)r]);
            }
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh, ih;
                rs_ >> round_of[i] >> verdicts[i] >> kh >> ih;
                load_key(kh, &keys[8 * (size_t)i]), load_key(ih, &ids[8 * (size_t)i]);
            }
            u32 steps = 77;
            rounds_best_distinct_host(R, B, round_of.data(), keys.data(), ids.data(), verdicts.data(), floors.data(), K, tranche, cap, best.data(), nb.data(),
                                      nc.data(), ne.data(), nd.data(), &steps, status.data());
            printf("bestsd %u", steps);
            for (u32 r = 0; r < R; r++) {
                printf("|%u %u %u %u", nb[r], nc[r], ne[r], nd[r]);
                for (u32 j = 0; j < cap; j++) {
                    if (j < nb[r])
                        printf(" %u", best[(size_t)r * cap + j]);
                    else
                        CHECK(best[(size_t)r * cap + j] == 0xeeeeeeeeu);  // entries beyond min(n_best, cap) are not written
                }
                CHECK((unsigned long long)ne[r] + nd[r] <= nc[r] && steps <= best_max_tranches(B, best_tranche0(K, tranche, B)) + 1);
            }
            printf("|#|");
            for (u32 i = 0; i < B; i++) printf(" %d", status[i]);
            printf("\n");
        } else if (cmd == "table") {
            u32 log2, n;
            ls >> log2 >> n;
            const u32 slots = 1u << log2, mask = slots - 1;
            std::vector<u32> keys(8 * (size_t)n), ids(8 * (size_t)n), round_of(n), table(slots, BEST_EMPTY);
            std::vector<int> enters(n);
            for (u32 i = 0; i < n; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh, ih;
                rs_ >> enters[i] >> round_of[i] >> kh >> ih;
                load_key(kh, &keys[8 * (size_t)i]), load_key(ih, &ids[8 * (size_t)i]);
            }
            u32 flag = 0, claimed = 0;
            for (u32 i = 0; i < n; i++)
                if (enters[i]) claimed += bests_table_insert(table.data(), mask, ids.data(), round_of.data(), keys.data(), 8, i, n, &flag);
            std::vector<u32> held;
            for (u32 p = 0; p < slots; p++)
                if (table[p] != BEST_EMPTY) held.push_back(table[p]);
            std::sort(held.begin(), held.end());
            printf("table %u %u |", flag, claimed);
            for (u32 h : held) printf(" %u", h);
            printf(" |");
            for (u32 i = 0; i < n; i++)
                printf(" %d", (int)bests_table_find(table.data(), mask, ids.data(), round_of.data(), round_of[i], &ids[8 * (size_t)i], &flag));
            printf("\n");
        } else if (!cmd.empty()) {
            printf("FAILED unknown command %s\n", cmd.c_str());
            failures++;
        }
    }
    if (failures) return 1;
    printf("rounds_best_distinct_check ok\n");
    return 0;
}
