// Test-only stand-alone program (AddressSanitizer + UBSan, CPU build): the one-per-bidder part of csrc/round_best.h -- the rules of
// bbp_verify_round_best_distinct (round_best_distinct_host), the identity table's hash, probe, insert and lookup as the kernels run them
// (here one row after the other), and the extra layout -- driven by a command file that tests/test_round_best_distinct_host.py writes,
// one command per line, every value in hex as the bytes travel (little-endian):
//   distinct B K tranche cap floor32   then B lines "verdict key32 id32"
//                                      -> "distinct n_best n_candidates n_examined n_duplicates | best... | status..."
//   table log2 n                       then n lines "insert key32 id32" (insert: 0 / 1), rows 0..n-1; the rows with insert = 1 enter the table
//                                      in the order given  -> "table flag claimed | the occupied slots' rows, ascending | find of every row's id (-1: none)"
// and, with no command at all, self-checks of the helpers and of the layout.  Ends with "round_best_distinct_check ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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

// a table of 2^log2 slots with exactly one empty slot, placed so that row 0's probe is the longest there is and wraps
static void one_empty_slot(u32 log2) {
    const u32 slots = 1u << log2, mask = slots - 1;
    std::vector<u32> ids(8 * (size_t)(slots + 1)), keys(8 * (size_t)(slots + 1), 0), table(slots, BEST_EMPTY);
    for (u32 i = 0; i <= slots; i++)
        for (int w = 0; w < 8; w++) ids[8 * (size_t)i + w] = 0x9e3779b9u * (i + 1) + (u32)w;  // distinct identities
    for (u32 i = 0; i <= slots; i++) keys[8 * (size_t)i] = slots - i + 1;                      // row 0 first in candidate order
    const u32 h = best_id_hash(&ids[0]) & mask, gap = (h + mask) & mask;                       // the slot just before row 0's
    u32 row = 1;
    for (u32 p = h; p != gap; p = best_probe_next(p, mask)) table[p] = row++;  // slots - 1 slots, rows 1..slots-1, each of another identity
    CHECK(row == slots);
    u32 flag = 0;
    CHECK(best_table_find(table.data(), mask, ids.data(), &ids[0], &flag) == BEST_EMPTY && flag == 0);  // walks slots - 1 slots, ends at the gap
    CHECK(best_table_insert(table.data(), mask, ids.data(), keys.data(), 8, 0, slots, &flag) == 1 && flag == 0);
    CHECK(table[gap] == 0 && best_table_find(table.data(), mask, ids.data(), &ids[0], &flag) == 0 && flag == 0);
    for (u32 i = 1; i < slots; i++) CHECK(best_table_find(table.data(), mask, ids.data(), &ids[8 * (size_t)i], &flag) == i);
    CHECK(flag == 0);
    // the table is full now: an identity it does not hold raises the flag, in lookup and in insert, and neither loops nor writes
    const std::vector<u32> before = table;
    CHECK(best_table_find(table.data(), mask, ids.data(), &ids[8 * (size_t)slots], &flag) == BEST_EMPTY && flag == BEST_FLAG_PROBE);
    flag = 0;
    CHECK(best_table_insert(table.data(), mask, ids.data(), keys.data(), 8, slots, slots, &flag) == 0 && flag == BEST_FLAG_PROBE);
    CHECK(table == before);
}

static void self_checks() {
    CHECK(BBP_ROW_DUPLICATE == -2 && BBP_ROW_DUPLICATE != BBP_ROW_SKIPPED && BBP_ROW_DUPLICATE != BBP_OK);
    CHECK(BEST_EMPTY == 0xffffffffu && BEST_EMPTY >= BBP_SELECT_MAX_BIDS);  // no row index is the empty mark
    // the table's size: the least power of two >= 2 B, at most 2^21 slots = 8 MB
    CHECK(best_table_log2(1) == 1 && best_table_log2(2) == 2 && best_table_log2(3) == 3 && best_table_log2(4) == 3 && best_table_log2(5) == 4);
    CHECK(best_table_log2(BBP_SELECT_MAX_BIDS) == BEST_TABLE_LOG2_MAX && (4ull << BEST_TABLE_LOG2_MAX) == (8ull << 20));
    for (u32 B : {1u, 63u, 64u, 65u, 1000u, 65536u, 1u << 20}) {
        const u32 s = best_table_log2(B);
        CHECK((1ull << s) >= 2ull * B && (s == 1 || (1ull << (s - 1)) < 2ull * B));
    }
    // every word of an identity moves the hash; the probe wraps; the compare reads all 32 bytes
    u32 a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8];
    for (int w = 0; w < 8; w++)
        for (u32 bit : {0u, 7u, 31u}) {
            memcpy(b, a, sizeof a);
            b[w] ^= 1u << bit;
            CHECK(best_id_hash(a) != best_id_hash(b) && !best_id_equal(a, b));
        }
    memcpy(b, a, sizeof a);
    CHECK(best_id_equal(a, b) && best_id_hash(a) == best_id_hash(b));
    CHECK(best_probe_next(0, 7) == 1 && best_probe_next(7, 7) == 0 && best_probe_next(0, 0) == 0);
    // the order the holder is a minimum of: key descending, then index ascending, at either stride
    u32 k8[16] = {}, krs[2 * RS_WORDS] = {};
    k8[7] = 1, k8[8 + 7] = 2, krs[RS_Q + 7] = 1, krs[RS_WORDS + RS_Q + 7] = 2;
    CHECK(best_before_at(k8, 8, 1, 0) && !best_before_at(k8, 8, 0, 1) && best_before_at(krs + RS_Q, RS_WORDS, 1, 0) && best_before(k8, 1, 0));
    k8[8 + 7] = 1;
    CHECK(best_before_at(k8, 8, 0, 1) && !best_before_at(k8, 8, 1, 0));
    for (u32 log2 : {1u, 2u, 3u, 6u}) one_empty_slot(log2);
    // one identity, three rows: a row that comes later in candidate order does not displace the holder, one that comes earlier does
    // (max_replace = 0 still allows the one exchange an uncontended insert needs)
    {
        u32 ids[24] = {}, keys[24] = {}, table[2] = {BEST_EMPTY, BEST_EMPTY}, flag = 0;
        keys[0] = 1, keys[8] = 2, keys[16] = 3;  // one identity (all zero), row 2 first in candidate order
        CHECK(best_table_insert(table, 1, ids, keys, 8, 0, 4, &flag) == 1 && best_table_insert(table, 1, ids, keys, 8, 1, 4, &flag) == 0 && flag == 0);
        CHECK(best_table_find(table, 1, ids, ids, &flag) == 1);
        CHECK(best_table_insert(table, 1, ids, keys, 8, 2, 0, &flag) == 0 && flag == 0 && best_table_find(table, 1, ids, ids, &flag) == 2);
    }
    // the extra layout: behind BestLayout(B, false), regions in order, none overlapping, 256-aligned; BestLayout itself is untouched
    for (u32 B : {1u, 63u, 70u, 5000u, 1u << 20})
        for (bool host : {false, true})
            for (u32 log2 : {0u, 5u, 21u}) {
                const BestLayout L(B, false);
                const BestDistinctLayout D(L, B, log2, host);
                const size_t n = B;
                CHECK(D.log2 == (log2 ? log2 : best_table_log2(B)) && D.slots == 1u << D.log2);
                CHECK(D.dctr >= L.bytes && D.ids >= D.dctr + 4 * BEST_D_WORDS && D.table >= D.ids + 32 * n && D.kid >= D.table + 4 * (size_t)D.slots);
                CHECK(D.bytes >= D.kid + (host ? 64 * n : 0));
                CHECK(D.h_dctr >= L.h_bytes && D.h_kid >= D.h_dctr + 4 * BEST_D_WORDS && D.h_bytes >= D.h_kid + (host ? 64 * n : 0));
                for (size_t o : {D.dctr, D.ids, D.table, D.kid, D.h_dctr, D.h_kid}) CHECK(o % 256 == 0);
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
        if (cmd == "distinct") {
            u32 B, K, tranche, cap;
            std::string fh;
            ls >> B >> K >> tranche >> cap >> fh;
            u32 floor[8];
            load_key(fh, floor);
            std::vector<u32> keys(8 * (size_t)B), ids(8 * (size_t)B), best(cap);  // (exactly cap entries: ASan sees a write beyond them)
            std::vector<int32_t> verdicts(B), status(B, 77);
            for (u32 i = 0; i < B; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh, ih;
                rs_ >> verdicts[i] >> kh >> ih;
                load_key(kh, &keys[8 * (size_t)i]), load_key(ih, &ids[8 * (size_t)i]);
            }
            u32 nb = 0, nc = 0, ne = 0, nd = 0;
            round_best_distinct_host(B, keys.data(), ids.data(), verdicts.data(), floor, K, tranche, cap, best.data(), &nb, &nc, &ne, &nd, status.data());
            printf("distinct %u %u %u %u |", nb, nc, ne, nd);
            for (u32 j = 0; j < nb && j < cap; j++) printf(" %u", best[j]);
            printf(" |");
            for (u32 i = 0; i < B; i++) printf(" %d", status[i]);
            printf("\n");
            CHECK((unsigned long long)ne + nd <= nc);
        } else if (cmd == "table") {
            u32 log2, n;
            ls >> log2 >> n;
            const u32 slots = 1u << log2, mask = slots - 1;
            std::vector<u32> keys(8 * (size_t)n), ids(8 * (size_t)n), table(slots, BEST_EMPTY);
            std::vector<int> enters(n);
            for (u32 i = 0; i < n; i++) {
                std::getline(in, line);
                std::istringstream rs_(line);
                std::string kh, ih;
                rs_ >> enters[i] >> kh >> ih;
                load_key(kh, &keys[8 * (size_t)i]), load_key(ih, &ids[8 * (size_t)i]);
            }
            u32 flag = 0, claimed = 0;
            for (u32 i = 0; i < n; i++)
                if (enters[i]) claimed += best_table_insert(table.data(), mask, ids.data(), keys.data(), 8, i, n, &flag);
            std::vector<u32> held;
            for (u32 p = 0; p < slots; p++)
                if (table[p] != BEST_EMPTY) held.push_back(table[p]);
            std::sort(held.begin(), held.end());
            printf("table %u %u |", flag, claimed);
            for (u32 h : held) printf(" %u", h);
            printf(" |");
            for (u32 i = 0; i < n; i++) printf(" %d", (int)best_table_find(table.data(), mask, ids.data(), &ids[8 * (size_t)i], &flag));
            printf("\n");
        } else if (!cmd.empty()) {
            printf("FAILED unknown command %s\n", cmd.c_str());
            failures++;
        }
    }
    if (failures) return 1;
    printf("round_best_distinct_check ok\n");
    return 0;
}
