// Test-only shim: csrc/round_bids.h -- the per-row logic of bbp_prove_round (witness, list search, status, expanded row, output row)
// -- compiled for the host CPU, so that the not-gpu tier checks it against the big-int oracle.  Nothing in the shipped library calls this.
#include <string.h>

#include <vector>

#include "../dusk_blindbidproof_amd/csrc/round_bids.h"

using namespace bbp;

extern "C" {

// One round, B bids.  table: seed || pub_list (32 (1 + N) bytes); bids: B x 64; mimc90: the 90 constants.  The table is reduced as the
// device reduces it (seed: canonicity flag + reduction; items: Scalar::from_bits), then every output comes from the header:
//   rb          B x RB_WORDS words        prove_in   B x (7*32 + 32 N + 8) bytes
//   rows        B x (record + 64) bytes, from `records` (B x record bytes; may be NULL: rows is then not written)
void rc_round(uint32_t N, const uint8_t* table, uint32_t B, const uint8_t* bids, const uint8_t* mimc90, uint32_t* rb, uint8_t* prove_in,
              const uint8_t* records, uint8_t* rows) {
    std::vector<sc> c(BBP_MIMC_ROUNDS), rblk(1 + (size_t)N);
    memcpy(c.data(), mimc90, 32 * BBP_MIMC_ROUNDS);
    u32 w[8];
    memcpy(w, table, 32);
    const int32_t flag = sc_is_canonical(w) ? BBP_OK : BBP_ERR_FORMAT;
    rblk[0] = sc_reduce256(w);
    for (uint32_t i = 0; i < N; i++) {
        memcpy(w, table + 32 * (1 + (size_t)i), 32);
        rblk[1 + i] = sc_from_bits(w);
    }
    const uint32_t pw = round_in_words(N), rec = BBP_R1CS_PROOF_BYTES + 32 * (4 + N);
    for (uint32_t p = 0; p < B; p++) {
        u32* r = rb + (size_t)RB_WORDS * p;
        const uint8_t* bid = bids + BBP_ROUND_BID_BYTES * (size_t)p;
        round_bid_eval(N, bid, rblk.data(), flag, c.data(), r);
        for (uint32_t k = 0; k < pw; k++) {
            const u32 v = round_expand_word(N, k, bid, table, r);
            memcpy(prove_in + 4 * ((size_t)pw * p + k), &v, 4);
        }
        if (records)
            for (uint32_t o = 0; o < rec + 64; o++) rows[(size_t)(rec + 64) * p + o] = round_row_byte(N, o, records + (size_t)rec * p, r);
    }
}

uint32_t rc_rb_words() { return RB_WORDS; }
uint32_t rc_scratch_end(uint32_t B, uint32_t N) { return (uint32_t)round_scratch(B, N).end; }
}
