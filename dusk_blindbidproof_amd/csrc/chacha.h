// On-device entropy: the ChaCha20 block function (RFC 8439 section 2.3) and the expansion of one 32-byte key into the engine's
// entropy layouts (host + device).  Replaces the calling thread's /dev/urandom reads and host wide reductions (what thread_rng does
// for Proof::prove, src/blindbid/proof.rs:53-64, and for Verifier::verify's TranscriptRng) when bbp_set_entropy_source(DEVICE).
// Every row has a ChaCha20 stream of its own, so rows are drawn in parallel and each can be re-derived alone:
//   prove row i of list length N, m = 4 + N:  nonce = "BBPE" || u32le(N) || u32le(i)
//     slot k < m  blinding k = LE integer of block(key, k, nonce) (64 bytes) mod l, 32 canonical LE bytes at offset 32 k
//     slot m      TranscriptRng seed = first 32 bytes of block(key, m, nonce), at offset 32 m      (bbp_entropy_size(N) bytes)
//   verify row i:                             nonce = "BBPV" || u32le(0) || u32le(i); the row = first 32 bytes of block(key, 0, nonce)
// Callers: capi_prove.hip (k_draw_entropy, one lane per 32-byte slot; the checked host path re-derives a failed record's row);
// tests/test_entropy_host.py (RFC 8439 known answer, the expansion against a Python restatement).
#pragma once
#include "../../include/bbp.h"
#include "scalar.h"

namespace bbp {

struct ChachaKey {
    u32 w[8];  // the 32 key bytes as little-endian words
};

BBP_HD u32 cc_rotl(u32 x, int n) { return (x << n) | (x >> (32 - n)); }  // a constant rotation: one v_alignbit_b32

BBP_HD void cc_quarter(u32& a, u32& b, u32& c, u32& d) {
    a += b; d ^= a; d = cc_rotl(d, 16);
    c += d; b ^= c; b = cc_rotl(b, 12);
    a += b; d ^= a; d = cc_rotl(d, 8);
    c += d; b ^= c; b = cc_rotl(b, 7);
}

// RFC 8439 2.3: 16 output words (64 bytes, little-endian) of block `counter` under (key, nonce)
BBP_HD void chacha20_block(const ChachaKey& key, u32 counter, u32 n0, u32 n1, u32 n2, u32 out[16]) {
    u32 x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.w[0], key.w[1], key.w[2], key.w[3],
                 key.w[4], key.w[5], key.w[6], key.w[7], counter, n0, n1, n2};
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        cc_quarter(x[0], x[4], x[8], x[12]);
        cc_quarter(x[1], x[5], x[9], x[13]);
        cc_quarter(x[2], x[6], x[10], x[14]);
        cc_quarter(x[3], x[7], x[11], x[15]);
        cc_quarter(x[0], x[5], x[10], x[15]);
        cc_quarter(x[1], x[6], x[11], x[12]);
        cc_quarter(x[2], x[7], x[8], x[13]);
        cc_quarter(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] += x[i];
}

static constexpr u32 CC_NONCE_PROVE = 0x45504242u;   // "BBPE" as a little-endian word
static constexpr u32 CC_NONCE_VERIFY = 0x56504242u;  // "BBPV"

// slot `slot` (0 .. 4+N) of prove row `row`: 8 words of the row's bbp_entropy_size(N) bytes at offset 32 slot
BBP_HD void entropy_prove_slot(const ChachaKey& key, u32 N, u32 row, u32 slot, u32 out8[8]) {
    u32 b[16];
    chacha20_block(key, slot, CC_NONCE_PROVE, N, row, b);
    if (slot < 4 + N) {
        const sc s = sc_from_wide(b);  // Scalar::from_bytes_mod_order_wide, as the host path reduces 64 OS bytes
#pragma unroll
        for (int i = 0; i < 8; i++) out8[i] = s.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) out8[i] = b[i];
    }
}

BBP_HD void entropy_verify_row(const ChachaKey& key, u32 row, u32 out8[8]) {
    u32 b[16];
    chacha20_block(key, 0, CC_NONCE_VERIFY, 0, row, b);
#pragma unroll
    for (int i = 0; i < 8; i++) out8[i] = b[i];
}

// a whole prove row, bbp_entropy_size(N) bytes (host: the checked path's re-prove, the CPU tier)
inline void entropy_prove_row_bytes(const ChachaKey& key, u32 N, u32 row, u8* out) {
    for (u32 k = 0; k <= 4 + N; k++) {
        u32 w[8];
        entropy_prove_slot(key, N, row, k, w);
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 4; j++) out[32 * k + 4 * i + j] = (u8)(w[i] >> (8 * j));
    }
}

inline ChachaKey chacha_key_from_bytes(const u8* k32) {
    ChachaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = (u32)k32[4 * i] | (u32)k32[4 * i + 1] << 8 | (u32)k32[4 * i + 2] << 16 | (u32)k32[4 * i + 3] << 24;
    return k;
}

}  // namespace bbp
