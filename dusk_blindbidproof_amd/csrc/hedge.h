// Hedged on-device entropy (host + device): a prove row's ChaCha20 key is derived from the call key AND the row's own inputs, so a call
// key that comes back (a VM snapshot restored twice, a forked supervisor, a broken /dev/urandom) no longer repeats a blinding over a
// different witness (include/bbp.h "Hedged on-device entropy", bbp_set_entropy_source(HEDGED)).  For prove row i of a call with list
// length N, call key K and input row row_i = scalars7 || pub_list || toggle(u64 LE) (232 + 32 N raw bytes, bbp_prove_batch's row):
//   rowkey_i = SHA3-256("BBP-hedge-v1" || K || u32le(N) || row_i)                  (FIPS 202: rate 136, suffix 0x06)
//   nonce_i  = "BBPH" || u32le(N) || u32le(i)
//   slot k < 4+N  blinding k = LE integer of block(rowkey_i, k, nonce_i) (64 bytes) mod l, 32 canonical LE bytes at offset 32 k
//   slot 4+N      TranscriptRng seed = first 32 bytes of block(rowkey_i, 4+N, nonce_i)
// i.e. chacha.h's prove row under the row's own key and the nonce word "BBPH".  The message is 35 + 4 N 64-bit words (the 48-byte
// prefix is six of them, the row is 8-byte granular), so the sponge absorbs whole words and never handles a single byte.
// Callers: capi_prove.hip (k_hedge_keys: hedge_row_key_wave, one wavefront per row; k_draw_entropy_rowkey; the checked host path
// re-derives a failed row's key with hedge_row_key); tests/test_hedge_host.py and tests/hedge_san.cpp (the host form against
// hashlib.sha3_256 in tests/hedge_ref.py); tests/test_gpu_entropy_hedged.py (the kernels against the same restatement).
#pragma once
#include <stddef.h>

#include "chacha.h"
#include "keccak.h"
#if defined(__HIPCC__)
#include "keccak_wave.h"
#endif

namespace bbp {

static constexpr u32 CC_NONCE_HEDGED = 0x48504242u;  // "BBPH" as a little-endian word
static constexpr u32 HEDGE_PREFIX_WORDS = 6;         // "BBP-hedge-v1" (12) || K (32) || u32le(N) (4) = 48 bytes
static constexpr u32 HEDGE_RATE_WORDS = 17;          // SHA3-256: 136 bytes
BBP_HD u32 hedge_row_words(u32 N) { return 29 + 4 * N; }  // prove_in_bytes(N) / 8

// word `j` (0..16) of sponge block `b` >= 1: the row's word, the 0x06 suffix right behind the message, zero beyond it; the closing
// 0x80 goes into the last word of the block that holds the suffix.  `row(r)` is 64-bit word r of the input row, little-endian.
template <class Row>
BBP_HD u64 hedge_block_word(const Row& row, u32 rw, u32 b, u32 j) {
    const u32 r = HEDGE_RATE_WORDS * b - HEDGE_PREFIX_WORDS + j;  // the row word at this position
    u64 w = r < rw ? row(r) : r == rw ? 0x06ull : 0ull;
    if (j == HEDGE_RATE_WORDS - 1 && r >= rw) w |= 0x8000000000000000ull;
    return w;
}

// block b >= 1 into nx: a block that lies wholly inside the row is 17 unconditional loads (one clause), only the last two are predicated
template <class Row>
BBP_HD void hedge_fetch_block(const Row& row, u32 rw, u32 b, u64 nx[HEDGE_RATE_WORDS]) {
    const u32 r0 = HEDGE_RATE_WORDS * b - HEDGE_PREFIX_WORDS;
    if (r0 + HEDGE_RATE_WORDS <= rw) {
#pragma unroll
        for (u32 j = 0; j < HEDGE_RATE_WORDS; j++) nx[j] = row(r0 + j);
    } else {
#pragma unroll
        for (u32 j = 0; j < HEDGE_RATE_WORDS; j++) nx[j] = hedge_block_word(row, rw, b, j);
    }
}

// rowkey = SHA3-256(prefix || row), one thread per row: the host's form (the checked path's re-prove, the CPU tier) and the first
// device shape that was measured (DESIGN.md "Randomness": ~12 us per sponge block for a lone wavefront; hedge_row_key_wave below is
// what the kernel runs).  The 25 words stay in registers (every index below is static after unrolling); block b + 1 is fetched before
// the permutation of block b runs.
template <class Row>
BBP_HD ChachaKey hedge_row_key(const ChachaKey& K, u32 N, const Row& row) {
    const u32 rw = hedge_row_words(N);
    const u32 n_blocks = (HEDGE_PREFIX_WORDS + rw) / HEDGE_RATE_WORDS + 1;  // the padding always adds at least one byte; >= 3
    u64 a[25], nx[HEDGE_RATE_WORDS];
    a[0] = 0x676465682d504242ull;                  // "BBP-hedg"
    a[1] = 0x31762d65ull | (u64)K.w[0] << 32;      // "e-v1", K[0..3]
    a[2] = K.w[1] | (u64)K.w[2] << 32;
    a[3] = K.w[3] | (u64)K.w[4] << 32;
    a[4] = K.w[5] | (u64)K.w[6] << 32;
    a[5] = K.w[7] | (u64)N << 32;
#pragma unroll
    for (u32 j = HEDGE_PREFIX_WORDS; j < HEDGE_RATE_WORDS; j++) a[j] = row(j - HEDGE_PREFIX_WORDS);  // rw >= 33: block 0 is all message
#pragma unroll
    for (u32 j = HEDGE_RATE_WORDS; j < 25; j++) a[j] = 0;
    hedge_fetch_block(row, rw, 1, nx);
    for (u32 b = 1; b <= n_blocks; b++) {
        keccak_f1600_body(a);
        if (b == n_blocks) break;
#pragma unroll
        for (u32 j = 0; j < HEDGE_RATE_WORDS; j++) a[j] ^= nx[j];
        if (b + 1 < n_blocks) hedge_fetch_block(row, rw, b + 1, nx);
    }
    ChachaKey k;
#pragma unroll
    for (int i = 0; i < 4; i++) k.w[2 * i] = (u32)a[i], k.w[2 * i + 1] = (u32)(a[i] >> 32);
    return k;
}

#if defined(__HIPCC__)
// The device form: ONE WAVEFRONT per row, the sponge spread over its lanes as in the prover's draw chain (keccak_wave.h: one 32-bit
// half of a state word per lane, bit-interleaved, ~600 instructions per permutation instead of ~7000).  The lanes of words 0..16
// each fetch their own word of the block -- 136 consecutive bytes per load, the next block's before the current permutation -- so a
// row is read as one stream whatever the row stride.  Lane L of the wavefront calls this; every lane must (uniform control flow).
// The lanes of words 0..3 (lower half of the wavefront) store the key's 8 words at out.  No LDS memory, no atomics, no scratch.
template <class Row>
__device__ __forceinline__ void hedge_row_key_wave(const ChachaKey& K, u32 N, const Row& row, u32 L, u32* out) {
    const kw_lane c = kw_setup(L);
    const kw_iota k = kw_iota_setup(L);
    const u32 rw = hedge_row_words(N);
    const u32 n_blocks = (HEDGE_PREFIX_WORDS + rw) / HEDGE_RATE_WORDS + 1;
    const bool rate = c.live && c.word < HEDGE_RATE_WORDS;
    const u32 j = c.word;
    const u64 pre = j == 0 ? 0x676465682d504242ull : j == 1 ? (0x31762d65ull | (u64)K.w[0] << 32) : j == 2 ? (K.w[1] | (u64)K.w[2] << 32)
                  : j == 3 ? (K.w[3] | (u64)K.w[4] << 32) : j == 4 ? (K.w[5] | (u64)K.w[6] << 32) : (K.w[7] | (u64)N << 32);
    u32 a = !rate ? 0u : kw_half(j < HEDGE_PREFIX_WORDS ? pre : row(j - HEDGE_PREFIX_WORDS), c.half);  // rw >= 33: block 0 is all message
    u64 nx = rate ? hedge_block_word(row, rw, 1, j) : 0ull;
    for (u32 b = 1; b <= n_blocks; b++) {
        a = kw_keccak_f(a, c, k);
        if (b == n_blocks) break;
        a ^= kw_half(nx, c.half);
        if (b + 1 < n_blocks) nx = rate ? hedge_block_word(row, rw, b + 1, j) : 0ull;
    }
    const auto q = __builtin_amdgcn_permlane32_swap(a, a, false, false);  // the odd halves, for the lanes of the even ones
    if (c.live && c.lower && j < 4) {
        const u64 w = kw_join(a, q[1]);
        out[2 * j] = (u32)w, out[2 * j + 1] = (u32)(w >> 32);
    }
}
#endif

// slot `slot` (0 .. 4+N) of prove row `row` under its own key: entropy_prove_slot with the nonce word "BBPH"
BBP_HD void hedge_prove_slot(const ChachaKey& rowkey, u32 N, u32 row, u32 slot, u32 out8[8]) {
    u32 b[16];
    chacha20_block(rowkey, slot, CC_NONCE_HEDGED, N, row, b);
    if (slot < 4 + N) {
        const sc s = sc_from_wide(b);
#pragma unroll
        for (int i = 0; i < 8; i++) out8[i] = s.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) out8[i] = b[i];
    }
}

// ---- host: rows in byte form (the checked path's re-prove, the CPU tier) ---------------------------------------------------------
struct HedgeRowBytes {
    const u8* p;  // 232 + 32 N bytes, any alignment
    BBP_HD u64 operator()(u32 r) const {
        u64 w = 0;
        for (int i = 0; i < 8; i++) w |= (u64)p[8 * (size_t)r + i] << (8 * i);
        return w;
    }
};
inline ChachaKey hedge_row_key_bytes(const ChachaKey& K, u32 N, const u8* row) { return hedge_row_key(K, N, HedgeRowBytes{row}); }

// a whole prove row, bbp_entropy_size(N) bytes, under a row key
inline void hedge_prove_row_bytes(const ChachaKey& rowkey, u32 N, u32 row, u8* out) {
    for (u32 k = 0; k <= 4 + N; k++) {
        u32 w[8];
        hedge_prove_slot(rowkey, N, row, k, w);
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 4; j++) out[32 * k + 4 * i + j] = (u8)(w[i] >> (8 * j));
    }
}

inline void chacha_key_to_bytes(const ChachaKey& k, u8* out32) {
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out32[4 * i + j] = (u8)(k.w[i] >> (8 * j));
}

}  // namespace bbp
