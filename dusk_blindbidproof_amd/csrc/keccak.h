// Keccak-f[1600], STROBE-128 and the Merlin transcript (host + gfx950 device).
//
// Replaces the role of merlin 1.3.0 (+ keccak 0.1.0), un-vendored;
// reference call site: src/blindbid/mod.rs:37 `Transcript::new(b"BlindBidProofGadget")`, everything else
// is driven from inside bulletproofs' prover / verifier.  On the device one lane owns one proof's
// transcript (200-byte sponge + 3 counters); the 25 lanes of the sponge are 64-bit register pairs
// during the permutation.
#pragma once
#include "field.h"

namespace bbp {

// 64-bit rotate left.  On the device a rotation by a constant is two v_alignbit_b32 (the compiler's own lowering of the shift /
// or form costs three instructions: 64-bit shift, 32-bit shift, or) -- 29 rotations, 58 of the 180 vector instructions of a Keccak
// round (keccak_f1600_body below), and the prover's 2935-permutation rng chain runs at exactly the single-wave issue limit.
// n is taken mod 64 and a rotation by 0 returns x: v_alignbit_b32 reads its shift mod 32, so s = 32 would select b and swap the
// halves, and the host's x >> 64 is undefined.  For the literal amounts of keccak_f1600_body both checks fold away.
BBP_HD u64 rotl64(u64 x, int n) {
    n &= 63;
    if (n == 0) return x;
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    if (n == 32) return ((u64)lo << 32) | hi;
    const u32 a = n < 32 ? lo : hi, b = n < 32 ? hi : lo;  // rotate {b:a} left by n mod 32
    const u32 s = 32u - ((u32)n & 31u);
    const u32 rl = __builtin_amdgcn_alignbit(a, b, s), rh = __builtin_amdgcn_alignbit(b, a, s);
    return ((u64)rh << 32) | rl;
#else
    return (x << n) | (x >> (64 - n));
#endif
}

// The two Boolean steps of a round on three 64-bit lanes.  gfx950 has v_bitop3_b32 (any function of three inputs, result bit =
// table[(s0 << 2) | (s1 << 1) | s2] per bit position): one instruction per 32-bit half where plain ^ ~ & compile to two (v_xor_b32
// twice, or v_bfi_b32 + v_xor_b32), and the one-lane chain's time is its instruction count.  Tables as in keccak_wave.h's BBP_KW_ROUND.
#define BBP_BITOP3_XOR3 0x96  // s0 ^ s1 ^ s2
#define BBP_BITOP3_CHI 0xd2   // s0 ^ (~s1 & s2)
BBP_HD u64 keccak_xor3(u64 a, u64 b, u64 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = __builtin_amdgcn_bitop3_b32((u32)a, (u32)b, (u32)c, BBP_BITOP3_XOR3);
    const u32 hi = __builtin_amdgcn_bitop3_b32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32), BBP_BITOP3_XOR3);
    return ((u64)hi << 32) | lo;
#else
    return a ^ b ^ c;
#endif
}
BBP_HD u64 keccak_chi(u64 a, u64 b, u64 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = __builtin_amdgcn_bitop3_b32((u32)a, (u32)b, (u32)c, BBP_BITOP3_CHI);
    const u32 hi = __builtin_amdgcn_bitop3_b32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32), BBP_BITOP3_CHI);
    return ((u64)hi << 32) | lo;
#else
    return a ^ (~b & c);
#endif
}

// forceinline body: with `s` a local array indexed statically the 25 lanes live in registers across calls
BBP_HD void keccak_f1600_body(u64* s) {
    const u64 RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
                        0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                        0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
                        0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
                        0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    u64 a00 = s[0], a01 = s[1], a02 = s[2], a03 = s[3], a04 = s[4];
    u64 a05 = s[5], a06 = s[6], a07 = s[7], a08 = s[8], a09 = s[9];
    u64 a10 = s[10], a11 = s[11], a12 = s[12], a13 = s[13], a14 = s[14];
    u64 a15 = s[15], a16 = s[16], a17 = s[17], a18 = s[18], a19 = s[19];
    u64 a20 = s[20], a21 = s[21], a22 = s[22], a23 = s[23], a24 = s[24];
    for (int r = 0; r < 24; r++) {
        // theta: column parities, then a ^= c[x - 1] ^ rot(c[x + 1], 1) in one step (d is never formed)
        const u64 c0 = keccak_xor3(keccak_xor3(a00, a05, a10), a15, a20);
        const u64 c1 = keccak_xor3(keccak_xor3(a01, a06, a11), a16, a21);
        const u64 c2 = keccak_xor3(keccak_xor3(a02, a07, a12), a17, a22);
        const u64 c3 = keccak_xor3(keccak_xor3(a03, a08, a13), a18, a23);
        const u64 c4 = keccak_xor3(keccak_xor3(a04, a09, a14), a19, a24);
        const u64 r0 = rotl64(c0, 1), r1 = rotl64(c1, 1), r2 = rotl64(c2, 1), r3 = rotl64(c3, 1), r4 = rotl64(c4, 1);
        a00 = keccak_xor3(a00, c4, r1); a05 = keccak_xor3(a05, c4, r1); a10 = keccak_xor3(a10, c4, r1); a15 = keccak_xor3(a15, c4, r1); a20 = keccak_xor3(a20, c4, r1);
        a01 = keccak_xor3(a01, c0, r2); a06 = keccak_xor3(a06, c0, r2); a11 = keccak_xor3(a11, c0, r2); a16 = keccak_xor3(a16, c0, r2); a21 = keccak_xor3(a21, c0, r2);
        a02 = keccak_xor3(a02, c1, r3); a07 = keccak_xor3(a07, c1, r3); a12 = keccak_xor3(a12, c1, r3); a17 = keccak_xor3(a17, c1, r3); a22 = keccak_xor3(a22, c1, r3);
        a03 = keccak_xor3(a03, c2, r4); a08 = keccak_xor3(a08, c2, r4); a13 = keccak_xor3(a13, c2, r4); a18 = keccak_xor3(a18, c2, r4); a23 = keccak_xor3(a23, c2, r4);
        a04 = keccak_xor3(a04, c3, r0); a09 = keccak_xor3(a09, c3, r0); a14 = keccak_xor3(a14, c3, r0); a19 = keccak_xor3(a19, c3, r0); a24 = keccak_xor3(a24, c3, r0);
        // rho + pi : B[y][2x+3y] = rot(A[x][y])
        u64 b00 = a00;
        u64 b10 = rotl64(a01, 1), b20 = rotl64(a02, 62), b05 = rotl64(a03, 28), b15 = rotl64(a04, 27);
        u64 b16 = rotl64(a05, 36), b01 = rotl64(a06, 44), b11 = rotl64(a07, 6), b21 = rotl64(a08, 55), b06 = rotl64(a09, 20);
        u64 b07 = rotl64(a10, 3), b17 = rotl64(a11, 10), b02 = rotl64(a12, 43), b12 = rotl64(a13, 25), b22 = rotl64(a14, 39);
        u64 b23 = rotl64(a15, 41), b08 = rotl64(a16, 45), b18 = rotl64(a17, 15), b03 = rotl64(a18, 21), b13 = rotl64(a19, 8);
        u64 b14 = rotl64(a20, 18), b24 = rotl64(a21, 2), b09 = rotl64(a22, 61), b19 = rotl64(a23, 56), b04 = rotl64(a24, 14);
        // chi
        a00 = keccak_chi(b00, b01, b02); a01 = keccak_chi(b01, b02, b03); a02 = keccak_chi(b02, b03, b04); a03 = keccak_chi(b03, b04, b00); a04 = keccak_chi(b04, b00, b01);
        a05 = keccak_chi(b05, b06, b07); a06 = keccak_chi(b06, b07, b08); a07 = keccak_chi(b07, b08, b09); a08 = keccak_chi(b08, b09, b05); a09 = keccak_chi(b09, b05, b06);
        a10 = keccak_chi(b10, b11, b12); a11 = keccak_chi(b11, b12, b13); a12 = keccak_chi(b12, b13, b14); a13 = keccak_chi(b13, b14, b10); a14 = keccak_chi(b14, b10, b11);
        a15 = keccak_chi(b15, b16, b17); a16 = keccak_chi(b16, b17, b18); a17 = keccak_chi(b17, b18, b19); a18 = keccak_chi(b18, b19, b15); a19 = keccak_chi(b19, b15, b16);
        a20 = keccak_chi(b20, b21, b22); a21 = keccak_chi(b21, b22, b23); a22 = keccak_chi(b22, b23, b24); a23 = keccak_chi(b23, b24, b20); a24 = keccak_chi(b24, b20, b21);
        a00 ^= RC[r];
    }
    s[0] = a00; s[1] = a01; s[2] = a02; s[3] = a03; s[4] = a04;
    s[5] = a05; s[6] = a06; s[7] = a07; s[8] = a08; s[9] = a09;
    s[10] = a10; s[11] = a11; s[12] = a12; s[13] = a13; s[14] = a14;
    s[15] = a15; s[16] = a16; s[17] = a17; s[18] = a18; s[19] = a19;
    s[20] = a20; s[21] = a21; s[22] = a22; s[23] = a23; s[24] = a24;
}

BBP_HD_NOINLINE void keccak_f1600(u64* s) { keccak_f1600_body(s); }

// ---- STROBE-128 (rate 166) -------------------------------------------------------------------------
struct merlin_transcript {
    u64 st[25];
    u32 pos, pos_begin, cur_flags;
    u32 wave;  // device, prover.hip only: all 64 lanes of the wavefront hold THIS transcript and run it in lockstep; the permutation is then
               // spread over them (keccak_wave.h keccak_f1600_wave: 2.4 us instead of 15).  Set by the kernel after loading, meaningless in memory.
};
#if defined(__HIP_DEVICE_COMPILE__) && defined(BBP_KECCAK_WAVE)
__device__ void keccak_f1600_wave(u64* s);  // keccak_wave.h
#endif

#define BBP_STROBE_R 166u
#define BBP_FLAG_I 1u
#define BBP_FLAG_A 2u
#define BBP_FLAG_C 4u
#define BBP_FLAG_M 16u
#define BBP_FLAG_K 32u

BBP_HD void strobe_xor_byte(merlin_transcript& t, u32 pos, u32 b) { t.st[pos >> 3] ^= (u64)b << (8 * (pos & 7)); }
BBP_HD void strobe_set_byte(merlin_transcript& t, u32 pos, u32 b) {
    u32 sh = 8 * (pos & 7);
    t.st[pos >> 3] = (t.st[pos >> 3] & ~((u64)0xff << sh)) | ((u64)b << sh);
}
BBP_HD u32 strobe_get_byte(const merlin_transcript& t, u32 pos) { return (u32)(t.st[pos >> 3] >> (8 * (pos & 7))) & 0xffu; }

BBP_HD void strobe_run_f(merlin_transcript& t) {
    strobe_xor_byte(t, t.pos, t.pos_begin);
    strobe_xor_byte(t, t.pos + 1, 0x04);
    strobe_xor_byte(t, BBP_STROBE_R + 1, 0x80);
#if defined(__HIP_DEVICE_COMPILE__) && defined(BBP_KECCAK_WAVE)
    if (t.wave) keccak_f1600_wave(t.st);
    else
#endif
        keccak_f1600(t.st);
    t.pos = 0;
    t.pos_begin = 0;
}

BBP_HD void strobe_absorb(merlin_transcript& t, const uint8_t* d, u32 n) {
    for (u32 i = 0; i < n; i++) {
        strobe_xor_byte(t, t.pos, d[i]);
        if (++t.pos == BBP_STROBE_R) strobe_run_f(t);
    }
}

BBP_HD void strobe_overwrite(merlin_transcript& t, const uint8_t* d, u32 n) {
    for (u32 i = 0; i < n; i++) {
        strobe_set_byte(t, t.pos, d[i]);
        if (++t.pos == BBP_STROBE_R) strobe_run_f(t);
    }
}

BBP_HD void strobe_squeeze(merlin_transcript& t, uint8_t* d, u32 n) {
    for (u32 i = 0; i < n; i++) {
        d[i] = (uint8_t)strobe_get_byte(t, t.pos);
        strobe_set_byte(t, t.pos, 0);
        if (++t.pos == BBP_STROBE_R) strobe_run_f(t);
    }
}

BBP_HD void strobe_begin_op(merlin_transcript& t, u32 flags, bool more) {
    if (more) return;  // caller guarantees flags == cur_flags
    uint8_t hdr[2] = {(uint8_t)t.pos_begin, (uint8_t)flags};
    t.pos_begin = t.pos + 1;
    t.cur_flags = flags;
    strobe_absorb(t, hdr, 2);
    if ((flags & (BBP_FLAG_C | BBP_FLAG_K)) && t.pos != 0) strobe_run_f(t);
}

BBP_HD void strobe_meta_ad(merlin_transcript& t, const uint8_t* d, u32 n, bool more) {
    strobe_begin_op(t, BBP_FLAG_M | BBP_FLAG_A, more);
    strobe_absorb(t, d, n);
}
BBP_HD void strobe_ad(merlin_transcript& t, const uint8_t* d, u32 n, bool more) {
    strobe_begin_op(t, BBP_FLAG_A, more);
    strobe_absorb(t, d, n);
}
BBP_HD void strobe_prf(merlin_transcript& t, uint8_t* d, u32 n, bool more) {
    strobe_begin_op(t, BBP_FLAG_I | BBP_FLAG_A | BBP_FLAG_C, more);
    strobe_squeeze(t, d, n);
}
BBP_HD void strobe_key(merlin_transcript& t, const uint8_t* d, u32 n, bool more) {
    strobe_begin_op(t, BBP_FLAG_A | BBP_FLAG_C, more);
    strobe_overwrite(t, d, n);
}

BBP_HD void le32(uint8_t* o, u32 x) {
    o[0] = (uint8_t)x;
    o[1] = (uint8_t)(x >> 8);
    o[2] = (uint8_t)(x >> 16);
    o[3] = (uint8_t)(x >> 24);
}

// ---- Merlin ----------------------------------------------------------------------------------------
BBP_HD void merlin_append(merlin_transcript& t, const uint8_t* label, u32 llen, const uint8_t* msg, u32 mlen) {
    uint8_t len4[4];
    le32(len4, mlen);
    strobe_meta_ad(t, label, llen, false);
    strobe_meta_ad(t, len4, 4, true);
    strobe_ad(t, msg, mlen, false);
}

BBP_HD void merlin_append_u64(merlin_transcript& t, const uint8_t* label, u32 llen, u64 x) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(x >> (8 * i));
    merlin_append(t, label, llen, b, 8);
}

BBP_HD void merlin_init(merlin_transcript& t, const uint8_t* label, u32 llen) {
    for (int i = 0; i < 25; i++) t.st[i] = 0;
    const uint8_t hdr[18] = {1, 168, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    for (u32 i = 0; i < 18; i++) strobe_xor_byte(t, i, hdr[i]);
    keccak_f1600(t.st);
    t.pos = t.pos_begin = t.cur_flags = t.wave = 0;
    const uint8_t proto[11] = {'M', 'e', 'r', 'l', 'i', 'n', ' ', 'v', '1', '.', '0'};
    strobe_meta_ad(t, proto, 11, false);
    const uint8_t ds[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
    merlin_append(t, ds, 7, label, llen);
}

BBP_HD void merlin_challenge(merlin_transcript& t, const uint8_t* label, u32 llen, uint8_t* out, u32 n) {
    uint8_t len4[4];
    le32(len4, n);
    strobe_meta_ad(t, label, llen, false);
    strobe_meta_ad(t, len4, 4, true);
    strobe_prf(t, out, n, false);
}

// TranscriptRngBuilder on a COPY of the transcript
BBP_HD void merlin_rng_rekey(merlin_transcript& t, const uint8_t* label, u32 llen, const uint8_t* w, u32 wlen) {
    uint8_t len4[4];
    le32(len4, wlen);
    strobe_meta_ad(t, label, llen, false);
    strobe_meta_ad(t, len4, 4, true);
    strobe_key(t, w, wlen, false);
}

BBP_HD void merlin_rng_finalize(merlin_transcript& t, const uint8_t* ent32) {
    const uint8_t l[3] = {'r', 'n', 'g'};
    strobe_meta_ad(t, l, 3, false);
    strobe_key(t, ent32, 32, false);
}

BBP_HD void merlin_rng_fill(merlin_transcript& t, uint8_t* out, u32 n) {
    uint8_t len4[4];
    le32(len4, n);
    strobe_meta_ad(t, len4, 4, false);
    strobe_prf(t, out, n, false);
}

// `count` consecutive TranscriptRng::fill_bytes(64) calls (one per Scalar::random) in steady state.
// After any 64-byte fill the sponge sits at pos = 64, pos_begin = 0, and the next fill is always the same byte script:
//   meta_ad(u32_le(64))  -> absorb [0x00, M|A = 0x12] at 64,65 and [0x40,0,0,0] at 66..69
//   prf begin            -> absorb [65, I|A|C = 0x07] at 70,71 ; run_f: st[72] ^= 71, st[73] ^= 0x04, st[167] ^= 0x80
//   squeeze 64           -> output bytes 0..63, zero them, pos = 64
// so each draw is three constant lane XORs, one Keccak-f[1600] and a copy of lanes 0..7 -- no byte loops, and the 25
// lanes stay in registers for the whole run.  Returns false (and does nothing) if the sponge is not in that state.
BBP_HD bool merlin_rng_fill64_bulk(merlin_transcript& t, u32 count, u32* out_words /* count * 16 */) {
    if (t.pos != 64 || t.pos_begin != 0) return false;
    u64 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = t.st[i];
    for (u32 c = 0; c < count; c++) {
        a[8] ^= 0x0741000000401200ull;
        a[9] ^= 0x0000000000000447ull;
        a[20] ^= 0x8000000000000000ull;
        keccak_f1600_body(a);
        u32* o = out_words + (size_t)c * 16;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            o[2 * i] = (u32)a[i];
            o[2 * i + 1] = (u32)(a[i] >> 32);
            a[i] = 0;
        }
    }
#pragma unroll
    for (int i = 0; i < 25; i++) t.st[i] = a[i];
    t.cur_flags = BBP_FLAG_I | BBP_FLAG_A | BBP_FLAG_C;
    return true;
}

// ---- pair form: half a state per lane ---------------------------------------------------------------
// The only operations of Keccak-f[1600] that mix the two 32-bit halves of a 64-bit lane are its 29 rotations per round (theta: 5 by 1;
// rho: 24, none by 0 or 32); theta's XORs, chi and iota are bitwise.  Two adjacent GPU lanes share a state: the even one holds the 25 low
// words, the odd one the 25 high words.  Each then runs 60 three-input operations per round instead of 120, and per rotation one partner
// fetch (a DPP move inside the quad, no LDS) plus ONE v_alignbit_b32, the same instruction in both lanes:
//   rotl by r < 32:  own' = alignbit(own, partner, 32 - r)        rotl by r > 32:  own' = alignbit(partner, own, 64 - r)
// A round is three phases between two partner reads (the column parities; the 24 words rho rotates), so the same phase functions serve
// the device, where the read is keccak_pair_partner, and the host model, which keeps a pair as two arrays of 25 words and reads the
// other array (keccak_f1600_pair_model: what the CPU tier checks the split with).
BBP_HD u32 keccak_alignbit(u32 a, u32 b, u32 s) {  // low word of {a:b} >> s, 0 < s < 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(a, b, s);
#else
    return (u32)(((((u64)a) << 32) | b) >> s);
#endif
}
BBP_HD u32 keccak_xor3_32(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, BBP_BITOP3_XOR3);
#else
    return (u32)keccak_xor3(a, b, c);
#endif
}
BBP_HD u32 keccak_chi_32(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, BBP_BITOP3_CHI);
#else
    return (u32)keccak_chi(a, b, c);
#endif
}
#define BBP_PAIR_IOTA_TABLE 0x78  // s0 ^ (s1 & s2)
BBP_HD u32 keccak_xorand_32(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, BBP_PAIR_IOTA_TABLE);
#else
    return a ^ (b & c);
#endif
}
// this half of rotl64 by the literal r (not 0, not 32): `own` and `partner` are the two halves of the word
BBP_HD u32 keccak_pair_rotl(u32 own, u32 partner, int r) { return r < 32 ? keccak_alignbit(own, partner, 32u - (u32)r) : keccak_alignbit(partner, own, 64u - (u32)r); }

// phase 1: the five column parities of this half
BBP_HD void keccak_pair_parity(const u32* a, u32* c) {
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = keccak_xor3_32(keccak_xor3_32(a[x], a[x + 5], a[x + 10]), a[x + 15], a[x + 20]);
}
// phase 2: a[x + 5y] ^= c[x - 1] ^ rotl(C[x + 1], 1); pc = the partner's parities
BBP_HD void keccak_pair_theta(u32* a, const u32* c, const u32* pc) {
#pragma unroll
    for (int x = 0; x < 5; x++) {
        const u32 cm = c[(x + 4) % 5], rp = keccak_pair_rotl(c[(x + 1) % 5], pc[(x + 1) % 5], 1);
#pragma unroll
        for (int y = 0; y < 5; y++) a[x + 5 * y] = keccak_xor3_32(a[x + 5 * y], cm, rp);
    }
}
// phase 3: rho + pi + chi; pa[1..24] = the partner's halves of the words that rho rotates (pa[0] is not read)
BBP_HD void keccak_pair_rho_pi_chi(u32* a, const u32* pa) {
    u32 b[25];
    b[0] = a[0];
#define BBP_KP_RHO(dst, src, r) b[dst] = keccak_pair_rotl(a[src], pa[src], r)
    BBP_KP_RHO(10, 1, 1); BBP_KP_RHO(20, 2, 62); BBP_KP_RHO(5, 3, 28); BBP_KP_RHO(15, 4, 27);
    BBP_KP_RHO(16, 5, 36); BBP_KP_RHO(1, 6, 44); BBP_KP_RHO(11, 7, 6); BBP_KP_RHO(21, 8, 55); BBP_KP_RHO(6, 9, 20);
    BBP_KP_RHO(7, 10, 3); BBP_KP_RHO(17, 11, 10); BBP_KP_RHO(2, 12, 43); BBP_KP_RHO(12, 13, 25); BBP_KP_RHO(22, 14, 39);
    BBP_KP_RHO(23, 15, 41); BBP_KP_RHO(8, 16, 45); BBP_KP_RHO(18, 17, 15); BBP_KP_RHO(3, 18, 21); BBP_KP_RHO(13, 19, 8);
    BBP_KP_RHO(14, 20, 18); BBP_KP_RHO(24, 21, 2); BBP_KP_RHO(9, 22, 61); BBP_KP_RHO(19, 23, 56); BBP_KP_RHO(4, 24, 14);
#undef BBP_KP_RHO
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
#pragma unroll
        for (int x = 0; x < 5; x++) a[y + x] = keccak_chi_32(b[y + x], b[y + (x + 1) % 5], b[y + (x + 2) % 5]);
    }
}
// iota.  Round constants as (low word, low ^ high): with sel = 0 in the low-word lane and ~0 in the high-word lane, the lane's constant
// is low ^ (sel & (low ^ high)) -- chosen by parity once per round in two operations, no select
BBP_HD void keccak_pair_iota(u32* a, u32 sel, int r) {
#define BBP_KP_RC(hi, lo) (((u64)((hi) ^ (lo)) << 32) | (lo))
    const u64 RC[24] = {BBP_KP_RC(0x00000000u, 0x00000001u), BBP_KP_RC(0x00000000u, 0x00008082u), BBP_KP_RC(0x80000000u, 0x0000808Au),
                        BBP_KP_RC(0x80000000u, 0x80008000u), BBP_KP_RC(0x00000000u, 0x0000808Bu), BBP_KP_RC(0x00000000u, 0x80000001u),
                        BBP_KP_RC(0x80000000u, 0x80008081u), BBP_KP_RC(0x80000000u, 0x00008009u), BBP_KP_RC(0x00000000u, 0x0000008Au),
                        BBP_KP_RC(0x00000000u, 0x00000088u), BBP_KP_RC(0x00000000u, 0x80008009u), BBP_KP_RC(0x00000000u, 0x8000000Au),
                        BBP_KP_RC(0x00000000u, 0x8000808Bu), BBP_KP_RC(0x80000000u, 0x0000008Bu), BBP_KP_RC(0x80000000u, 0x00008089u),
                        BBP_KP_RC(0x80000000u, 0x00008003u), BBP_KP_RC(0x80000000u, 0x00008002u), BBP_KP_RC(0x80000000u, 0x00000080u),
                        BBP_KP_RC(0x00000000u, 0x0000800Au), BBP_KP_RC(0x80000000u, 0x8000000Au), BBP_KP_RC(0x80000000u, 0x80008081u),
                        BBP_KP_RC(0x80000000u, 0x00008080u), BBP_KP_RC(0x00000000u, 0x80000001u), BBP_KP_RC(0x80000000u, 0x80008008u)};
#undef BBP_KP_RC
    const u64 k = RC[r];
    a[0] = keccak_xorand_32(a[0], sel, (u32)(k >> 32)) ^ (u32)k;
}

#if defined(__HIPCC__)
// the other lane of the pair: lane ^ 1, DPP quad_perm:[1,0,3,2].  Both lanes of a pair must be active.
__device__ __forceinline__ u32 keccak_pair_partner(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, true); }

// Keccak-f[1600] on this lane's 25 half-words; sel = 0 in the even (low-word) lane, ~0 in the odd (high-word) lane
__device__ __forceinline__ void keccak_f1600_pair(u32* a, u32 sel) {
    for (int r = 0; r < 24; r++) {
        u32 c[5], pc[5], pa[25];
        keccak_pair_parity(a, c);
#pragma unroll
        for (int x = 0; x < 5; x++) pc[x] = keccak_pair_partner(c[x]);
        keccak_pair_theta(a, c, pc);
        pa[0] = 0;
#pragma unroll
        for (int i = 1; i < 25; i++) pa[i] = keccak_pair_partner(a[i]);
        keccak_pair_rho_pi_chi(a, pa);
        keccak_pair_iota(a, sel, r);
    }
}
#endif

// The plain-C model of a pair: lo[] is what the even lane holds, hi[] the odd lane; every partner read is a read of the other array
// as it stood when the phase began.
inline void keccak_f1600_pair_model(u32* lo, u32* hi) {
    for (int r = 0; r < 24; r++) {
        u32 cl[5], ch[5], pl[25], ph[25];
        keccak_pair_parity(lo, cl);
        keccak_pair_parity(hi, ch);
        keccak_pair_theta(lo, cl, ch);
        keccak_pair_theta(hi, ch, cl);
        for (int i = 0; i < 25; i++) pl[i] = lo[i], ph[i] = hi[i];
        keccak_pair_rho_pi_chi(lo, ph);
        keccak_pair_rho_pi_chi(hi, pl);
        keccak_pair_iota(lo, 0u, r);
        keccak_pair_iota(hi, ~0u, r);
    }
}

// The framing of one steady-state draw (merlin_rng_fill64_bulk's three lane XORs) on the words one lane of a pair owns
BBP_HD void merlin_pair_draw_framing(u32* a, u32 sel) {
    a[8] ^= sel ? 0x07410000u : 0x00401200u;
    a[9] ^= sel ? 0u : 0x00000447u;
    a[20] ^= sel ? 0x80000000u : 0u;
}

#if defined(__HIPCC__)
// Pair form of merlin_rng_fill64_bulk.  Both lanes of the pair enter with the same full transcript and the same arguments; each keeps
// its half, runs `count` draws, writes its own eight words of every draw (word 2i low, word 2i + 1 high: the one-lane layout), and one
// exchange at the end leaves the same full state in both.  `odd` = this lane holds the high words.
__device__ __forceinline__ bool merlin_rng_fill64_bulk_pair(merlin_transcript& t, u32 count, u32* out_words /* count * 16 */, u32 odd) {
    if (t.pos != 64 || t.pos_begin != 0) return false;
    const u32 sel = odd ? ~0u : 0u;
    u32 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = odd ? (u32)(t.st[i] >> 32) : (u32)t.st[i];
    for (u32 c = 0; c < count; c++) {
        merlin_pair_draw_framing(a, sel);  // (the lane's three words are loop invariants)
        keccak_f1600_pair(a, sel);
        u32* o = out_words + (size_t)c * 16 + odd;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            o[2 * i] = a[i];
            a[i] = 0;
        }
    }
#pragma unroll
    for (int i = 0; i < 25; i++) {
        const u32 q = keccak_pair_partner(a[i]);
        t.st[i] = odd ? ((u64)a[i] << 32) | q : ((u64)q << 32) | a[i];
    }
    t.cur_flags = BBP_FLAG_I | BBP_FLAG_A | BBP_FLAG_C;
    return true;
}
#endif

// ... and its model: the pair as two arrays, entered from and left to a full state
inline bool merlin_rng_fill64_bulk_pair_model(merlin_transcript& t, u32 count, u32* out_words /* count * 16 */) {
    if (t.pos != 64 || t.pos_begin != 0) return false;
    u32 lo[25], hi[25];
    for (int i = 0; i < 25; i++) lo[i] = (u32)t.st[i], hi[i] = (u32)(t.st[i] >> 32);
    for (u32 c = 0; c < count; c++) {
        merlin_pair_draw_framing(lo, 0u);
        merlin_pair_draw_framing(hi, ~0u);
        keccak_f1600_pair_model(lo, hi);
        u32* o = out_words + (size_t)c * 16;
        for (int i = 0; i < 8; i++) {
            o[2 * i] = lo[i];      // what the even lane stores
            o[2 * i + 1] = hi[i];  // what the odd lane stores
            lo[i] = hi[i] = 0;
        }
    }
    for (int i = 0; i < 25; i++) t.st[i] = ((u64)hi[i] << 32) | lo[i];
    t.cur_flags = BBP_FLAG_I | BBP_FLAG_A | BBP_FLAG_C;
    return true;
}

}  // namespace bbp
