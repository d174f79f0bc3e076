// The EXPANDED blinding draw (include/bbp.h bbp_set_blinding_draw): a proof's 3 + 2 n1 blinding scalars i~, o~, s~, s_L[n1], s_R[n1] as
// independent ChaCha20 blocks under one key squeezed from the proof's TranscriptRng, instead of one Keccak-f[1600] per draw, each
// feeding the next (host + device).
//   key     = rng.fill_bytes(32), the rng built as merlin builds it: clone of the transcript, rekeyed with every v_blinding, finalised
//             with the row's 32-byte seed
//   draw j  = sc_from_wide(block(key, counter j, nonce words ("BBPX", 0, 0))), 0 <= j < 3 + 2 n1              (RFC 8439 section 2.3)
//             j = 0 i_blinding1, 1 o_blinding1, 2 s_blinding1, 3 + i s_L[i], 3 + n1 + i s_R[i]: the order of the merlin draws
// The rng goes on after the key squeeze: the five t blindings are its next draws.
// Callers: prover.hip (k_open_key, k_expand_draws); tests/blinding_expand_check.cpp (the host restatement against a Python model).
#pragma once
#include "chacha.h"
#include "keccak.h"

namespace bbp {

static constexpr u32 CC_NONCE_BLINDING = 0x58504242u;  // "BBPX" as a little-endian word

BBP_HD u32 blinding_draws(u32 n1) { return 3 + 2 * n1; }

// step 2: the key, merlin's ordinary 32-byte draw
BBP_HD ChachaKey blinding_key_squeeze(merlin_transcript& r) {
    uint8_t b[32];
    merlin_rng_fill(r, b, 32);
    ChachaKey k;
#pragma unroll
    for (int i = 0; i < 8; i++) k.w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
    return k;
}

// step 3: draw j
BBP_HD sc blinding_expand_draw(const ChachaKey& key, u32 j) {
    u32 b[16];
    chacha20_block(key, j, CC_NONCE_BLINDING, 0, 0, b);
    return sc_from_wide(b);
}

// where draw j of proof p goes, as k_reduce_draws places the merlin draws: 0 -> ai1[p (1 + 2 n1)], 1 -> ao1[p (1 + n1)], j >= 2 ->
// s1[p (1 + 2 n1) + j - 2].  which: 0 ai1, 1 ao1, 2 s1
struct BlindingSlot {
    u32 which;
    size_t index;
};
BBP_HD BlindingSlot blinding_slot(u32 p, u32 j, u32 n1) {
    if (j == 0) return {0u, (size_t)p * (1 + 2 * (size_t)n1)};
    if (j == 1) return {1u, (size_t)p * (1 + (size_t)n1)};
    return {2u, (size_t)p * (1 + 2 * (size_t)n1) + (j - 2)};
}

// The host restatement of steps 1 and 2 for one proof: V[m] the encoded commitments, vb[m] the canonical v_blindings, seed the row's last
// 32 bytes.  Returns the key; *rng_after (optional) is the rng as k_open_key stores it, ready for the t blindings.
inline ChachaKey blinding_expand_host(u32 m, const u8* V, const u8* vb, const u8 seed[32], merlin_transcript* rng_after = nullptr) {
    merlin_transcript t;
    merlin_init(t, reinterpret_cast<const uint8_t*>("BlindBidProofGadget"), 19);
    merlin_append(t, reinterpret_cast<const uint8_t*>("dom-sep"), 7, reinterpret_cast<const uint8_t*>("r1cs v1"), 7);
    for (u32 i = 0; i < m; i++) merlin_append(t, reinterpret_cast<const uint8_t*>("V"), 1, V + 32 * (size_t)i, 32);
    merlin_append_u64(t, reinterpret_cast<const uint8_t*>("m"), 1, (u64)m);
    merlin_transcript r = t;
    for (u32 i = 0; i < m; i++) merlin_rng_rekey(r, reinterpret_cast<const uint8_t*>("v_blinding"), 10, vb + 32 * (size_t)i, 32);
    merlin_rng_finalize(r, seed);
    const ChachaKey k = blinding_key_squeeze(r);
    if (rng_after) *rng_after = r;
    return k;
}

}  // namespace bbp
