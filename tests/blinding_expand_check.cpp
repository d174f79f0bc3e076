// Stand-alone program (CPU build, AddressSanitizer + UBSan) of tests/test_expanded_draw_host.py: the host restatement of the EXPANDED
// blinding draw (csrc/blinding_expand.h blinding_expand_host, blinding_expand_draw, blinding_slot) for inputs given on the command line.
//   blinding_expand_check M N1 P HEX_V HEX_VB HEX_SEED J...
// M commitments (HEX_V: M x 32 bytes), their canonical blindings (HEX_VB: M x 32 bytes), the row's seed (32 bytes); N1 multipliers; P the
// proof's index in a batch (for the slots).  Prints
//   key <32 bytes>
//   draw <j> <the scalar, 32 bytes> <array: 0 ai1, 1 ao1, 2 s1> <index>      for every J
//   next <64 bytes>                                                         the rng's next 64-byte draw after the key squeeze
// Exit status 2 on malformed arguments (a J beyond 2 + 2 N1 included).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../dusk_blindbidproof_amd/csrc/blinding_expand.h"

using namespace bbp;

static bool unhex(const char* s, std::vector<u8>& out, size_t want) {
    if (strlen(s) != 2 * want) return false;
    out.resize(want);
    for (size_t i = 0; i < want; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (u8)v;
    }
    return true;
}

static void put_hex(const u8* b, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const u32 m = (u32)strtoul(argv[1], nullptr, 10), n1 = (u32)strtoul(argv[2], nullptr, 10), p = (u32)strtoul(argv[3], nullptr, 10);
    std::vector<u8> V, vb, seed;
    if (!m || !unhex(argv[4], V, 32 * (size_t)m) || !unhex(argv[5], vb, 32 * (size_t)m) || !unhex(argv[6], seed, 32)) return 2;
    merlin_transcript rng;
    const ChachaKey key = blinding_expand_host(m, V.data(), vb.data(), seed.data(), &rng);
    u8 kb[32];
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) kb[4 * i + b] = (u8)(key.w[i] >> (8 * b));
    printf("key ");
    put_hex(kb, 32);
    printf("\n");
    for (int a = 7; a < argc; a++) {
        const u32 j = (u32)strtoul(argv[a], nullptr, 10);
        if (j >= blinding_draws(n1)) return 2;
        const sc s = blinding_expand_draw(key, j);
        u8 sb[32];
        sc_tobytes(sb, s);
        const BlindingSlot slot = blinding_slot(p, j, n1);
        printf("draw %u ", j);
        put_hex(sb, 32);
        printf(" %u %zu\n", slot.which, slot.index);
    }
    u8 next[64];
    merlin_rng_fill(rng, next, 64);
    printf("next ");
    put_hex(next, 64);
    printf("\n");
    return 0;
}
