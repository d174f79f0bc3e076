// Stand-alone program (CPU build, AddressSanitizer + UBSan): the IPA tail's walk with the B-term share (csrc/scalarmul.h
// ge_scalarmul_pieces_shared, tail_share_of) as one side of k_tail_lr's wavefront runs it.  For 32 tables over multiples of a fixed
// point and the table of B: the sum of the 32 lanes' results -- each lane with its own term scalar and its share of sB, summed in
// tail_side_sum's order -- must encode to the same bytes as  sum_j ge_scalarmul_pieces(s_j, T_j) + ge_scalarmul_pieces(sB, btab).
// sB: 0, 1, l - 1, 2^252 + 1, every digit 8 (the largest digit everywhere), 0x0888..89 (a carry through all 64 digits), every nibble
// 7, random; term scalars: random, all zero, all l - 1.  The shares must also tile sB's digits: every (piece, digit) in exactly one
// lane, and sum d 16^r 2^(w k) = sB.  The tables live in heap buffers of exactly their size, so a read past one is caught.
// Exit status 0 and "tail_share_check ok" when everything agrees.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../dusk_blindbidproof_amd/csrc/scalarmul.h"

using namespace bbp;

static u32 lcg = 20240521u;
static u32 rnd32() {
    u32 r = 0;
    for (int i = 0; i < 4; i++) r = (r << 8) | ((lcg = lcg * 1664525u + 1013904223u) >> 24);
    return r;
}
static sc rnd_sc() {
    u32 w[16];
    for (u32& x : w) x = rnd32();
    return sc_from_wide(w);
}
static sc sc_nibbles(u32 nib, u32 low) {  // 0x0nnn..nl
    sc s;
    for (int w = 0; w < 8; w++) s.v[w] = 0x11111111u * nib;
    s.v[7] &= 0x0fffffffu;
    s.v[0] = (s.v[0] & ~15u) | low;
    return s;
}

static int fail(const char* what, int a, int b) {
    fprintf(stderr, "tail_share_check: %s (term set %d, sB case %d)\n", what, a, b);
    return 1;
}

int main() {
    // tables of P_j = (3 j + 2) B, j < TAIL_SIDE, and of B: each in a buffer of exactly TAIL_TAB points
    const ge Bp = ge_basepoint();
    std::vector<ge*> tab(TAIL_SIDE);
    ge P = ge_dbl(Bp);
    for (int j = 0; j < TAIL_SIDE; j++) {
        tab[j] = (ge*)malloc(sizeof(ge) * TAIL_TAB);
        tail_table_build(P, tab[j]);
        P = ge_add(ge_add(P, Bp), ge_dbl(Bp));
    }
    ge* btab = (ge*)malloc(sizeof(ge) * TAIL_TAB);
    tail_table_build(Bp, btab);

    sc lm1 = sc_l();
    lm1.v[0] -= 1;
    std::vector<sc> sBs = {sc_zero(), sc_one(), lm1, BBP_SC_LIT(1, 0, 0, 0, 0, 0, 0, 0x10000000u), sc_nibbles(8, 8), sc_nibbles(8, 9), sc_nibbles(7, 7)};
    for (int i = 0; i < 5; i++) sBs.push_back(rnd_sc());
    for (const sc& s : sBs)
        if (!sc_is_canonical(s.v)) return fail("a case scalar is not canonical", -1, -1);

    for (size_t bi = 0; bi < sBs.size(); bi++) {  // the shares tile the digits and recompose sB
        int seen[TAIL_PIECES][TAIL_DIGITS] = {};
        const sc two = sc_from_u32(2), sixteen = sc_from_u32(16);
        sc total = sc_zero();
        for (u32 j = 0; j < (u32)TAIL_SIDE; j++) {
            const tail_share sh = tail_share_of(sBs[bi], j);
            if (sh.k < 0 || sh.k >= TAIL_PIECES || sh.r0 < 0 || sh.r0 + TAIL_SHARE_DIGITS > TAIL_DIGITS) return fail("a share lies outside the table", -1, (int)bi);
            for (int i = 0; i < TAIL_SHARE_DIGITS; i++) {
                seen[sh.k][sh.r0 + i]++;
                const int d = sh.d[i];
                if (d < -7 || d > 8) return fail("a digit outside [-7, 8]", -1, (int)bi);
                sc wgt = sc_from_u32((u32)(d < 0 ? -d : d));
                for (int t = 0; t < sh.r0 + i; t++) wgt = sc_mul(wgt, sixteen);
                for (int t = 0; t < TAIL_PIECE_BITS * sh.k; t++) wgt = sc_mul(wgt, two);
                total = d < 0 ? sc_sub(total, wgt) : sc_add(total, wgt);
            }
        }
        for (int k = 0; k < TAIL_PIECES; k++)
            for (int r = 0; r < TAIL_DIGITS; r++)
                if (seen[k][r] != 1) return fail("the shares do not tile the digits", -1, (int)bi);
        if (memcmp(total.v, sBs[bi].v, 32)) return fail("the shares do not recompose sB", -1, (int)bi);
    }

    for (int ts = 0; ts < 4; ts++) {
        sc s[TAIL_SIDE];
        for (int j = 0; j < TAIL_SIDE; j++) s[j] = ts == 1 ? sc_zero() : ts == 2 ? lm1 : rnd_sc();
        ge terms = ge_identity();
        for (int j = 0; j < TAIL_SIDE; j++) terms = ge_add(terms, ge_scalarmul_pieces(s[j], tab[j]));
        for (size_t bi = 0; bi < sBs.size(); bi++) {
            u32 want[8], got[8];
            ge_encode_words(want, ge_add(terms, ge_scalarmul_pieces(sBs[bi], btab)));
            ge lane[TAIL_SIDE];
            for (u32 j = 0; j < (u32)TAIL_SIDE; j++) lane[j] = ge_scalarmul_pieces_shared(s[j], tab[j], tail_share_of(sBs[bi], j), btab);
            for (int d = TAIL_SIDE / 2; d >= 1; d >>= 1)  // tail_side_sum: lane q adds lane q + d
                for (int q = 0; q < d; q++) lane[q] = ge_add(lane[q], lane[q + d]);
            ge_encode_words(got, lane[0]);
            if (memcmp(want, got, 32)) return fail("the side's sum differs from the terms plus sB B", ts, (int)bi);
        }
    }
    for (ge* t : tab) free(t);
    free(btab);
    puts("tail_share_check ok");
    return 0;
}
