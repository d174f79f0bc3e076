// The base-index lists of the prover's and the verifier's fixed-base MSMs, as host functions over a compiled circuit: which table
// base every term's scalar rides on.  circuit_get (prover.hip) uploads what they return; a wrong entry is a wrong proof, so the CPU
// test tier compiles them too (tests/host_check.cpp).  Host only, no HIP calls.
#pragma once
#include <vector>

#include "../../include/bbp.h"
#include "batch_layout.h"
#include "circuit.h"

namespace bbp {

// Extra table bases (internal, after the 4098 public ones): PAD_BASE0 + N - 1 = sum_{k = 418 + 3N}^{1023} H[k], the generators
// that the first IPA round multiplies by ONE common scalar (the zero-padded multipliers n1 = 1442 + 3N .. 2047 contribute
// b[i] h[i - 1024] = -y^1024 for every i): 582 table-row walks become one (prover.hip k_ipa_round, index_ipa).
constexpr int PAD_BASES = 202;                             // one per list length N = 1..202
constexpr unsigned PAD_BASE0 = BBP_NUM_BASES;
// Merged bases for multiplier inputs that always carry the same value (the MiMC rounds wire a to L_i, R_i, R_{i+1} and a^2 to
// L_{i+1}, L_{i+2}, R_{i+2}: index_ai): MRG1(i) = G[i] + H[i] + H[i+1], MRG2(i) = G[i] + G[i+1] + H[i+1], i = 0..2046 --
// A_I1 then needs one term where it had three.
constexpr unsigned MRG_BASE0 = PAD_BASE0 + PAD_BASES;
constexpr int MRG_BASES = 2 * (int)IPA_N;
constexpr unsigned MSM_SKIP_BASE = 0xffffffffu;            // index-list entry: this term's scalar rides on another term's merged base
constexpr unsigned TAB_BASES = BBP_NUM_BASES + PAD_BASES + MRG_BASES;  // bases with rows in ptable

// S1 (independent random scalars): B_blinding, G[0..n1), H[0..n1)
inline std::vector<u32> index_s1(const circuit::Compiled& c) {
    std::vector<u32> s1;
    s1.push_back(BBP_BASE_BBLIND);
    for (u32 i = 0; i < c.n_mul; i++) s1.push_back(BBP_BASE_G0 + i);
    for (u32 i = 0; i < c.n_mul; i++) s1.push_back(BBP_BASE_H0 + i);
    return s1;
}
// A_O1: B_blinding, G[0..n1)
inline std::vector<u32> index_ao(const circuit::Compiled& c) {
    std::vector<u32> ao;
    ao.push_back(BBP_BASE_BBLIND);
    for (u32 i = 0; i < c.n_mul; i++) ao.push_back(BBP_BASE_G0 + i);
    return ao;
}
// A_I1: the layout of S1 with equal-valued inputs merged; *n_terms: the terms that are not skipped
inline std::vector<u32> index_ai(const circuit::Compiled& c, u32* n_terms) {
    std::vector<u32> ai = index_s1(c);
    // Multiplier inputs wired to the SAME linear combination always carry the same scalar: where three of them sit as
    // {L_i, R_i, R_i+1} or {L_i, L_i+1, R_i+1} (every MiMC round has one of each: a and a^2) the first keeps the scalar on the
    // merged base G/H sum and the other two are skipped by the sort kernel -- 1440 of A_I1's 2933 terms.
    const u32 n = c.n_mul;
    auto side = [&](u32 s) {  // s < n: left input of multiplier s, else right input of multiplier s - n
        const bool right = s >= n;
        const u32 i = right ? s - n : s;
        const u32 b = right ? c.w_roff[i] : c.w_loff[i], e = right ? c.w_loff[i + 1] : c.w_roff[i];
        return std::vector<u32>(c.w_terms.begin() + b, c.w_terms.begin() + e);
    };
    auto same = [&](u32 a, u32 b, u32 d) { return side(a) == side(b) && side(a) == side(d); };
    std::vector<char> used(2 * n, 0);
    for (u32 i = 0; i + 1 < n; i++) {
        const u32 Li = i, Ri = n + i, Li1 = i + 1, Ri1 = n + i + 1;
        if (!used[Li] && !used[Ri] && !used[Ri1] && same(Li, Ri, Ri1)) {
            ai[1 + Li] = MRG_BASE0 + i;
            ai[1 + Ri] = ai[1 + Ri1] = MSM_SKIP_BASE;
            used[Li] = used[Ri] = used[Ri1] = 1;
        } else if (!used[Li] && !used[Li1] && !used[Ri1] && same(Li, Li1, Ri1)) {
            ai[1 + Li] = MRG_BASE0 + IPA_N + i;
            ai[1 + Li1] = ai[1 + Ri1] = MSM_SKIP_BASE;
            used[Li] = used[Li1] = used[Ri1] = 1;
        }
    }
    *n_terms = 0;
    for (u32 v : ai) *n_terms += v != MSM_SKIP_BASE;
    return ai;
}
// L and R of every IPA round: [IPA_ROUNDS][2 (L, R)][IPA_TERMS]
inline std::vector<u32> index_ipa(const circuit::Compiled& c) {
    std::vector<u32> ipa;
    // IPA round r (1-based), n = 1024 >> (r-1): term rank = blk*n + io of block blk = k / 2n
    for (u32 r = 1; r <= IPA_ROUNDS; r++) {
        const u32 n = IPA_HALF >> (r - 1);
        std::vector<u32> L(IPA_TERMS), R(IPA_TERMS);
        for (u32 rank = 0; rank < IPA_HALF; rank++) {
            u32 blk = rank / n, io = rank % n;
            u32 k_lo = blk * 2 * n + io, k_hi = k_lo + n;
            L[rank] = BBP_BASE_G0 + k_hi;
            L[IPA_HALF + rank] = BBP_BASE_H0 + k_lo;
            R[rank] = BBP_BASE_G0 + k_lo;
            R[IPA_HALF + rank] = BBP_BASE_H0 + k_hi;
        }
        L[IPA_N] = R[IPA_N] = BBP_BASE_B;
        // round 1: the padded multipliers' terms of L share one scalar; their first slot carries it on the range-sum base, the
        // others carry zero (k_ipa_round)
        if (r == 1 && c.n_mul < IPA_N) L[IPA_HALF + (c.n_mul - IPA_HALF)] = PAD_BASE0 + c.n_items - 1;
        ipa.insert(ipa.end(), L.begin(), L.end());
        ipa.insert(ipa.end(), R.begin(), R.end());
    }
    return ipa;
}
// verifier fixed part, the same for every N: G[0..2048), H[0..2048), B, B_blinding
inline std::vector<u32> index_ver() {
    std::vector<u32> ver;
    for (u32 i = 0; i < IPA_N; i++) ver.push_back(BBP_BASE_G0 + i);
    for (u32 i = 0; i < IPA_N; i++) ver.push_back(BBP_BASE_H0 + i);
    ver.push_back(BBP_BASE_B);
    ver.push_back(BBP_BASE_BBLIND);
    return ver;
}

}  // namespace bbp
