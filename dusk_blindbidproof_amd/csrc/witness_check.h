// Does a prove-input row satisfy the blind-bid circuit?  The relations proof_gadget (src/gadgets.rs:6-34) constrains, evaluated
// natively from the row (host + device):
//   m = mimc(k, 0), x = mimc(d, m)                    :20-22
//   toggle < N and pub_list[toggle] = x (mod l)       one_of_many_gadget :88-132 (toggle bits are (i == toggle), sum 1)
//   z_img = mimc(seed, m)                             :28-30
//   mimc(seed, x) * y_inv = 1                         score_gadget :70-80
//   q = d * y_inv                                     :82-85
// y is committed but never constrained, so it is not read.  List items are Scalar::from_bits values (src/blindbid/bid.rs:27): an
// encoding of x + l passes.  A row that satisfies all of them proves to a record every verifier accepts; one that does not proves
// to a record every verifier rejects (Proof::prove does not check its witness, src/blindbid/proof.rs:36-91).
// Callers: capi_prove.hip (k_witness_check, one lane per proof; the host path's error text); tests/test_prove_check_host.py.
#pragma once
#include "../../include/bbp.h"
#include "scalar.h"

namespace bbp {

// failed-relation bits of witness_check_row, in the order the error text names them
enum : u32 {
    WC_TOGGLE = 1u,     // toggle >= N
    WC_FORMAT = 2u,     // one of d,k,y,y_inv,q,z_img,seed is not a canonical encoding (< l)
    WC_LIST = 4u,       // pub_list[toggle] != x
    WC_ZIMG = 8u,       // z_img != mimc(seed, m)
    WC_SCORE_INV = 16u, // mimc(seed, x) * y_inv != 1
    WC_SCORE_Q = 32u    // q != d * y_inv
};

BBP_HD sc wc_load(const u32* w) { return BBP_SC_LIT(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]); }

// src/gadgets.rs:37-68 on plain scalars: 90 rounds of x <- (x + key + c_i)^7, then x + key
BBP_HD sc wc_mimc(sc x, const sc& key, const sc* c) {
    for (int i = 0; i < BBP_MIMC_ROUNDS; i++) {
        const sc a = sc_add(sc_add(x, key), c[i]);
        const sc a2 = sc_mul(a, a), a3 = sc_mul(a2, a), a4 = sc_mul(a2, a2);
        x = sc_mul(a4, a3);
    }
    return sc_add(x, key);
}

// row: d,k,y,y_inv,q,z_img,seed (8 LE words each) || N list items || toggle (u64 LE) -- bbp_prove_batch's input row.
// Returns 0 when the circuit accepts the witness, else the WC_* bits of the relations that fail (a row with WC_FORMAT or
// WC_TOGGLE is not evaluated further; the list is never indexed with an unchecked toggle).
BBP_HD u32 witness_check_row(u32 N, const u32* row, const sc* mimc_c) {
    u32 fail = 0;
    for (int i = 0; i < 7; i++)
        if (!sc_is_canonical(row + 8 * i)) fail |= WC_FORMAT;
    const u64 toggle = (u64)row[56 + 8 * N] | ((u64)row[57 + 8 * N] << 32);
    if (toggle >= N) fail |= WC_TOGGLE;
    if (fail) return fail;
    const sc d = wc_load(row), k = wc_load(row + 8), y_inv = wc_load(row + 24), q = wc_load(row + 32), z_img = wc_load(row + 40),
             seed = wc_load(row + 48);
    const sc m = wc_mimc(k, sc_zero(), mimc_c);
    const sc x = wc_mimc(d, m, mimc_c);
    if (!sc_eq(sc_from_bits(row + 56 + 8 * (u32)toggle), x)) fail |= WC_LIST;
    if (!sc_eq(wc_mimc(seed, m, mimc_c), z_img)) fail |= WC_ZIMG;
    if (!sc_eq(sc_mul(wc_mimc(seed, x, mimc_c), y_inv), sc_one())) fail |= WC_SCORE_INV;
    if (!sc_eq(sc_mul(d, y_inv), q)) fail |= WC_SCORE_Q;
    return fail;
}

// the first failed relation of a witness_check_row mask, as the last-error text of a refused row
inline const char* witness_check_text(u32 fail) {
    if (fail & WC_TOGGLE) return "toggle >= N";
    if (fail & WC_FORMAT) return "non-canonical scalar input";
    if (fail & WC_LIST) return "witness not satisfied: pub_list[toggle] != x = mimc(d, mimc(k, 0))";
    if (fail & WC_ZIMG) return "witness not satisfied: z_img != mimc(seed, mimc(k, 0))";
    if (fail & WC_SCORE_INV) return "witness not satisfied: mimc(seed, x) * y_inv != 1";
    if (fail & WC_SCORE_Q) return "witness not satisfied: q != d * y_inv";
    return "witness satisfied";
}

}  // namespace bbp
