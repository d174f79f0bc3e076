// Mixed-N verification (bbp_verify_batch_mixed*): one call verifies rows of any mix of bid-list lengths.  Textually included by
// verifier.inc, ahead of its host code.
//
// Only the front end depends on N: parse, transcript replay, z powers, flatten, generator scalars and the variable-base terms.
// The kernels here are those of the uniform path (the row helpers below are their bodies) with the row's geometry read from a
// per-row descriptor instead of launch arguments; the uniform kernels themselves are left as they are.  The generator MSM
// (4098 terms over G, H, B, B_blinding, the same list for every N), k_group_sum, k_vfinal, k_var_sum and the aggregated
// fallback do not depend on N and are shared.  Per-row scratch strides are those of the largest N in the call.
#include <algorithm>

namespace bbp {

struct VCirc {  // what the front end needs of circuit N (ctx->vctab[N], filled when circuit N is first used by a mixed call)
    u32 n_mul, n_cons, n_cst, n_cterms;
    const u32 *f_off, *f_ent, *c_q, *c_cst;
};
// record || score || z_img || seed || list
__host__ __device__ __forceinline__ u64 vrow_bytes(u32 n, u32 ver) { return (ver ? 1217u : 1121u) + 32u * (4u + n) + 96u + 32u * n; }

// row offsets: one workgroup, a contiguous run of rows per lane, a scan over the lanes' sums.  vers (one byte per row) may be
// null: every row is then a compact record
__global__ __launch_bounds__(VROWS_BLK) void k_vrows(u32 B, const u32* __restrict__ ns, const u8* __restrict__ vers, VRow* __restrict__ rows) {
    __shared__ u64 part[VROWS_BLK];
    const u32 tid = threadIdx.x, per = (B + VROWS_BLK - 1) / VROWS_BLK;
    const u32 lo = min(B, tid * per), hi = min(B, lo + per);
    u64 sum = 0;
    for (u32 i = lo; i < hi; i++) sum += vrow_bytes(ns[i], vers ? vers[i] : 0u);
    part[tid] = sum;
    __syncthreads();
    for (u32 d = 1; d < VROWS_BLK; d <<= 1) {
        const u64 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u64 off = part[tid] - sum;
    for (u32 i = lo; i < hi; i++) {
        const u32 n = ns[i], ver = vers ? (vers[i] ? 1u : 0u) : 0u;
        rows[i] = VRow{off, n, (uint16_t)(4 + n), (uint16_t)ver};
        off += vrow_bytes(n, ver);
    }
}

__device__ __forceinline__ void vparse_row(u32 p, u32 n_items, u32 rec_ver, const u8* __restrict__ r, u32* __restrict__ o, sc* __restrict__ vchal,
                                           sc* __restrict__ cst, int32_t* __restrict__ status) {
    const u32 m = 4 + n_items;
    int32_t st = BBP_OK;
    if (r[0] != (u8)rec_ver) st = BBP_ERR_FORMAT;  // version byte must match the layout implied by the length
    auto ldw = [&](const u8* b, u32* w) {
        for (int i = 0; i < 8; i++) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
    };
    const u8* q = r + 1;
    for (u32 i = 0; i < 3; i++, q += 32) ldw(q, o + 8 * i);
    if (rec_ver) {
        for (u32 i = 3; i < 6; i++, q += 32) ldw(q, o + 8 * i);
    } else {
        for (u32 i = 24; i < 48; i++) o[i] = 0;  // A_I2 = A_O2 = S2 = identity
    }
    for (u32 i = 0; i < 5; i++, q += 32) ldw(q, o + 8 * (6 + m + i));
    sc* vc = vchal + (size_t)p * VC_COUNT;
    u32 w[8];
    for (u32 i = 0; i < 3; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&vc[VC_TX + i], BBP_SC_LIT(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
    }
    for (u32 j = 0; j < 11; j++, q += 64) {
        ldw(q, o + 8 * (6 + m + 5 + j));
        ldw(q + 32, o + 8 * (6 + m + 5 + 11 + j));
    }
    for (u32 i = 0; i < 2; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&vc[VC_A + i], BBP_SC_LIT(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
    }
    for (u32 i = 0; i < m; i++, q += 32) ldw(q, o + 8 * (6 + i));
    // public inputs: score, z_img, seed are serde-deserialised Scalars in the reference (verify.rs:100-104): canonical encodings
    // only, anything else is an error before Verify::verify runs -> FormatError here; pub_list via from_bits (verify.rs:115)
    st_sc(&cst[circuit::CST_ONE], sc_one());
    st_sc(&cst[circuit::CST_ZERO], sc_zero());
    const u32 pub_slot[3] = {circuit::CST_Q, circuit::CST_ZIMG, circuit::CST_SEED};
    for (u32 i = 0; i < 3; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&cst[pub_slot[i]], sc_reduce256(w));
    }
    for (u32 i = 0; i < n_items; i++, q += 32) {
        ldw(q, w);
        st_sc(&cst[circuit::CST_ITEM0 + i], sc_from_bits(w));
    }
    status[p] = st;
}

__device__ __forceinline__ void vtranscript_row(u32 p, u32 m, const merlin_transcript& prefix, const u32* __restrict__ pt, const u8* __restrict__ entropy,
                                                sc* __restrict__ vchal, sc* __restrict__ misc, int32_t* __restrict__ status, u32 wave) {
    sc* vc = vchal + (size_t)p * VC_COUNT;
    sc* ms = misc + (size_t)p * MS_COUNT;
    merlin_transcript t = prefix;
    t.wave = wave;
    bool ok = true;
    for (u32 i = 0; i < m; i++) v_append_words(t, VLBL("V"), pt + 8 * (6 + i));  // Verifier::commit: plain append
    merlin_append_u64(t, VLBL("m"), (u64)m);
    ok &= v_validate_append(t, VLBL("A_I1"), pt);
    ok &= v_validate_append(t, VLBL("A_O1"), pt + 8);
    ok &= v_validate_append(t, VLBL("S1"), pt + 16);
    merlin_append(t, VLBL("dom-sep"), VLBL("r1cs-1phase"));
    v_append_words(t, VLBL("A_I2"), pt + 24);  // no identity check on the phase-2 points
    v_append_words(t, VLBL("A_O2"), pt + 32);
    v_append_words(t, VLBL("S2"), pt + 40);
    sc y = v_challenge_sc(t, VLBL("y"));
    sc z = v_challenge_sc(t, VLBL("z"));
    const u32* T = pt + 8 * (6 + m);
    ok &= v_validate_append(t, VLBL("T_1"), T);
    ok &= v_validate_append(t, VLBL("T_3"), T + 8);
    ok &= v_validate_append(t, VLBL("T_4"), T + 16);
    ok &= v_validate_append(t, VLBL("T_5"), T + 24);
    ok &= v_validate_append(t, VLBL("T_6"), T + 32);
    sc u = v_challenge_sc(t, VLBL("u"));
    sc x = v_challenge_sc(t, VLBL("x"));
    sc tx = ld_sc(&vc[VC_TX]), txb = ld_sc(&vc[VC_TXB]), ebl = ld_sc(&vc[VC_EBL]);
    v_append_words(t, VLBL("t_x"), tx.v);
    v_append_words(t, VLBL("t_x_blinding"), txb.v);
    v_append_words(t, VLBL("e_blinding"), ebl.v);
    sc w = v_challenge_sc(t, VLBL("w"));
    merlin_append(t, VLBL("dom-sep"), VLBL("ipp v1"));
    merlin_append_u64(t, VLBL("n"), IPA_N);
    const u32 *Lp = pt + 8 * (6 + m + 5), *Rp = Lp + 8 * 11;
    // The eleven challenges and the prefix products of the batch inversion below live in the proof's own OUTPUT rows (vc[VC_U + j],
    // vc[VC_UI + j]: this lane's, L2-resident) instead of two local arrays: indexed by a loop variable those were 736 bytes of
    // scratch per lane (round 3: 1200 B in all for this kernel).
    sc run = y;  // prefix product y u_1 .. u_j
    for (int j = 0; j < 11; j++) {
        ok &= v_validate_append(t, VLBL("L"), Lp + 8 * j);
        ok &= v_validate_append(t, VLBL("R"), Rp + 8 * j);
        const sc ujj = v_challenge_sc(t, VLBL("u"));
        st_sc(&vc[VC_U + j], ujj);
        st_sc(&vc[VC_UI + j], run);  // pre[j] = y u_1 .. u_j (before this round's challenge): read back by the unwinding loop
        run = sc_mul(run, ujj);
    }
    // TranscriptRng with no witness data: external entropy only, then one scalar r (A.7)
    merlin_transcript rg = t;
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = entropy[32 * (size_t)p + i];
    merlin_rng_finalize(rg, seed);
    uint8_t rb[64];
    merlin_rng_fill(rg, rb, 64);
    u32 rw[16];
    for (int i = 0; i < 16; i++) rw[i] = (u32)rb[4 * i] | ((u32)rb[4 * i + 1] << 8) | ((u32)rb[4 * i + 2] << 16) | ((u32)rb[4 * i + 3] << 24);
    sc r = sc_from_wide(rw);
    // a second draw from the same rng: the weight of this proof in an aggregated check (verify_batch_agg_dev); unused otherwise
    merlin_rng_fill(rg, rb, 64);
    for (int i = 0; i < 16; i++) rw[i] = (u32)rb[4 * i] | ((u32)rb[4 * i + 1] << 8) | ((u32)rb[4 * i + 2] << 16) | ((u32)rb[4 * i + 3] << 24);
    st_sc(&ms[MS_RHO], sc_from_wide(rw));
    // batch inversion of y, u_1..u_11 (Scalar::batch_invert): prefix products (above), one inversion, unwind
    sc inv = sc_invert(run);  // a zero challenge has probability ~2^-252; inversion of 0 yields 0 like dalek's invert
    sc allinv = sc_one();
    for (int j = 10; j >= 0; j--) {
        const sc prej = ld_sc(&vc[VC_UI + j]), ujj = ld_sc(&vc[VC_U + j]);
        sc uji = sc_mul(inv, prej);
        inv = sc_mul(inv, ujj);
        st_sc(&vc[VC_UI + j], uji);
        allinv = sc_mul(allinv, uji);
    }
    st_sc(&ms[MS_Y], y);
    st_sc(&ms[MS_Z], z);
    st_sc(&ms[MS_U], u);
    st_sc(&ms[MS_X], x);
    st_sc(&ms[MS_W], w);
    st_sc(&ms[MS_YINV], inv);
    st_sc(&ms[MS_R], r);
    st_sc(&ms[MS_ALLINV], allinv);
    if (!ok && status[p] == BBP_OK) status[p] = BBP_ERR_VERIFY;
}

__device__ __forceinline__ void vscalars_block(u32 p, u32 n1, u32 n_cterms, const u32* __restrict__ c_q, const u32* __restrict__ c_cst,
                                               const sc* __restrict__ cst, const sc* __restrict__ zp, const sc* __restrict__ yipow,
                                               const sc* __restrict__ wl, const sc* __restrict__ wr, const sc* __restrict__ wo,
                                               const sc* __restrict__ vchal, sc* __restrict__ misc, sc* __restrict__ s_all, sc* __restrict__ vs_all,
                                               u32 agg) {
    __shared__ u32 lds[2 * 8 * VS_BLK];
    const u32 tid = threadIdx.x;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    sc* ms = misc + (size_t)p * MS_COUNT;
    const sc* YI = yipow + (size_t)p * IPA_N;
    const sc *WL = wl + (size_t)p * IPA_N, *WR = wr + (size_t)p * IPA_N, *WO = wo + (size_t)p * IPA_N;
    sc* s = s_all + (size_t)p * IPA_N;
    sc* vs = vs_all + (size_t)p * 4098;
    const sc x = ld_sc(&ms[MS_X]), u = ld_sc(&ms[MS_U]), allinv = ld_sc(&ms[MS_ALLINV]);
    const sc a = ld_sc(&vc[VC_A]), b = ld_sc(&vc[VC_B]);
    // s[i] = allinv * prod_{bit b of i set} u_{10-b}^2   (verification_scalars, A.7), built by doubling: s[i + 2^L] = s[i] * u_{10-L}^2
    // for i < 2^L, one Montgomery multiplication per entry (the squares are kept as u^2 R)
    __shared__ u32 usq[11 * 8];
    if (tid < 11) {
        const sc uj = ld_sc(&vc[VC_U + (10 - tid)]);
        const sc q = sc_to_mont(sc_mul(uj, uj));
#pragma unroll
        for (int w = 0; w < 8; w++) usq[tid * 8 + w] = q.v[w];
    }
    if (tid == 0) st_sc(&s[0], allinv);
    __threadfence_block();
    __syncthreads();
    for (u32 L = 0; L < 11; L++) {
        sc q;
#pragma unroll
        for (int w = 0; w < 8; w++) q.v[w] = usq[L * 8 + w];
        const u32 half = 1u << L;
        for (u32 i = tid; i < half; i += VS_BLK) st_sc(&s[half + i], sc_montmul(ld_sc(&s[i]), q));
        __threadfence_block();
        __syncthreads();
    }
    sc acc[2] = {sc_zero(), sc_zero()};  // acc[0] = delta, acc[1] = -wc
    const sc xr = sc_to_mont(x), ar = sc_to_mont(a), br = sc_to_mont(b), ur = sc_to_mont(u);  // v * (c R) * R^-1 = v c: one multiplication
    const sc rho_r = sc_to_mont(ld_sc(&ms[MS_RHO]));  // aggregated mode: every generator scalar of this proof times its weight
    for (u32 i = tid; i < IPA_N; i += VS_BLK) {
        const bool live = i < n1;
        const sc yir = ld_sc(&YI[i]);  // y^-i R (k_powers, Montgomery output): a product with it is ONE multiplication
        sc ynw = live ? sc_montmul(ld_sc(&WR[i]), yir) : sc_zero();
        sc wli = live ? ld_sc(&WL[i]) : sc_zero(), woi = live ? ld_sc(&WO[i]) : sc_zero();
        if (live) acc[0] = sc_add(acc[0], sc_montmul(ynw, wli));  // delta R^-1, put right after the block sum
        sc gs = sc_sub(sc_montmul(ynw, xr), sc_montmul(ld_sc(&s[i]), ar));
        sc hs = sc_sub(sc_montmul(sc_sub(sc_add(sc_montmul(wli, xr), woi), sc_montmul(ld_sc(&s[2047 - i]), br)), yir), sc_one());
        gs = live ? gs : sc_montmul(gs, ur);
        hs = live ? hs : sc_montmul(hs, ur);
        st_sc(&vs[i], agg ? sc_montmul(gs, rho_r) : gs);
        st_sc(&vs[IPA_N + i], agg ? sc_montmul(hs, rho_r) : hs);
    }
    for (u32 e = tid; e < n_cterms; e += VS_BLK) {
        u32 w = c_q[e];
        sc term = sc_mul(ld_sc(&cst[c_cst[e]]), ld_sc(&zp[(w & 0x7fffffffu) + 1]));
        acc[1] = (w >> 31) ? sc_sub(acc[1], term) : sc_add(acc[1], term);
    }
    block_sum_sc<2, VS_BLK>(acc, lds);
    if (tid == 0) {
        sc delta = sc_to_mont(acc[0]), wc = sc_neg(acc[1]);
        sc r = ld_sc(&ms[MS_R]), w = ld_sc(&ms[MS_W]);
        sc tx = ld_sc(&vc[VC_TX]), txb = ld_sc(&vc[VC_TXB]), ebl = ld_sc(&vc[VC_EBL]);
        sc xx = sc_mul(x, x);
        // B: w (t_x - a b) + r (x^2 (wc + delta) - t_x) ;  B~: -e_blinding - r t_x_blinding
        sc sB = sc_add(sc_mul(w, sc_sub(tx, sc_mul(a, b))), sc_mul(r, sc_sub(sc_mul(xx, sc_add(wc, delta)), tx)));
        sc sBb = sc_sub(sc_neg(ebl), sc_mul(r, txb));
        st_sc(&vs[4096], agg ? sc_montmul(sB, rho_r) : sB);
        st_sc(&vs[4097], agg ? sc_montmul(sBb, rho_r) : sBb);
        st_sc(&ms[MS_WC], wc);
        st_sc(&ms[MS_DELTA], delta);
    }
}

__device__ __forceinline__ ge varbase_lane(u32 p, u32 q, u32 Q, u32 m, size_t row, const u32* __restrict__ vpts, const sc* __restrict__ vchal,
                                           const sc* __restrict__ misc, const sc* __restrict__ wvrow, ge* __restrict__ tab_all,
                                           u32* __restrict__ sp_all, int32_t* __restrict__ status, u32 agg, u32 one_phase) {
    const u32 np = vnpts(m);
    // one-phase records (rec_ver 0) carry no A_I2 / A_O2 / S2: those three slots (k = 3..5) are the identity and are skipped
    const u32 npa = one_phase ? np - 3 : np;
    const sc* ms = misc + (size_t)p * MS_COUNT;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    const sc x = ld_sc(&ms[MS_X]);
    for (u32 a = q; a < npa; a += Q) {
        const u32 k = (one_phase && a >= 3) ? a + 3 : a;
        const size_t pt = row + k;
        u32* sp = sp_all + pt * 8;
        ge P;
        u32 w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = vpts[pt * 8 + i];
        if (!ge_decode_words(P, w)) {
            atomicMax(&status[p], (int32_t)BBP_ERR_VERIFY);  // optional_multiscalar_mul -> None -> VerificationError
#pragma unroll
            for (int i = 0; i < 8; i++) sp[i] = 0x88888888u;  // all digits zero: the point drops out
            continue;
        }
        sc s;
        if (k < 6) {
            sc xx = sc_mul(x, x);
            s = (k % 3 == 0) ? x : (k % 3 == 1) ? xx : sc_mul(xx, x);
            if (k >= 3) s = sc_mul(s, ld_sc(&ms[MS_U]));
        } else if (k < 6 + m) {
            sc rxx = sc_mul(ld_sc(&ms[MS_R]), sc_mul(x, x));
            s = sc_mul(ld_sc(&wvrow[k - 6]), rxx);
        } else if (k < 6 + m + 5) {
            // r x, r x^3, r x^4, r x^5, r x^6
            const u32 e[5] = {1, 3, 4, 5, 6};
            sc xp = x;
            for (u32 i = 1; i < e[k - 6 - m]; i++) xp = sc_mul(xp, x);
            s = sc_mul(ld_sc(&ms[MS_R]), xp);
        } else if (k < 6 + m + 5 + 11) {
            sc uj = ld_sc(&vc[VC_U + (k - 6 - m - 5)]);
            s = sc_mul(uj, uj);
        } else {
            sc ui = ld_sc(&vc[VC_UI + (k - 6 - m - 5 - 11)]);
            s = sc_mul(ui, ui);
        }
        if (agg) s = sc_mul(s, ld_sc(&ms[MS_RHO]));
        u64 cy = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            cy += (u64)s.v[i] + 0x88888888u;
            sp[i] = (u32)cy;
            cy >>= 32;
        }
        ge* tab = tab_all + pt * 8;  // 1P .. 8P
        tab[0] = P;
        ge cur = P;
        for (int i = 1; i < 8; i++) {
            cur = ge_add(cur, P);
            tab[i] = cur;
        }
    }
    ge acc = ge_identity();
    for (int j = 63; j >= 0; j--) {
        if (j != 63) {
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
        }
        for (u32 a = q; a < npa; a += Q) {
            const u32 k = (one_phase && a >= 3) ? a + 3 : a;
            const size_t pt = row + k;
            const int d = (int)((sp_all[pt * 8 + (j >> 3)] >> (4 * (j & 7))) & 15u) - 8;
            if (d != 0) {
                ge e = tab_all[pt * 8 + (d > 0 ? d : -d) - 1];
                if (d < 0) e = ge_neg(e);
                acc = ge_add(acc, e);
            }
        }
    }
    return acc;
}

__device__ __forceinline__ void varprep_point(u32 p, u32 a, u32 m, size_t row, const u32* __restrict__ vpts, const sc* __restrict__ vchal,
                                              const sc* __restrict__ misc, const sc* __restrict__ wvrow, ge* __restrict__ tab_all,
                                              u32* __restrict__ sp_all, int32_t* __restrict__ status, u32 agg, u32 one_phase) {
    const sc* ms = misc + (size_t)p * MS_COUNT;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    const sc x = ld_sc(&ms[MS_X]);
    const u32 k = (one_phase && a >= 3) ? a + 3 : a;
    const size_t pt = row + k;
    u32* sp = sp_all + pt * 8;
    ge P;
    u32 w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = vpts[pt * 8 + i];
    if (!ge_decode_words(P, w)) {
        atomicMax(&status[p], (int32_t)BBP_ERR_VERIFY);  // optional_multiscalar_mul -> None -> VerificationError
#pragma unroll
        for (int i = 0; i < 8; i++) sp[i] = 0x88888888u;  // all digits zero: the point drops out (its table is never read)
        return;
    }
    sc s;
    if (k < 6) {
        sc xx = sc_mul(x, x);
        s = (k % 3 == 0) ? x : (k % 3 == 1) ? xx : sc_mul(xx, x);
        if (k >= 3) s = sc_mul(s, ld_sc(&ms[MS_U]));
    } else if (k < 6 + m) {
        sc rxx = sc_mul(ld_sc(&ms[MS_R]), sc_mul(x, x));
        s = sc_mul(ld_sc(&wvrow[k - 6]), rxx);
    } else if (k < 6 + m + 5) {
        const u32 e[5] = {1, 3, 4, 5, 6};  // r x, r x^3, r x^4, r x^5, r x^6
        sc xp = x;
        for (u32 i = 1; i < e[k - 6 - m]; i++) xp = sc_mul(xp, x);
        s = sc_mul(ld_sc(&ms[MS_R]), xp);
    } else if (k < 6 + m + 5 + 11) {
        sc uj = ld_sc(&vc[VC_U + (k - 6 - m - 5)]);
        s = sc_mul(uj, uj);
    } else {
        sc ui = ld_sc(&vc[VC_UI + (k - 6 - m - 5 - 11)]);
        s = sc_mul(ui, ui);
    }
    if (agg) s = sc_mul(s, ld_sc(&ms[MS_RHO]));
    u64 cy = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        cy += (u64)s.v[i] + 0x88888888u;
        sp[i] = (u32)cy;
        cy >>= 32;
    }
    ge* tab = tab_all + pt * 8;  // 1P .. 8P
    tab[0] = P;
    ge cur = P;
    for (int i = 1; i < 8; i++) {
        cur = ge_add(cur, P);
        tab[i] = cur;
    }
}

__device__ __forceinline__ ge varsum_lane(u32 lane, u32 m, size_t row, const ge* __restrict__ tab_all, const u32* __restrict__ sp_all, u32 one_phase) {
    const u32 np = vnpts(m);
    const u32 npa = one_phase ? np - 3 : np;
    ge acc = ge_identity();
    {
        // 2. digit positions 2 lane + 1 (first) and 2 lane of every point; both sit in word lane / 4 of the point's digit string
#pragma unroll 1
        for (int hi = 1; hi >= 0; hi--) {
            if (!hi) {
#pragma unroll 1
                for (int i = 0; i < 4; i++) acc = ge_dbl(acc);
            }
            const u32 j = 2 * lane + (u32)hi;
#pragma unroll 1
            for (u32 a = 0; a < npa; a++) {
                const u32 k = (one_phase && a >= 3) ? a + 3 : a;
                const size_t pt = row + k;
                const int d = (int)((sp_all[pt * 8 + (j >> 3)] >> (4 * (j & 7))) & 15u) - 8;
                if (d != 0) {
                    ge e = tab_all[pt * 8 + (d > 0 ? d : -d) - 1];
                    if (d < 0) e = ge_neg(e);
                    acc = ge_add(acc, e);
                }
            }
        }
        // 3. into place: 2^(8 lane)
#pragma unroll 1
        for (u32 i = 0; i < 8 * lane; i++) acc = ge_dbl(acc);
    }
    return acc;
}
// 4. the sum over the 32 lanes of a proof (every lane of the wavefront takes part in the shuffles)
__device__ __forceinline__ ge varsum_reduce(ge acc, u32 lane) {
#pragma unroll 1
    for (int d = 16; d >= 1; d >>= 1) {
        const ge other = v_shfl_down32(acc, d);
        if (lane < (u32)d) acc = ge_add(acc, other);
    }
    return acc;
}

__device__ __forceinline__ void powers_chunk(u32 p, u32 c, u32 count, const sc* __restrict__ misc, int slot, sc* __restrict__ out, u32 out_stride,
                                             u32 mont_out) {
    sc x = ld_sc(&misc[(size_t)p * MS_COUNT + slot]);
    sc xm = sc_to_mont(x);
    sc cur = sc_pow_small(x, c * 32);
    if (mont_out) cur = sc_to_mont(cur);
    sc* o = out + (size_t)p * out_stride;
    u32 end = min(count, c * 32 + 32);
    for (u32 e = c * 32; e < end; e++) {
        st_sc(&o[e], cur);
        cur = sc_montmul(cur, xm);
    }
}

// target k of one proof: zp its z powers, wvrow its wV (wl / wr / wo: [p][wstride])
__device__ __forceinline__ void flatten_target(u32 p, u32 k, u32 n_mul, const u32* __restrict__ f_off, const u32* __restrict__ f_ent,
                                               const sc* __restrict__ zp, sc* __restrict__ wl, sc* __restrict__ wr, sc* __restrict__ wo,
                                               sc* __restrict__ wvrow, u32 wstride) {
    sc acc = sc_zero();
    // eight entries at a time: their powers are fetched together (independent loads).  A handful of targets -- a MiMC key, the
    // hash input x -- sit in several hundred constraints, and one load round trip per entry made those lanes the whole kernel
    // (334 us for ONE proof)
    const u32 e0 = f_off[k], e1 = f_off[k + 1];
    for (u32 e = e0; e < e1; e += 8) {
        u32 w[8];
        sc zq[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = f_ent[min(e + (u32)i, e1 - 1)];
#pragma unroll
        for (int i = 0; i < 8; i++) zq[i] = ld_sc(&zp[(w[i] & 0x7fffffffu) + 1]);
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (e + (u32)i < e1) acc = (w[i] >> 31) ? sc_sub(acc, zq[i]) : sc_add(acc, zq[i]);
    }
    sc* dst = k < n_mul ? &wl[(size_t)p * wstride + k]
              : k < 2 * n_mul ? &wr[(size_t)p * wstride + (k - n_mul)]
              : k < 3 * n_mul ? &wo[(size_t)p * wstride + (k - 2 * n_mul)]
                              : &wvrow[k - 3 * n_mul];
    st_sc(dst, acc);
}

// ---- the front-end kernels of a mixed call (vstride: vpts words per row, np_stride = vstride / 8 points per row) -------------
__global__ BBP_LANE_KERNEL void k_vparse_mx(u32 B, const VRow* __restrict__ rows, u32 vstride, u32 cst_stride, const u8* __restrict__ in,
                                            u32* __restrict__ vpts, sc* __restrict__ vchal, sc* __restrict__ cst_all, int32_t* __restrict__ status) {
    BBP_THIN_PRIO();
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const VRow r = rows[p];
    vparse_row(p, r.n, r.ver, in + r.off, vpts + (size_t)p * vstride, vchal, cst_all + (size_t)p * cst_stride, status);
}

// (held at one wave per SIMD like k_vtranscript, whose 256 + 12 registers it matches: left to itself the compiler aims at two waves
// and spills 704 bytes a lane instead of 624)
__global__ BBP_LANE_KERNEL __attribute__((amdgpu_waves_per_eu(1, 1))) void k_vtranscript_mx(u32 B, const VRow* __restrict__ rows, u32 vstride, merlin_transcript prefix, const u32* __restrict__ vpts,
                                                 const u8* __restrict__ entropy, sc* __restrict__ vchal, sc* __restrict__ misc,
                                                 int32_t* __restrict__ status, u32 wave) {
    BBP_VTR_PRIO_SET();
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (wave) p >>= 6;
    if (p >= B) return;
    vtranscript_row(p, rows[p].m, prefix, vpts + (size_t)p * vstride, entropy, vchal, misc, status, wave);
}

// z^0 .. z^n_cons of each row's own circuit; chunks_max chunks of 32 per row
__global__ BBP_LANE_KERNEL void k_powers_mx(u32 B, u32 chunks_max, const VRow* __restrict__ rows, const VCirc* __restrict__ ctab,
                                            const sc* __restrict__ misc, int slot, sc* __restrict__ out, u32 out_stride) {
    BBP_THIN_PRIO();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * chunks_max) return;
    const u32 p = t / chunks_max, c = t % chunks_max;
    const u32 count = ctab[rows[p].n].n_cons + 1;
    if (c * 32 >= count) return;
    powers_chunk(p, c, count, misc, slot, out, out_stride, 0u);
}

__global__ void k_flatten_mx(u32 B, u32 n_tgt_max, const VRow* __restrict__ rows, const VCirc* __restrict__ ctab, const sc* __restrict__ zpow,
                             u32 zstride, sc* __restrict__ wl, sc* __restrict__ wr, sc* __restrict__ wo, sc* __restrict__ wv, u32 wv_stride) {
    BBP_THIN_PRIO();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * n_tgt_max) return;
    const u32 p = t / n_tgt_max, k = t % n_tgt_max;
    const VRow r = rows[p];
    const VCirc& c = ctab[r.n];
    if (k >= 3 * c.n_mul + r.m) return;
    flatten_target(p, k, c.n_mul, c.f_off, c.f_ent, zpow + (size_t)p * zstride, wl, wr, wo, wv + (size_t)p * wv_stride, IPA_N);
}

__global__ __launch_bounds__(VS_BLK) void k_vscalars_mx(const VRow* __restrict__ rows, const VCirc* __restrict__ ctab, u32 cst_stride, u32 zstride,
                                                         const sc* __restrict__ cst_all, const sc* __restrict__ zpow, const sc* __restrict__ yipow,
                                                         const sc* __restrict__ wl, const sc* __restrict__ wr, const sc* __restrict__ wo,
                                                         const sc* __restrict__ vchal, sc* __restrict__ misc, sc* __restrict__ s_all,
                                                         sc* __restrict__ vs_all, u32 agg) {
    __builtin_amdgcn_s_setprio(BBP_VSC_PRIO);
    const u32 p = blockIdx.x;
    const VCirc& c = ctab[rows[p].n];
    vscalars_block(p, c.n_mul, c.n_cterms, c.c_q, c.c_cst, cst_all + (size_t)p * cst_stride, zpow + (size_t)p * zstride, yipow, wl, wr, wo, vchal,
                   misc, s_all, vs_all, agg);
}

// The record layout is the row's own: a compact row has no A_I2 / A_O2 / S2 and skips those three point slots, a two-phase row
// weighs them, so the number of active points differs per row (npa_max: the call's largest).  The transcript replay needs no
// version: it absorbs the three slots as they stand in vpts, and k_vparse_mx has zeroed them (the identity) for a compact row.
__global__ __launch_bounds__(64) void k_varprep_mx(u32 B, u32 npa_max, u32 np_stride, const VRow* __restrict__ rows, const u32* __restrict__ vpts,
                                                    const sc* __restrict__ vchal, const sc* __restrict__ misc, const sc* __restrict__ wv, u32 wv_stride,
                                                    ge* __restrict__ tab_all, u32* __restrict__ sp_all, int32_t* __restrict__ status, u32 agg) {
    BBP_THIN_PRIO();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;  // one lane per (row, point slot)
    if (t >= B * npa_max) return;
    const u32 p = t / npa_max, a = t % npa_max;
    const VRow r = rows[p];
    const u32 m = r.m, one_phase = r.ver ? 0u : 1u;
    if (a >= vnpts(m) - 3 * one_phase) return;
    varprep_point(p, a, m, (size_t)p * np_stride, vpts, vchal, misc, wv + (size_t)p * wv_stride, tab_all, sp_all, status, agg, one_phase);
}

__global__ __launch_bounds__(64) void k_varsum_mx(u32 B, u32 np_stride, const VRow* __restrict__ rows, const ge* __restrict__ tab_all,
                                                   const u32* __restrict__ sp_all, ge* __restrict__ out) {
    BBP_VARBASE_PRIO_SET();
    const u32 lane = threadIdx.x & 31u;
    const u32 p = blockIdx.x * 2 + (threadIdx.x >> 5);
    const bool live = p < B;
    ge acc = ge_identity();
    if (live) acc = varsum_lane(lane, rows[p].m, (size_t)p * np_stride, tab_all, sp_all, rows[p].ver ? 0u : 1u);
    acc = varsum_reduce(acc, lane);
    if (live && lane == 0) out[p] = acc;
}

__global__ __launch_bounds__(64) void k_varbase_mx(u32 B, u32 Q, u32 np_stride, const VRow* __restrict__ rows, const u32* __restrict__ vpts,
                                                    const sc* __restrict__ vchal, const sc* __restrict__ misc, const sc* __restrict__ wv, u32 wv_stride,
                                                    ge* __restrict__ tab_all, u32* __restrict__ sp_all, ge* __restrict__ out, int32_t* __restrict__ status,
                                                    u32 agg) {
    BBP_VARBASE_PRIO_SET();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * Q) return;
    const u32 p = t / Q, q = t % Q;
    out[(size_t)p * Q + q] = varbase_lane(p, q, Q, rows[p].m, (size_t)p * np_stride, vpts, vchal, misc, wv + (size_t)p * wv_stride, tab_all, sp_all,
                                          status, agg, rows[p].ver ? 0u : 1u);
}

// ---- rounds (bbp_verify_rounds*): rows carry record || score || z_img; seed and bid list come once per round ---------------------
// The caller's round table is round r = seed || pub_list(N_r), packed: scalar roff[r] of the table is round r's seed, the N_r
// scalars behind it its items, roff[R] the total.  k_round_consts reduces the table ONCE per call into a block of the same layout
// (what k_vparse does per row: canonicity of the seed, sc_reduce256, Scalar::from_bits for the items), the parse kernels below copy
// a row's constants from it.  Only these read the short rows; everything from the transcript replay on is the existing front end.
__host__ __device__ __forceinline__ u64 vround_row_bytes(u32 n) { return 1121u + 32u * (4u + n) + 64u; }  // record || score || z_img

// one lane per scalar of the table; rflag[r]: BBP_ERR_FORMAT for a non-canonical seed (a serde-deserialised Scalar, as in k_vparse)
__global__ BBP_LANE_KERNEL void k_round_consts(u32 R, const u32* __restrict__ roff, const u8* __restrict__ rounds, sc* __restrict__ rblk,
                                               int32_t* __restrict__ rflag) {
    BBP_THIN_PRIO();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= roff[R]) return;
    u32 lo = 0, hi = R;  // roff[lo] <= t < roff[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (roff[mid] <= t) lo = mid;
        else hi = mid;
    }
    const u8* b = rounds + 32 * (size_t)t;
    u32 w[8];
    for (int i = 0; i < 8; i++) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
    if (t == roff[lo]) {
        rflag[lo] = sc_is_canonical(w) ? (int32_t)BBP_OK : (int32_t)BBP_ERR_FORMAT;
        st_sc(&rblk[t], sc_reduce256(w));
    } else
        st_sc(&rblk[t], sc_from_bits(w));
}

// vparse_row for a compact record and a short row: rb is the row's round in the reduced block (seed, then the items), rfl its flag.
// The outer loops stay rolled: unrolled, the byte loads of several fields are in flight at once and the two kernels below need
// 78 / 84 VGPRs; rolled they need 64 each, below k_vparse (68) and k_vparse_mx (96).
__device__ __forceinline__ void vparse_round_row(u32 p, u32 n_items, const u8* __restrict__ r, const sc* __restrict__ rb, int32_t rfl,
                                                 u32* __restrict__ o, sc* __restrict__ vchal, sc* __restrict__ cst, int32_t* __restrict__ status) {
    const u32 m = 4 + n_items;
    int32_t st = rfl;
    if (r[0] != 0) st = BBP_ERR_FORMAT;  // compact records only
    auto ldw = [&](const u8* b, u32* w) {
        for (int i = 0; i < 8; i++) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
    };
    st_sc(&cst[circuit::CST_SEED], ld_sc(&rb[0]));
#pragma unroll 1
    for (u32 i = 0; i < n_items; i++) st_sc(&cst[circuit::CST_ITEM0 + i], ld_sc(&rb[1 + i]));
    const u8* q = r + 1;
#pragma unroll 1
    for (u32 i = 0; i < 3; i++, q += 32) ldw(q, o + 8 * i);
#pragma unroll 1
    for (u32 i = 24; i < 48; i++) o[i] = 0;  // A_I2 = A_O2 = S2 = identity
#pragma unroll 1
    for (u32 i = 0; i < 5; i++, q += 32) ldw(q, o + 8 * (6 + m + i));
    sc* vc = vchal + (size_t)p * VC_COUNT;
    u32 w[8];
#pragma unroll 1
    for (u32 i = 0; i < 3; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&vc[VC_TX + i], BBP_SC_LIT(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
    }
#pragma unroll 1
    for (u32 j = 0; j < 11; j++, q += 64) {
        ldw(q, o + 8 * (6 + m + 5 + j));
        ldw(q + 32, o + 8 * (6 + m + 5 + 11 + j));
    }
#pragma unroll 1
    for (u32 i = 0; i < 2; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&vc[VC_A + i], BBP_SC_LIT(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
    }
#pragma unroll 1
    for (u32 i = 0; i < m; i++, q += 32) ldw(q, o + 8 * (6 + i));
    st_sc(&cst[circuit::CST_ONE], sc_one());
    st_sc(&cst[circuit::CST_ZERO], sc_zero());
    const u32 pub_slot[2] = {circuit::CST_Q, circuit::CST_ZIMG};  // score, z_img: the row's own, screened like k_vparse's
#pragma unroll 1
    for (u32 i = 0; i < 2; i++, q += 32) {
        ldw(q, w);
        if (!sc_is_canonical(w)) st = BBP_ERR_FORMAT;
        st_sc(&cst[pub_slot[i]], sc_reduce256(w));
    }
    status[p] = st;
}

// one round: feeds the uniform front end (the reduced block is one round: the loads from it are the same for every lane)
__global__ BBP_LANE_KERNEL void k_vparse_round(u32 B, u32 n_items, u32 n_cst, const u8* __restrict__ in, const sc* __restrict__ rblk,
                                               const int32_t* __restrict__ rflag, u32* __restrict__ vpts, sc* __restrict__ vchal,
                                               sc* __restrict__ cst_all, int32_t* __restrict__ status) {
    BBP_THIN_PRIO();
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    vparse_round_row(p, n_items, in + vround_row_bytes(n_items) * p, rblk, rflag[0], vpts + (size_t)p * vnpts(4 + n_items) * 8, vchal,
                     cst_all + (size_t)p * n_cst, status);
}

// several rounds: k_vrows for the short rows (N of a row from its round), and the parse that feeds the mixed front end
__global__ __launch_bounds__(VROWS_BLK) void k_vrows_rounds(u32 B, const u32* __restrict__ round_of, const u32* __restrict__ roff,
                                                             VRow* __restrict__ rows) {
    __shared__ u64 part[VROWS_BLK];
    const u32 tid = threadIdx.x, per = (B + VROWS_BLK - 1) / VROWS_BLK;
    const u32 lo = min(B, tid * per), hi = min(B, lo + per);
    auto n_of = [&](u32 i) { return roff[round_of[i] + 1] - roff[round_of[i]] - 1; };
    u64 sum = 0;
    for (u32 i = lo; i < hi; i++) sum += vround_row_bytes(n_of(i));
    part[tid] = sum;
    __syncthreads();
    for (u32 d = 1; d < VROWS_BLK; d <<= 1) {
        const u64 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u64 off = part[tid] - sum;
    for (u32 i = lo; i < hi; i++) {
        const u32 n = n_of(i);
        rows[i] = VRow{off, n, (uint16_t)(4 + n), (uint16_t)0};
        off += vround_row_bytes(n);
    }
}

__global__ BBP_LANE_KERNEL void k_vparse_rounds_mx(u32 B, const VRow* __restrict__ rows, const u32* __restrict__ round_of,
                                                   const u32* __restrict__ roff, u32 vstride, u32 cst_stride, const u8* __restrict__ in,
                                                   const sc* __restrict__ rblk, const int32_t* __restrict__ rflag, u32* __restrict__ vpts,
                                                   sc* __restrict__ vchal, sc* __restrict__ cst_all, int32_t* __restrict__ status) {
    BBP_THIN_PRIO();
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const VRow r = rows[p];
    const u32 rd = round_of[p];
    vparse_round_row(p, r.n, in + r.off, rblk + roff[rd], rflag[rd], vpts + (size_t)p * vstride, vchal, cst_all + (size_t)p * cst_stride, status);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// What the launches of one call take of its circuit or circuits: the counts the plan is made from (verify_plan.h), the generator
// list of the check (the same for every N), and the tables -- the uniform front ends' one circuit, or the mixed ones' ctx->vctab.
struct VerifyCircuit {
    VerifyDims d;
    const u32* idx_ver = nullptr;
    const CircuitDev* uniform = nullptr;
    const VCirc* ctab = nullptr;
};
// Compiles every N of the call on first use (as the uniform calls do) and fills its entry of ctx->vctab; c.d becomes the largest of
// every count over the call's N.  The rows' Ns are host memory and screened by the caller; checked again here because they index the
// device table.
static int32_t mixed_prepare(bbp_ctx* ctx, const VerifyRows& v, VerifyCircuit& c) {
    if (!ctx->vctab) BBP_HIP_TRY(ctx, hipMalloc(&ctx->vctab, sizeof(VCirc) * (BBP_MAX_ITEMS + 1)));
    bool seen[BBP_MAX_ITEMS + 1] = {};
    for (u32 i = 0; i < v.B; i++) {
        const u32 n = v.n_of(i);
        if (n == 0 || n > BBP_MAX_ITEMS) {
            ctx->err = "mixed verification: bid-list length out of range";
            return BBP_ERR_BAD_ARG;
        }
        if (seen[n]) continue;
        seen[n] = true;
        const CircuitDev* cp;
        if (int32_t rc = circuit_get(ctx, n, &cp)) return rc;
        if (!ctx->vctab_has[n]) {
            const VCirc v{cp->n_mul, cp->n_cons, cp->n_cst, cp->n_cterms, cp->f_off, cp->f_ent, cp->c_q, cp->c_cst};
            BBP_HIP_TRY(ctx, hipMemcpy((VCirc*)ctx->vctab + n, &v, sizeof v, hipMemcpyHostToDevice));
            ctx->vctab_has[n] = 1;
        }
        if (!c.idx_ver) c.idx_ver = cp->idx_ver;
        c.d.widen(cp->dims());
    }
    c.ctab = (const VCirc*)ctx->vctab;
    return BBP_OK;
}
// the circuit side of any call: a mixed front end's table, or the one circuit of a uniform one
static int32_t verify_circuit(bbp_ctx* ctx, const VerifyRows& v, VerifyCircuit& c) {
    if (v.mixed_front()) return mixed_prepare(ctx, v, c);
    if (int32_t rc = circuit_get(ctx, v.front_n(), &c.uniform)) return rc;
    c.d = c.uniform->dims(), c.idx_ver = c.uniform->idx_ver;
    return BBP_OK;
}

// The host arrays of a call -- a (na bytes) and, when given, b (nb bytes) right behind it -> dst on s through the lane's pinned
// staging: Ns and the version bytes of a mixed call, round_of and the round offsets of a rounds call.  No synchronisation unless
// NS_RING such calls are still queued on the lane ahead of this one: then the oldest upload is waited for before its staging is
// reused.  An entry grows to what the call needs.
constexpr size_t NS_RING = 16;
static int32_t stage_host(bbp_ctx* ctx, bbp_ctx::VLane& L, const void* a, size_t na, const void* b, size_t nb, void* dst, hipStream_t s) {
    const size_t bytes = na + nb;
    bbp_ctx::VLane::NsStage* st = nullptr;
    for (auto& e : L.ns_ring)
        if (hipEventQuery(e.ev) == hipSuccess) {  // its copy has run (or it was never used)
            st = &e;
            break;
        }
    if (!st && L.ns_ring.size() < NS_RING) {
        L.ns_ring.emplace_back();
        st = &L.ns_ring.back();
        BBP_HIP_TRY(ctx, hipEventCreateWithFlags(&st->ev, hipEventDisableTiming));
    }
    if (!st) {
        st = &L.ns_ring[L.ns_oldest++ % NS_RING];
        BBP_HIP_TRY(ctx, hipEventSynchronize(st->ev));
    }
    if (st->cap < bytes) {
        if (st->h) BBP_HIP_TRY(ctx, hipHostFree(st->h));
        st->h = nullptr;
        st->cap = 0;
        const size_t want = (std::max(bytes + bytes / 2, (size_t)65536) + 15) & ~(size_t)15;  // whole 16-byte grains, like dev_reserve's
        BBP_HIP_TRY(ctx, hipHostMalloc(&st->h, want, hipHostMallocDefault));
        st->cap = want;
    }
    if (na) memcpy(st->h, a, na);
    if (nb) memcpy((u8*)st->h + na, b, nb);
    BBP_HIP_TRY(ctx, hipMemcpyAsync(dst, st->h, bytes, hipMemcpyHostToDevice, s));
    BBP_HIP_TRY(ctx, hipEventRecord(st->ev, s));
    return BBP_OK;
}

}  // namespace bbp
