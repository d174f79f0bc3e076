// Batched R1CS verifier for the blind-bid circuit on gfx950: replaces Verify::verify (src/blindbid/verify.rs:47-89) and
// bulletproofs' Verifier::verify + InnerProductProof::verification_scalars under it (SURVEY.md App. A.7).
//
//   k_vparse       R1CSProof::from_bytes field split + canonical-scalar checks (FormatError), public-input table
//   k_vtranscript  Merlin replay: "V" x m, "m", A_*, y, z, T_*, u, x, t_x.., w, (L_j, R_j, u_j) x 11, verifier's r   (K7)
//   k_powers       z^k, y^-k
//   k_flatten      wL, wR, wO, wV                                                                                   (K4)
//   k_vscalars     wc, s vector, delta, the 4096 generator scalars g[i], h[i] and the B / B~ scalars              (K8)
//   MSM            ONE 4098-term fixed-base MSM per proof over the resident table (k_msm_sort + k_msm_acc)         (K1)
//   k_varbase      decompress the ~45 proof points and multiply each by its scalar (4-bit windows)                (K9)
//   k_vfinal       sum, identity test -> Ok / VerificationError
// (textually included at the end of prover.hip: shares k_powers / k_flatten / k_fill_mimc / block_sum_sc)
namespace bbp {

// wave priority of the verifier's two long-lived thin kernels (the transcript replay: 16 wavefronts for 1 ms per 1024 proofs; the
// variable-base multiplications: 1024 wavefronts for 1 ms): experiments -DBBP_VTR_PRIO / -DBBP_VARBASE_PRIO, DESIGN.md section 6b
#ifndef BBP_VTR_PRIO
#define BBP_VTR_PRIO 3
#endif
#ifndef BBP_VARBASE_PRIO
#define BBP_VARBASE_PRIO 3
#endif
#ifndef BBP_VSC_PRIO
#define BBP_VSC_PRIO 3
#endif
#define BBP_VTR_PRIO_SET() __builtin_amdgcn_s_setprio(BBP_VTR_PRIO)
#define BBP_VARBASE_PRIO_SET() __builtin_amdgcn_s_setprio(BBP_VARBASE_PRIO)

// words_to_bytes32 etc. live in prover.hip as static-inline device helpers; re-declare the few we need
__device__ __forceinline__ void v_words_to_bytes32(uint8_t* o, const u32* w) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        o[4 * i] = (uint8_t)w[i];
        o[4 * i + 1] = (uint8_t)(w[i] >> 8);
        o[4 * i + 2] = (uint8_t)(w[i] >> 16);
        o[4 * i + 3] = (uint8_t)(w[i] >> 24);
    }
}
#define VLBL(s) reinterpret_cast<const uint8_t*>(s), (u32)(sizeof(s) - 1)

__device__ void v_append_words(merlin_transcript& t, const uint8_t* label, u32 llen, const u32* w8) {
    uint8_t b[32];
    v_words_to_bytes32(b, w8);
    merlin_append(t, label, llen, b, 32);
}
__device__ bool v_is_zero8(const u32* w) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}
// validate_and_append_point: the identity encoding is a VerificationError (A.1 tail)
__device__ bool v_validate_append(merlin_transcript& t, const uint8_t* label, u32 llen, const u32* w8) {
    if (v_is_zero8(w8)) return false;
    v_append_words(t, label, llen, w8);
    return true;
}
__device__ sc v_challenge_sc(merlin_transcript& t, const uint8_t* label, u32 llen) {
    uint8_t b[64];
    merlin_challenge(t, label, llen, b, 64);
    u32 w[16];
    for (int i = 0; i < 16; i++) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
    return sc_from_wide(w);
}

// ---- per-proof verifier arrays (alias BatchDev fields) ---------------------------------------------------------
// vpts words per proof: [A_I1 A_O1 S1 A_I2 A_O2 S2 | V[m] | T_1 T_3 T_4 T_5 T_6 | L_1..L_11 | R_1..R_11]   (8 words each)
__device__ __forceinline__ u32 vnpts(u32 m) { return 6 + m + 5 + 22; }
// vchal per proof (scalars): [u_j (11) | u_j^-1 (11) | t_x t_xb e_bl a b (5)]

// rec_ver: 0 = compact 1-phase records (1121 bytes), 1 = 2-phase layout (1217 bytes)
__global__ BBP_LANE_KERNEL void k_vparse(u32 B, u32 n_items, u32 n_cst, u32 rec_ver, const u8* __restrict__ in, u32* __restrict__ vpts, sc* __restrict__ vchal,
                         sc* __restrict__ cst_all, int32_t* __restrict__ status) {
    BBP_THIN_PRIO();
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const u32 m = 4 + n_items;
    const u32 plen = rec_ver ? 1217u : 1121u;
    const size_t stride = (size_t)plen + 32 * (size_t)m + verify_tail_bytes(n_items);
    const u8* r = in + stride * p;
    int32_t st = BBP_OK;
    if (r[0] != (u8)rec_ver) st = BBP_ERR_FORMAT;  // version byte must match the layout implied by the length
    u32* o = vpts + (size_t)p * vnpts(m) * 8;
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
    sc* cst = cst_all + (size_t)p * n_cst;
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

__global__ BBP_LANE_KERNEL void k_vtranscript(u32 B, u32 m, merlin_transcript prefix, const u32* __restrict__ vpts, const u8* __restrict__ entropy,
                              sc* __restrict__ vchal, sc* __restrict__ misc, int32_t* __restrict__ status, u32 wave) {
    BBP_VTR_PRIO_SET();
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (wave) p >>= 6;  // small launches: one proof per wavefront, every lane in lockstep, the permutations spread over the lanes (keccak_wave.h)
    if (p >= B) return;
    const u32* pt = vpts + (size_t)p * vnpts(m) * 8;
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

// wc, s, delta, generator scalars.  vs per proof: [g (2048) | h (2048) | B | B~]
__global__ __launch_bounds__(VS_BLK) void k_vscalars(u32 n1, u32 n_cterms, u32 n_cst, u32 zstride, const u32* __restrict__ c_q,
                                                      const u32* __restrict__ c_cst, const sc* __restrict__ cst_all, const sc* __restrict__ zpow,
                                                      const sc* __restrict__ yipow, const sc* __restrict__ wl, const sc* __restrict__ wr,
                                                      const sc* __restrict__ wo, const sc* __restrict__ vchal, sc* __restrict__ misc,
                                                      sc* __restrict__ s_all, sc* __restrict__ vs_all, u32 agg) {
    __builtin_amdgcn_s_setprio(BBP_VSC_PRIO);
    __shared__ u32 lds[2 * 8 * VS_BLK];
    const u32 p = blockIdx.x, tid = threadIdx.x;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    sc* ms = misc + (size_t)p * MS_COUNT;
    const sc *zp = zpow + (size_t)p * zstride, *cst = cst_all + (size_t)p * n_cst, *YI = yipow + (size_t)p * IPA_N;
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

// K9: the ~45 proof points of one verification: decompress, scalar from the challenge algebra, 4-bit signed windows.
// A proof's points are dealt round-robin to Q lanes; each lane runs Straus over its share -- ONE chain of 256 doublings for
// all of its points instead of one per point (one lane per point costs 44 x (256 + 64) point operations per proof, eight lanes
// per proof 8 x (256 + 6 x 64)) -- and leaves a partial sum in out[p * Q + q].  Q is chosen by the host so that the launch
// still has about one wavefront per SIMD.
// Digits: with s' = s + 0x88..8 (s < 2^253, no overflow) the j-th signed radix-16 digit is nibble_j(s') - 8, in [-8, 7].
__global__ __launch_bounds__(64) void k_varbase(u32 B, u32 m, u32 Q, const u32* __restrict__ vpts, const sc* __restrict__ vchal,
                                                 const sc* __restrict__ misc, const sc* __restrict__ wv, ge* __restrict__ tab_all,
                                                 u32* __restrict__ sp_all, ge* __restrict__ out, int32_t* __restrict__ status, u32 agg,
                                                 u32 one_phase) {
    BBP_VARBASE_PRIO_SET();
    const u32 np = vnpts(m);
    // one-phase records (rec_ver 0) carry no A_I2 / A_O2 / S2: those three slots (k = 3..5) are the identity and are skipped
    const u32 npa = one_phase ? np - 3 : np;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * Q) return;
    const u32 p = t / Q, q = t % Q;
    const sc* ms = misc + (size_t)p * MS_COUNT;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    const sc x = ld_sc(&ms[MS_X]);
    for (u32 a = q; a < npa; a += Q) {
        const u32 k = (one_phase && a >= 3) ? a + 3 : a;
        const size_t pt = (size_t)p * np + k;
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
            s = sc_mul(ld_sc(&wv[(size_t)p * m + (k - 6)]), rxx);
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
            const size_t pt = (size_t)p * np + k;
            const int d = (int)((sp_all[pt * 8 + (j >> 3)] >> (4 * (j & 7))) & 15u) - 8;
            if (d != 0) {
                ge e = tab_all[pt * 8 + (d > 0 ? d : -d) - 1];
                if (d < 0) e = ge_neg(e);
                acc = ge_add(acc, e);
            }
        }
    }
    out[(size_t)p * Q + q] = acc;
}

// K9, round 3: the same sum over a proof's ~41 points with HALF A WAVEFRONT PER PROOF (two proofs per 64-lane workgroup) and the
// doublings shared by all points.  The first version gives every point a lane and a doubling chain of its own: 41 x (252
// doublings + 64 additions) per proof, 1024 wavefronts per 1024 proofs alive for a millisecond at raised priority -- knocking the
// kernel out showed it costs the two-lane pipeline 1.33 ms of a 6.7 ms step, as much as it takes alone.  Here:
//   1. (k_varprep, one lane per point) decode the points, derive their scalars / radix-16 digits and build the 1P..8P tables;
//   2. lane l owns the digit positions 2l and 2l + 1 of EVERY point: S_l = sum_points (16 d_{2l+1} + d_{2l}) P  (82 table additions, 4 doublings);
//   3. lane l shifts its partial sum into place, 8 l doublings (the wavefront runs the longest lane's 248: what one Straus chain costs);
//   4. the 32 partial sums are added up through wave shuffles (5 additions).
// Per proof 41 x 64 additions as before but 4 x 32 + 248 doublings instead of 41 x 252 (-64 % field multiplications), 512
// wavefronts per 1024 proofs instead of 1024, the chain 20 % longer.  One partial sum per proof (nq = 1 for k_vfinal / k_var_sum).
__device__ __forceinline__ ge v_shfl_down32(const ge& p, int d) {  // within each 32-lane half of the wavefront
    ge r;
    const u32* w = reinterpret_cast<const u32*>(&p);
    u32* o = reinterpret_cast<u32*>(&r);
#pragma unroll
    for (int i = 0; i < GE_WORDS; i++) o[i] = (u32)__shfl_down((int)w[i], d, 32);
    return r;
}

// (two kernels: the decode / scalar algebra of step 1 needs 250+ registers, the long chain of steps 2-4 does not -- and only a wave
// of at most 192 registers fits on a SIMD beside the two accumulate waves of the lane next door: compiled as one kernel the whole
// chain ran at 256 + 65 registers and displaced an accumulate wave for as long as it lived)
__global__ __launch_bounds__(64) void k_varprep(u32 B, u32 m, const u32* __restrict__ vpts, const sc* __restrict__ vchal,
                                                 const sc* __restrict__ misc, const sc* __restrict__ wv, ge* __restrict__ tab_all,
                                                 u32* __restrict__ sp_all, int32_t* __restrict__ status, u32 agg, u32 one_phase) {
    BBP_THIN_PRIO();
    const u32 np = vnpts(m);
    const u32 npa = one_phase ? np - 3 : np;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;  // one lane per (proof, point)
    if (t >= B * npa) return;
    const u32 p = t / npa, a = t % npa;
    const sc* ms = misc + (size_t)p * MS_COUNT;
    const sc* vc = vchal + (size_t)p * VC_COUNT;
    const sc x = ld_sc(&ms[MS_X]);
    const u32 k = (one_phase && a >= 3) ? a + 3 : a;
    const size_t pt = (size_t)p * np + k;
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
        s = sc_mul(ld_sc(&wv[(size_t)p * m + (k - 6)]), rxx);
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

__global__ __launch_bounds__(64) void k_varsum(u32 B, u32 m, const ge* __restrict__ tab_all, const u32* __restrict__ sp_all, ge* __restrict__ out,
                                                u32 one_phase) {
    BBP_VARBASE_PRIO_SET();
    const u32 np = vnpts(m);
    const u32 npa = one_phase ? np - 3 : np;
    const u32 lane = threadIdx.x & 31u;
    const u32 p = blockIdx.x * 2 + (threadIdx.x >> 5);
    const bool live = p < B;  // (an odd B leaves the second half of the last wavefront without a proof: it still takes part in the shuffles)
    ge acc = ge_identity();
    if (live) {
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
                const size_t pt = (size_t)p * np + k;
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
    // 4. sum over the 32 lanes of the proof (every lane of the wavefront takes part in the shuffles)
#pragma unroll 1
    for (int d = 16; d >= 1; d >>= 1) {
        const ge other = v_shfl_down32(acc, d);
        if (lane < (u32)d) acc = ge_add(acc, other);
    }
    if (live && lane == 0) out[p] = acc;
}

// nq partial sums per proof in var (k_varbase: Q of them; k_varbase2: one)
__global__ BBP_LANE_KERNEL void k_vfinal(u32 B, u32 nq, const ge* __restrict__ fixed, const ge* __restrict__ var, int32_t* __restrict__ status) {
    BBP_THIN_PRIO();
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    ge acc = fixed[p];
    for (u32 k = 0; k < nq; k++) acc = ge_add(acc, var[(size_t)p * nq + k]);
    if (status[p] == BBP_OK && !ge_is_identity(acc)) status[p] = BBP_ERR_VERIFY;
}


// ---- aggregated verification (SURVEY.md 8f-4; the reference has no equivalent) ------------------------------------------------
// The per-proof check  sum_i vs[p][i] Base_i + sum_k sv[p][k] P[p][k] == 0  is linear, so a group of proofs is checked at once
// with random weights rho_p (drawn from each proof's own verifier TranscriptRng, seeded with the caller's entropy):
//   sum_i (sum_p rho_p vs[p][i]) Base_i + sum_p sum_k rho_p sv[p][k] P[p][k] == 0
// -- ONE 4098-term fixed-base MSM per group instead of one per proof.  A group that fails is verified again proof by proof
// (verify_batch_agg_dev), so the per-proof statuses are those of the plain path (a bad proof passing needs a ~2^-250 accident).
__global__ __launch_bounds__(GS_BLK) void k_group_sum(u32 B, u32 G, const sc* __restrict__ vs_all, const int32_t* __restrict__ status,
                                                       sc* __restrict__ vsg) {
    const u32 i = blockIdx.x * GS_BLK + threadIdx.x, g = blockIdx.y;
    if (i >= 4098u) return;
    const u32 p0 = g * G, p1 = min(B, p0 + G);
    sc acc = sc_zero();
    for (u32 p = p0; p < p1; p++)
        if (status[p] == BBP_OK) acc = sc_add(acc, ld_sc(&vs_all[(size_t)p * 4098 + i]));  // proofs already rejected stay out of the sum
    st_sc(&vsg[(size_t)g * 4098 + i], acc);
}

__global__ BBP_LANE_KERNEL void k_var_sum(u32 B, u32 nq, const ge* __restrict__ var, const int32_t* __restrict__ status, ge* __restrict__ varsum) {
    BBP_THIN_PRIO();
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    ge acc = ge_identity();
    if (status[p] == BBP_OK)
        for (u32 k = 0; k < nq; k++) acc = ge_add(acc, var[(size_t)p * nq + k]);
    varsum[p] = acc;
}

__global__ BBP_LANE_KERNEL void k_group_final(u32 B, u32 G, u32 n_groups, const ge* __restrict__ fixedg, const ge* __restrict__ varsum,
                                               int32_t* __restrict__ gstatus) {
    BBP_THIN_PRIO();
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const u32 p0 = g * G, p1 = min(B, p0 + G);
    ge acc = fixedg[g];
    for (u32 p = p0; p < p1; p++) acc = ge_add(acc, varsum[p]);
    gstatus[g] = ge_is_identity(acc) ? (int32_t)BBP_OK : (int32_t)BBP_ERR_VERIFY;
}

// Fallback of a failing group, sized ON THE DEVICE: k_compact_failing lists the members of failing groups that are still OK
// (count in counters[0], also added to the running total counters[1]); the MSM kernels are launched for the largest possible
// number of proofs and leave at once beyond the count, reading the weighted generator scalars of proof idx[j] in place (they are
// still in memory from the group pass); rho_p (sum_i vs[p][i] Base_i + var_p) = 0 is the proof's own check (rho_p != 0).
__global__ void k_compact_failing(u32 B, u32 G, u32 n_groups, const int32_t* __restrict__ gstatus, const int32_t* __restrict__ status,
                                  u32* __restrict__ idx, u32* __restrict__ counters) {
    __shared__ u32 n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    for (u32 p = threadIdx.x; p < B; p += blockDim.x)
        if (gstatus[p / G] != BBP_OK && status[p] == BBP_OK) idx[atomicAdd(&n, 1u)] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        counters[0] = n;
        counters[1] += n;
    }
}

__global__ BBP_LANE_KERNEL void k_fallback_final(const u32* __restrict__ counters, const u32* __restrict__ idx, const ge* __restrict__ fixed_c,
                                                  const ge* __restrict__ varsum, int32_t* __restrict__ status, u32* __restrict__ total_out) {
    BBP_THIN_PRIO();
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && total_out) *total_out = counters[1];  // running total of the host call's chunks, next to its statuses
    if (j >= counters[0]) return;
    const u32 p = idx[j];
    if (!ge_is_identity(ge_add(fixed_c[j], varsum[p]))) status[p] = BBP_ERR_VERIFY;
}


}  // namespace bbp
#include "verifier_mixed.inc"
namespace bbp {

// in_dev: B * (record || score || z_img || seed || pub_list); ent_dev: B * 32; status_dev: B * int32
// G = 0: every proof gets its own mega-check MSM (the reference's semantics, one Verifier::verify per proof).
// G > 0: groups of G proofs share one weighted check; status_dev then only carries the rejections found before the group
//        check (format, identity or undecodable points) and the per-group verdicts land in ctx->agg (see verify_batch_agg_dev).
static int vlane_of(const bbp_ctx* ctx, hipStream_t s) {  // a lane's own stream selects it; any other stream is lane 0
    for (int i = 1; i < bbp_ctx::VLANES; i++)
        if (s == ctx->vl[i].stream) return i;
    return 0;
}

// The variable-base launches of one call, in one place: verify_batch_dev and bbp_debug_varbase (the kernel tests) share the geometry
// (verify_plan.h varbase_geom).  mixed: the _mx kernels (m, np, npa those of the call's largest row: the strides).
struct VarbaseLaunch {
    bool mixed;
    VarbaseGeom g;
    const VRow* rows;
    const u32* vpts;
    const sc *vchal, *misc, *wv;
    ge *tab, *var;
    u32* sp;
    int32_t* status;
};
static int32_t varbase_launch(bbp_ctx* ctx, const VarbaseLaunch& v, hipStream_t st, u32 agg_flag) {
    const VarbaseGeom& g = v.g;
    const u32 B = g.B, Q = g.Q, m = g.m, np = g.np, npa = g.npa;
    if (v.mixed) {
        if (g.vb2) {
            LAUNCH(ctx, TAG_VARBASE, k_varprep_mx, g.prep.grid, g.prep.block, st, B, npa, np, v.rows, v.vpts, v.vchal, v.misc, v.wv, m, v.tab, v.sp, v.status,
                   agg_flag);
            LAUNCH(ctx, TAG_VARBASE, k_varsum_mx, g.sum.grid, g.sum.block, st, B, np, v.rows, (const ge*)v.tab, (const u32*)v.sp, v.var);
        } else
            LAUNCH(ctx, TAG_VARBASE, k_varbase_mx, g.lanes.grid, g.lanes.block, st, B, Q, np, v.rows, v.vpts, v.vchal, v.misc, v.wv, m, v.tab, v.sp, v.var,
                   v.status, agg_flag);
    } else if (g.vb2) {
        LAUNCH(ctx, TAG_VARBASE, k_varprep, g.prep.grid, g.prep.block, st, B, m, v.vpts, v.vchal, v.misc, v.wv, v.tab, v.sp, v.status, agg_flag, g.one_phase);
        LAUNCH(ctx, TAG_VARBASE, k_varsum, g.sum.grid, g.sum.block, st, B, m, (const ge*)v.tab, (const u32*)v.sp, v.var, g.one_phase);
    } else
        LAUNCH(ctx, TAG_VARBASE, k_varbase, g.lanes.grid, g.lanes.block, st, B, m, Q, v.vpts, v.vchal, v.misc, v.wv, v.tab, v.sp, v.var, v.status, agg_flag,
               g.one_phase);
    return BBP_OK;
}

// The lane's scratch as typed pointers: made from the plan's layouts here and nowhere else.
struct VerifyBufs {
    u32 *vpts, *sp;
    sc *vchal, *vs, *rblk, *vsg;  // (vsg, fixedg, varsum, gstatus: L.agg, the aggregated pass)
    ge *tab, *var, *fixed;
    VRow* rows;
    u8* ns;           // a mixed call's Ns, then its version bytes
    u32* round_of;    // a rounds call: round_of (several rounds only) ...
    const u32* roff;  // ... and the R + 1 round offsets behind it
    int32_t *rflag, *gstatus;
    ge *fixedg, *varsum;
    VerifyBufs(const VerifyPlan& p, void* misc_base, void* agg_base) {
        u8 *b = static_cast<u8*>(misc_base), *a = static_cast<u8*>(agg_base);
        const VerifyPlan::Misc& m = p.misc;
        vpts = (u32*)(b + m.vpts.off), vchal = (sc*)(b + m.vchal.off), vs = (sc*)(b + m.vs.off), tab = (ge*)(b + m.tab.off), var = (ge*)(b + m.var.off);
        fixed = (ge*)(b + m.fixed.off), sp = (u32*)(b + m.sp.off), rows = (VRow*)(b + m.rows.off), ns = b + m.ns.off;
        round_of = (u32*)(b + m.rof.off), roff = round_of + p.rd_nof, rblk = (sc*)(b + m.rblk.off), rflag = (int32_t*)(b + m.rflag.off);
        vsg = (sc*)(a + p.agg.vsg.off), fixedg = (ge*)(a + p.agg.fixedg.off), varsum = (ge*)(a + p.agg.varsum.off), gstatus = (int32_t*)(a + p.agg.gstatus.off);
    }
};

// One device call while it is enqueued: what its steps share, and the steps in the order verify_batch_dev takes them.
struct VerifyCall {
    bbp_ctx* ctx;
    bbp_ctx::VLane& L;
    int lane;
    hipStream_t s;
    const VerifyRows& v;
    const VerifyPlan& p;
    const VerifyCircuit& c;
    const BatchDev& bd;
    const VerifyBufs& b;
    const u8 *in_dev, *ent_dev;
    int32_t* status_dev;
    int ko;        // knock-out mask: 0 in the product
    bool overlap;  // the variable-base part runs on a second stream beside the generator scalars and the MSM

    // the host arrays of a mixed or rounds call go up; the kernels that turn them into row descriptors and the reduced round table
    int32_t stage_rows() const {
        const u32 B = p.B;
        int32_t rc;
        if (p.rounds) {
            if ((rc = stage_host(ctx, L, v.round_of, 4 * (size_t)p.rd_nof, p.rd_off.data(), 4 * ((size_t)p.R + 1), b.round_of, s))) return rc;
            LAUNCH(ctx, TAG_TRANSCRIPT, k_round_consts, p.round_consts.grid, p.round_consts.block, s, p.R, b.roff, v.rounds, b.rblk, b.rflag);
            if (p.mixed) LAUNCH(ctx, TAG_TRANSCRIPT, k_vrows_rounds, p.vrows.grid, p.vrows.block, s, B, (const u32*)b.round_of, b.roff, b.rows);
        } else if (p.mixed) {
            if ((rc = stage_host(ctx, L, v.ns, 4 * (size_t)B, v.vers, v.vers ? (size_t)B : 0, b.ns, s))) return rc;
            LAUNCH(ctx, TAG_TRANSCRIPT, k_vrows, p.vrows.grid, p.vrows.block, s, B, (const u32*)b.ns, v.vers ? (const u8*)(b.ns + 4 * (size_t)B) : nullptr, b.rows);
        }
        return BBP_OK;
    }

    // parse, transcript replay, z and y^-1 powers, flatten
    int32_t front() const {
        const VerifyDims& d = p.d;
        const BatchStrides st = batch_strides(d);  // elements per proof of bd's arrays (batch_layout.h)
        const u32 B = p.B, N = v.front_n(), m = d.m;
        const VRow* rows = b.rows;
        int32_t rc;
        LAUNCH(ctx, TAG_WITNESS, k_fill_mimc, p.fill_mimc.grid, p.fill_mimc.block, s, B, d.n_cst, ctx->mimc_c, bd.cst);
        switch (p.front) {
            case VerifyPlan::ROUNDS_MX:
                LAUNCH(ctx, TAG_TRANSCRIPT, k_vparse_rounds_mx, p.parse.grid, p.parse.block, s, B, rows, (const u32*)b.round_of, b.roff, p.vstride, d.n_cst, in_dev,
                       (const sc*)b.rblk, (const int32_t*)b.rflag, b.vpts, b.vchal, bd.cst, status_dev);
                break;
            case VerifyPlan::ROUND1:
                LAUNCH(ctx, TAG_TRANSCRIPT, k_vparse_round, p.parse.grid, p.parse.block, s, B, N, d.n_cst, in_dev, (const sc*)b.rblk, (const int32_t*)b.rflag, b.vpts,
                       b.vchal, bd.cst, status_dev);
                break;
            case VerifyPlan::MIXED:
                LAUNCH(ctx, TAG_TRANSCRIPT, k_vparse_mx, p.parse.grid, p.parse.block, s, B, rows, p.vstride, d.n_cst, in_dev, b.vpts, b.vchal, bd.cst, status_dev);
                break;
            case VerifyPlan::UNIFORM:
                LAUNCH(ctx, TAG_TRANSCRIPT, k_vparse, p.parse.grid, p.parse.block, s, B, N, d.n_cst, v.rec_ver, in_dev, b.vpts, b.vchal, bd.cst, status_dev);
                break;
        }
        const merlin_transcript prefix = prover_prefix();
        // BBP_V_FENCE=1 (experiment): the transcript replay's serial waves get CUs of their own like the prover's opening kernels
        const bool fence = ctx->vknobs.fence && ctx->knobs.serial_lds > 0;
        if (ko & 4) {
        } else if (p.mixed) {
            u32 hog = lds_token(ctx);
            if (fence && (rc = serial_lds_bytes(ctx, (const void*)k_vtranscript_mx, &hog))) return rc;
            LAUNCH_LDS(ctx, TAG_TRANSCRIPT, k_vtranscript_mx, p.transcript.grid, p.transcript.block, hog, s, B, rows, p.vstride, prefix, b.vpts, ent_dev, b.vchal,
                       bd.misc, status_dev, p.vtw);
        } else if (fence) {
            u32 hog = 0;
            if ((rc = serial_lds_bytes(ctx, (const void*)k_vtranscript, &hog))) return rc;
            LAUNCH_LDS(ctx, TAG_TRANSCRIPT, k_vtranscript, p.transcript.grid, p.transcript.block, hog, s, B, m, prefix, b.vpts, ent_dev, b.vchal, bd.misc, status_dev,
                       p.vtw);
        } else
            LAUNCH(ctx, TAG_TRANSCRIPT, k_vtranscript, p.transcript.grid, p.transcript.block, s, B, m, prefix, b.vpts, ent_dev, b.vchal, bd.misc, status_dev, p.vtw);
        if (!(ko & 32)) {
            if (p.mixed)
                LAUNCH(ctx, TAG_POLY, k_powers_mx, p.powers_z.grid, p.powers_z.block, s, B, p.zchunks, rows, c.ctab, bd.misc, (int)MS_Z, bd.zpow, p.zstride);
            else
                LAUNCH(ctx, TAG_POLY, k_powers, p.powers_z.grid, p.powers_z.block, s, B, p.zstride, bd.misc, (int)MS_Z, bd.zpow, p.zstride, 0u);
            LAUNCH(ctx, TAG_POLY, k_powers, p.powers_yinv.grid, p.powers_yinv.block, s, B, st.yipow, bd.misc, (int)MS_YINV, bd.yipow, st.yipow, 1u);  // y^-i R
        }
        if (ko & 8) {
        } else if (p.mixed)
            LAUNCH(ctx, TAG_POLY, k_flatten_mx, p.flatten.grid, p.flatten.block, s, B, p.n_tgt, rows, c.ctab, bd.zpow, p.zstride, bd.wl, bd.wr, bd.wo, bd.wv, m);
        else
            LAUNCH(ctx, TAG_POLY, k_flatten, p.flatten.grid, p.flatten.block, s, B, p.n_tgt, d.n_mul, m, c.uniform->f_off, c.uniform->f_ent, bd.zpow, p.zstride, bd.wl,
                   bd.wr, bd.wo, bd.wv, st.wl);
        return BBP_OK;
    }

    int32_t varbase(hipStream_t st) const {
        const VarbaseLaunch vb{p.mixed, p.vb, b.rows, b.vpts, b.vchal, bd.misc, bd.wv, b.tab, b.var, b.sp, status_dev};
        return varbase_launch(ctx, vb, st, p.agg_flag);
    }
    // The variable-base part needs only the challenges and wV: it runs on a second stream beside the generator scalars and the
    // MSM (BBP_VERIFY_OVERLAP=0: on the caller's stream after them) and joins before the first kernel that reads its sums / status.
    int32_t fork_varbase() const {
        if (!overlap) return BBP_OK;
        hipStream_t side = ctx->lane[1];
        BBP_HIP_TRY(ctx, hipEventRecord(L.ev_vfork, s));
        BBP_HIP_TRY(ctx, hipStreamWaitEvent(side, L.ev_vfork, 0));
        if (int32_t rc = varbase(side)) return rc;
        BBP_HIP_TRY(ctx, hipEventRecord(L.ev_vjoin, side));
        return BBP_OK;
    }
    // ... the join, or the launches themselves on the caller's stream when the call did not fork
    int32_t join_varbase() const {
        if (!overlap) return varbase(s);
        BBP_HIP_TRY(ctx, hipStreamWaitEvent(s, L.ev_vjoin, 0));
        return BBP_OK;
    }

    int32_t scalars() const {
        const VerifyDims& d = p.d;
        if (ko & 16) {
        } else if (p.mixed)
            LAUNCH(ctx, TAG_VERIFY_SCALARS, k_vscalars_mx, p.vscalars.grid, p.vscalars.block, s, (const VRow*)b.rows, c.ctab, d.n_cst, p.zstride, bd.cst, bd.zpow,
                   bd.yipow, bd.wl, bd.wr, bd.wo, b.vchal, bd.misc, bd.a, b.vs, p.agg_flag);
        else
            LAUNCH(ctx, TAG_VERIFY_SCALARS, k_vscalars, p.vscalars.grid, p.vscalars.block, s, d.n_mul, c.uniform->n_cterms, d.n_cst, p.zstride, c.uniform->c_q,
                   c.uniform->c_cst, bd.cst, bd.zpow, bd.yipow, bd.wl, bd.wr, bd.wo, b.vchal, bd.misc, bd.a, b.vs, p.agg_flag);
        return BBP_OK;
    }

    // G = 0: one MSM per proof, then the verdicts
    int32_t tail_plain() const {
        int32_t rc;
        if (!(ko & 1) &&
            (rc = msm_launch(ctx, p.B, VERIFY_MSM_TERMS, (const u32*)b.vs, c.idx_ver, b.fixed, s, 1, bbp_ctx::VERIFY_SLOT + lane, nullptr, nullptr, true)))
            return rc;
        if (!(ko & 2) && (rc = join_varbase())) return rc;  // (a knocked-out variable-base part never forked)
        LAUNCH(ctx, TAG_VARBASE, k_vfinal, p.per_row.grid, p.per_row.block, s, p.B, p.vb.Q, b.fixed, b.var, status_dev);
        return BBP_OK;
    }
    // G > 0: one weighted MSM per group; the group verdicts, the per-proof sums and the weighted scalars stay in the lane for the fallback
    int32_t tail_groups() const {
        const u32 B = p.B, G = p.G, ng = p.ng;
        int32_t rc;
        L.agg_gstatus = b.gstatus, L.agg_varsum = b.varsum, L.agg_vs = b.vs;
        if ((rc = join_varbase())) return rc;
        LAUNCH(ctx, TAG_VERIFY_SCALARS, k_group_sum, dim3(p.group_sum.grid, ng), p.group_sum.block, s, B, G, (const sc*)b.vs, status_dev, b.vsg);
        if ((rc = msm_launch(ctx, ng, VERIFY_MSM_TERMS, (const u32*)b.vsg, c.idx_ver, b.fixedg, s, 1, bbp_ctx::VERIFY_SLOT + lane, nullptr, nullptr, true))) return rc;
        LAUNCH(ctx, TAG_VARBASE, k_var_sum, p.per_row.grid, p.per_row.block, s, B, p.vb.Q, b.var, status_dev, b.varsum);
        LAUNCH(ctx, TAG_VARBASE, k_group_final, p.group_final.grid, p.group_final.block, s, B, G, ng, b.fixedg, b.varsum, b.gstatus);
        return BBP_OK;
    }
};

// The circuit side and the plan of one call.  The round table's size is judged first: it needs no circuit.
static int32_t verify_prepare(bbp_ctx* ctx, const VerifyRows& v, u32 G, VerifyCircuit& c, VerifyPlan& p) {
    if (round_table_too_large(v)) {
        ctx->err = "round table too large";
        return BBP_ERR_BAD_ARG;
    }
    if (int32_t rc = verify_circuit(ctx, v, c)) return rc;
    ctx->vknobs.adopt_process();  // BBP_VARBASE_V1, BBP_V_FENCE: read by the first verify call of the process
    p = plan_verify(v, c.d, G, ctx->vknobs, ctx->knobs.tr_wave_below);
    return BBP_OK;
}

// One pass over the rows, plain (p.G = 0) or in groups.  The steps: reserve, host arrays, front end, variable-base fork, generator
// scalars, the plain or the aggregated tail (verify_plan.h; DESIGN.md "The plan of a verify call").
static int32_t verify_pass(bbp_ctx* ctx, const VerifyRows& v, const VerifyCircuit& c, const VerifyPlan& p, const u8* in_dev, const u8* ent_dev,
                           int32_t* status_dev, hipStream_t s) {
    const int lane = vlane_of(ctx, s);
    bbp_ctx::VLane& L = ctx->vl[lane];
    int32_t rc;
    BatchDev bd;
    StreamGuard guard(ctx, s, 1 + lane);  // this verifier lane: own batch buffer, own misc scratch, own MSM scratch slot
    if ((rc = guard.enter())) return rc;
    // the verifier has a batch buffer of its own (PROVE_BUFS + lane) and runs entirely on the caller's stream: sharing buffer 0 with the
    // prover made every second prove call's opening stage wait for the verification in between (98 ms per prove + verify pair
    // instead of 77)
    if ((rc = batch_reserve(ctx, v.B, c.d, bd, bbp_ctx::PROVE_BUFS + lane))) return rc;
    if ((rc = dev_reserve(ctx, L.misc, p.misc.bytes)) || (p.G && (rc = dev_reserve(ctx, L.agg, p.agg.bytes)))) return rc;
    const VerifyBufs b(p, L.misc.p, L.agg.p);
    const int ko = ctx->vknobs.knocked_out();  // knock-out mask of the experiment builds (verify_plan.h); the constant 0 in the product
    // Not beside the MSM when prove calls are interleaved with the verifications: that stream is the prover's second slice, and queueing
    // behind this call's fork point delays the next batch's slice (measured 67.7 vs 66.3 ms per prove + verify pair).
    const bool overlap = lane == 0 && ctx->vknobs.overlap && ctx->prove_state.calls == ctx->seq_at_last_verify && !(ko & 2);
    ctx->seq_at_last_verify = ctx->prove_state.calls;
    const VerifyCall k{ctx, L, lane, s, v, p, c, bd, b, in_dev, ent_dev, status_dev, ko, overlap};
    if ((rc = k.stage_rows()) || (rc = k.front()) || (rc = k.fork_varbase()) || (rc = k.scalars()) || (rc = p.G ? k.tail_groups() : k.tail_plain())) return rc;
    ctx->last_par = bbp_ctx::PROVE_BUFS + lane;
    return BBP_OK;
}

// v: what the rows at in_dev are (verify_rows.h).  A mixed front end runs with the strides of the largest N, the launches the same in
// number; a rounds call takes seed and bid list from v.rounds (device memory) -- one round behind k_vparse_round, several behind
// k_vparse_rounds_mx with every row's N taken from its round.
int32_t verify_batch_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s) {
    VerifyCircuit c;
    VerifyPlan p;
    const int32_t rc = verify_prepare(ctx, v, G, c, p);
    return rc ? rc : verify_pass(ctx, v, c, p, in_dev, ent_dev, status_dev, s);
}

// Aggregated verification with exact per-proof statuses: groups of G proofs are checked with one weighted MSM each; the members
// of every group that fails then get an MSM of their own over the (weighted) scalars the group pass left in memory -- no second
// parse / transcript / scalar pass.  Entirely stream-ordered: which groups failed is decided on the device (k_compact_failing),
// and the fallback kernels are launched for up to B proofs and size themselves from the device counter.  *n_fallback
// (optional) receives the number of proofs that were checked individually -- asking for it synchronises `s`.
int32_t verify_batch_agg_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s,
                             u32* n_fallback, u32* total_out_dev) {
    if (n_fallback) *n_fallback = 0;
    if (v.rec_ver) {  // aggregation: compact records only (the host path runs such a call plain)
        ctx->err = "aggregated verification takes compact records only";
        return BBP_ERR_BAD_ARG;
    }
    if (G <= 1) return verify_batch_dev(ctx, v, 0, in_dev, ent_dev, status_dev, s);
    const u32 B = v.B;
    int32_t rc;
    const int lane = vlane_of(ctx, s);
    bbp_ctx::VLane& L = ctx->vl[lane];
    if (!L.agg_count) {
        // zeroed ON `s`, the stream every consumer of the counters runs on (k_compact_failing, the device-sized MSM launches,
        // k_fallback_final): a hipMemset on the null stream has no ordering with a non-blocking stream, and a memset landing after
        // k_compact_failing had written counters[0] would skip the per-proof pass -- bad proofs inside failing groups keeping status OK
        BBP_HIP_TRY(ctx, hipMalloc(&L.agg_count, 2 * sizeof(u32)));
        BBP_HIP_TRY(ctx, hipMemsetAsync(L.agg_count, 0, 2 * sizeof(u32), s));
    }
    // the fallback may need one MSM per proof: have that scratch in place BEFORE anything of this call is enqueued (growing a
    // buffer frees it, and the group pass -- same scratch slot, same stream -- would still be using it)
    if ((rc = dev_reserve(ctx, ctx->slice_sorted[bbp_ctx::VERIFY_SLOT + lane], msm_scratch_bytes(B, VERIFY_MSM_TERMS)))) return rc;
    VerifyCircuit c;
    VerifyPlan p;
    if ((rc = verify_prepare(ctx, v, G, c, p)) || (rc = dev_reserve(ctx, L.agg_io, p.agg_io.bytes))) return rc;
    if ((rc = verify_pass(ctx, v, c, p, in_dev, ent_dev, status_dev, s))) return rc;
    u8* base = static_cast<u8*>(L.agg_io.p);
    u32* idx_dev = (u32*)(base + p.agg_io.idx.off);
    ge* fixed = (ge*)(base + p.agg_io.fixed.off);
    StreamGuard guard(ctx, s, 1 + lane);
    if ((rc = guard.enter())) return rc;
    LAUNCH(ctx, TAG_VERIFY_SCALARS, k_compact_failing, p.compact.grid, p.compact.block, s, B, G, p.ng, (const int32_t*)L.agg_gstatus,
           (const int32_t*)status_dev, idx_dev, L.agg_count);
    if ((rc = msm_launch(ctx, B, VERIFY_MSM_TERMS, (const u32*)L.agg_vs, c.idx_ver, fixed, s, 1, bbp_ctx::VERIFY_SLOT + lane, idx_dev, L.agg_count, true)))
        return rc;
    LAUNCH(ctx, TAG_VARBASE, k_fallback_final, p.per_row.grid, p.per_row.block, s, (const u32*)L.agg_count, (const u32*)idx_dev, (const ge*)fixed,
           (const ge*)L.agg_varsum, status_dev, total_out_dev);
    if (n_fallback) {
        BBP_HIP_TRY(ctx, hipMemcpyAsync(n_fallback, L.agg_count, sizeof(u32), hipMemcpyDeviceToHost, s));
        BBP_HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return BBP_OK;
}

// bbp_debug_varbase (include/bbp.h): the shipped variable-base kernels on caller-made rows, through varbase_launch on lane 0's
// stream.  The rows are packed into misc / vchal / wv / vpts at the slots the front end fills (MS_X, MS_R, MS_U, MS_RHO; VC_U, VC_UI;
// point slot k of row p at p * np + k); every buffer is the call's own, sized from the screened counts, and freed on every path.
// Digit words and status start out zero: a slot no kernel writes reads back as eight zero words.
namespace {
struct DebugScratch {
    std::vector<void*> ptrs;
    ~DebugScratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
};
}  // namespace

int32_t debug_varbase(bbp_ctx* ctx, u32 form, u32 B, u32 Q, u32 agg, const u32* ns, const u8* vers, const u8* pts, const u8* scal, const u8* wv,
                      const u8* uj, u8* sums_out, u32* digits_out, int32_t* status_out) {
    auto bad = [&](const char* why) {
        ctx->err = std::string("bbp_debug_varbase: ") + why;
        return (int32_t)BBP_ERR_BAD_ARG;
    };
    if (form > BBP_VARBASE_MX_PREP_SUM) return bad("form is 0..3");
    const bool mixed = form >= BBP_VARBASE_MX_LANES, vb2 = form == BBP_VARBASE_PREP_SUM || form == BBP_VARBASE_MX_PREP_SUM;
    if (B < 1 || B > 1024) return bad("B is 1..1024");
    if (vb2) Q = 1;
    if (Q < 1 || Q > 1024) return bad("Q is 1..1024");
    if (!ns || !vers || !pts || !scal || !wv || !uj || !sums_out || !digits_out || !status_out) return bad("null argument");
    u32 n_max = 0, any_two = 0;
    size_t n_wv = 0;  // wv scalars over all rows
    for (u32 p = 0; p < B; p++) {
        if (ns[p] < 1 || ns[p] > BBP_MAX_ITEMS) return bad("N is 1..202");
        if (vers[p] > 1) return bad("a record version is 0 or 1");
        if (!mixed && (ns[p] != ns[0] || vers[p] != vers[0])) return bad("the uniform forms take one N and one version");
        n_max = std::max(n_max, ns[p]);
        any_two |= vers[p];
        n_wv += 4 + ns[p];
    }
    auto canonical = [](const u8* b, size_t count) {
        for (size_t i = 0; i < count; i++) {
            u32 w[8];
            memcpy(w, b + 32 * i, 32);
            if (!sc_is_canonical(w)) return false;
        }
        return true;
    };
    if (!canonical(scal, 4 * (size_t)B) || !canonical(wv, n_wv) || !canonical(uj, 22 * (size_t)B)) return bad("a scalar is not canonical");
    // strides: the call's largest row (a uniform call: its one N), as verify_batch_dev takes them from the largest circuit
    const VarbaseGeom g = varbase_geom(B, 4 + n_max, any_two != 0, vb2, Q);
    const u32 m = g.m, np = g.np, nq = g.Q;
    std::vector<u8> h_vpts((size_t)B * np * 32, 0), h_misc((size_t)B * MS_COUNT * 32, 0), h_vchal((size_t)B * VC_COUNT * 32, 0), h_wv((size_t)B * m * 32, 0);
    std::vector<VRow> h_rows(B);
    {
        const u8 *pp = pts, *pw = wv;
        u64 off = 0;
        for (u32 p = 0; p < B; p++) {
            const u32 mp = 4 + ns[p], npp = 6 + mp + 5 + 22;
            memcpy(&h_vpts[(size_t)p * np * 32], pp, (size_t)npp * 32);
            memcpy(&h_wv[(size_t)p * m * 32], pw, (size_t)mp * 32);
            pp += (size_t)npp * 32, pw += (size_t)mp * 32;
            u8* ms = &h_misc[(size_t)p * MS_COUNT * 32];
            const int slot[4] = {MS_X, MS_R, MS_U, MS_RHO};
            for (int i = 0; i < 4; i++) memcpy(ms + 32 * slot[i], scal + 32 * (4 * (size_t)p + i), 32);
            u8* vc = &h_vchal[(size_t)p * VC_COUNT * 32];
            memcpy(vc + 32 * VC_U, uj + 32 * 22 * (size_t)p, 32 * 11);
            memcpy(vc + 32 * VC_UI, uj + 32 * (22 * (size_t)p + 11), 32 * 11);
            h_rows[p] = VRow{off, ns[p], (uint16_t)mp, (uint16_t)vers[p]};
            off += vrow_bytes(ns[p], vers[p]);
        }
    }
    DebugScratch scratch;
    auto dev = [&](void** out, const void* host, size_t bytes) -> int32_t {  // zeroed, then the host image when there is one
        BBP_HIP_TRY(ctx, hipMalloc(out, bytes));
        scratch.ptrs.push_back(*out);
        BBP_HIP_TRY(ctx, hipMemset(*out, 0, bytes));
        if (host) BBP_HIP_TRY(ctx, hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice));
        return BBP_OK;
    };
    void *d_vpts, *d_misc, *d_vchal, *d_wv, *d_rows, *d_tab, *d_sp, *d_var, *d_status, *d_enc;
    int32_t rc;
    if ((rc = dev(&d_vpts, h_vpts.data(), h_vpts.size())) || (rc = dev(&d_misc, h_misc.data(), h_misc.size())) ||
        (rc = dev(&d_vchal, h_vchal.data(), h_vchal.size())) || (rc = dev(&d_wv, h_wv.data(), h_wv.size())) ||
        (rc = dev(&d_rows, h_rows.data(), (size_t)B * sizeof(VRow))) || (rc = dev(&d_tab, nullptr, (size_t)B * np * 8 * sizeof(ge))) ||
        (rc = dev(&d_sp, nullptr, (size_t)B * np * 32)) || (rc = dev(&d_var, nullptr, (size_t)B * nq * sizeof(ge))) ||
        (rc = dev(&d_status, nullptr, (size_t)B * 4)) || (rc = dev(&d_enc, nullptr, (size_t)B * nq * 32)))
        return rc;
    // the fills above went to the null stream, which a non-blocking stream does not wait for: they are done before anything is launched
    BBP_HIP_TRY(ctx, hipDeviceSynchronize());
    hipStream_t s = ctx->vl[0].stream;
    {
        StreamGuard guard(ctx, s, 1);
        if ((rc = guard.enter())) return rc;
        const VarbaseLaunch vb{mixed, g, (const VRow*)d_rows, (const u32*)d_vpts, (const sc*)d_vchal,
                               (const sc*)d_misc, (const sc*)d_wv, (ge*)d_tab, (ge*)d_var, (u32*)d_sp, (int32_t*)d_status};
        if ((rc = varbase_launch(ctx, vb, s, agg ? 1u : 0u))) return rc;
        if ((rc = encode_launch(ctx, B * nq, (const ge*)d_var, (uint8_t*)d_enc, s))) return rc;
        BBP_HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    std::vector<u32> h_sp((size_t)B * np * 8);
    BBP_HIP_TRY(ctx, hipMemcpy(h_sp.data(), d_sp, h_sp.size() * 4, hipMemcpyDeviceToHost));
    BBP_HIP_TRY(ctx, hipMemcpy(sums_out, d_enc, (size_t)B * nq * 32, hipMemcpyDeviceToHost));
    BBP_HIP_TRY(ctx, hipMemcpy(status_out, d_status, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (u32 p = 0; p < B; p++) {
        const u32 npp = 6 + (4 + ns[p]) + 5 + 22;
        memcpy(digits_out, &h_sp[(size_t)p * np * 8], (size_t)npp * 32);
        digits_out += (size_t)npp * 8;
    }
    return BBP_OK;
}

// The table reduction of ONE round for the prove side (capi_prove.hip, bbp_prove_round*): k_round_consts as the verifier launches it,
// R = 1.  roff_dev: the two scalar offsets {0, 1 + N} in device memory; rblk: 1 + N scalars; rflag: one flag.
int32_t round_consts_launch(bbp_ctx* ctx, u32 N, const u8* round_dev, const u32* roff_dev, sc* rblk, int32_t* rflag, hipStream_t s) {
    LAUNCH(ctx, TAG_TRANSCRIPT, k_round_consts, cdiv(1 + N, 64), 64, s, 1u, roff_dev, round_dev, rblk, rflag);
    return BBP_OK;
}

}  // namespace bbp
