// Test-only shim: compiles the PRODUCT's limb arithmetic headers for the host CPU so the not-gpu test
// tier can compare them with the oracle.  Nothing in the shipped library calls this.
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/batch_layout.h"
#include "../dusk_blindbidproof_amd/csrc/keccak.h"
#include "../dusk_blindbidproof_amd/csrc/keccak_wave.h"
#include "../dusk_blindbidproof_amd/csrc/msm_index.h"
#include "../dusk_blindbidproof_amd/csrc/msm_plan.h"
#include "../dusk_blindbidproof_amd/csrc/point.h"
#include "../dusk_blindbidproof_amd/csrc/prove_io.h"
#include "../dusk_blindbidproof_amd/csrc/prove_plan.h"
#include "../dusk_blindbidproof_amd/csrc/scalar.h"
#include "../dusk_blindbidproof_amd/csrc/scalarmul.h"
#include "../dusk_blindbidproof_amd/csrc/verify_plan.h"
#include "../dusk_blindbidproof_amd/csrc/verify_rows.h"
#include "../dusk_blindbidproof_amd/csrc/witness.h"

using namespace bbp;

static void ld(u32* w, const uint8_t* b, int nwords) { memcpy(w, b, 4 * nwords); }

extern "C" {

// op: 0 add, 1 sub, 2 mul, 3 sq, 4 invert, 5 canon(a), 6 neg, 7 pow22523, 8 mul_small(a, b[0]), 9 sq2, 10 growth, 11 / 12 threaded-carry multiply
void hc_fe_op(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
    u32 wa[8], wb[8];
    ld(wa, a32, 8);
    ld(wb, b32, 8);
    fe a = fe_fromwords(wa), b = fe_fromwords(wb), r;  // bit 255 ignored
    switch (op) {
        case 0: r = fe_add(a, b); break;
        case 1: r = fe_sub(a, b); break;
        case 2: r = fe_mul(a, b); break;
        case 3: r = fe_sq(a); break;
        case 4: r = fe_invert(a); break;
        case 5: r = a; break;
        case 6: r = fe_neg(a); break;
        case 7: r = fe_pow22523(a); break;
        case 8: r = fe_mul_small(a, wb[0] & 0x3ffffffu); break;
        case 9: r = fe_sq2(a); break;
        case 10: {  // worst-case operand growth the point formulas produce: three-term sums into a multiply, twice
            fe m1 = fe_mul(a, b), m2 = fe_sq(b), m3 = fe_mul(b, fe_sq(a));
            fe s = fe_add(fe_add(m1, m1), m2), d = fe_sub(fe_sub(m3, m2), m1);
            r = fe_mul(s, d);
            r = fe_sq(fe_sub(fe_add(r, m1), m3));
            break;
        }
        case 11: r = fe_mul_chain_portable(a, b); break;  // the device path's threaded carry pass (field.h), column sums in plain C
        case 12: {  // the same on maximally loaded operands (three-term sums, as the point formulas feed them), limb bounds checked
            fe m1 = fe_mul_chain_portable(a, b), m2 = fe_mul_chain_portable(b, b), m3 = fe_mul_chain_portable(b, fe_mul_chain_portable(a, a));
            fe s = fe_add(fe_add(m1, m1), m2), d = fe_sub(fe_sub(m3, m2), m1);
            r = fe_mul_chain_portable(s, d);
            for (int i = 0; i < 10; i++) {  // carried: |h_even| <= 2^25, |h_odd| <= 2^24 (+ the one small carry into limb 1)
                const i32 bound = (i & 1) ? (1 << 24) : (1 << 25);
                const i32 v = r.v[i] < 0 ? -r.v[i] : r.v[i];
                if (v > bound + (i == 1 ? (1 << 17) : 0)) r = fe_zero();  // reported as a wrong value
            }
            fe t = fe_sub(fe_add(r, m1), m3);
            r = fe_mul_chain_portable(t, t);
            break;
        }
        default: r = fe_zero(); break;
    }
    fe_tobytes(out32, r);
}

// raw signed limbs in, raw limbs and canonical bytes out; op codes as device_check.hip dc_fe_limbs: 0 mul(a, b), 1 sq(a), 2 sq2(a),
// 3 mul_small(a, b[0]), 4 mul(a + b, a - b), 5 towords(a), 6 iszero(a), 7 isneg(a), 8 eq(a, b) (ops 5..8: bytes of a, predicate in limb 0)
void hc_fe_limbs(int op, const int32_t* a10, const int32_t* b10, int32_t* out10, uint8_t* out32) {
    fe a, b, r = fe_zero();
    for (int i = 0; i < 10; i++) {
        a.v[i] = a10[i];
        b.v[i] = b10[i];
    }
    switch (op) {
        case 0: r = fe_mul(a, b); break;
        case 1: r = fe_sq(a); break;
        case 2: r = fe_sq2(a); break;
        case 3: r = fe_mul_small(a, (u32)b.v[0] & 0x3ffffffu); break;
        case 4: r = fe_mul(fe_add(a, b), fe_sub(a, b)); break;
        case 6: r.v[0] = fe_iszero(a) ? 1 : 0; break;
        case 7: r.v[0] = fe_isneg(a) ? 1 : 0; break;
        case 8: r.v[0] = fe_eq(a, b) ? 1 : 0; break;
        default: break;
    }
    for (int i = 0; i < 10; i++) out10[i] = r.v[i];
    fe_tobytes(out32, op >= 5 ? a : r);
}

// NAF recoding used by the MSM kernels: writes (position, signed digit) pairs, returns the count (width 12 or 9)
int hc_sc_naf(int width, const uint8_t* a32, int32_t* pos_out, int32_t* digit_out) {
    u32 w[8];
    ld(w, a32, 8);
    int n = 0;
    auto emit = [&](u32 pos, u32 mag, u32 neg) {
        pos_out[n] = (int32_t)pos;
        digit_out[n] = neg ? -(int32_t)mag : (int32_t)mag;
        n++;
    };
    if (width == 12) sc_for_each_naf_digit<12>(w, emit);
    else sc_for_each_naf_digit<9>(w, emit);
    return n;
}

// op: 0 add, 1 sub, 2 mul, 3 invert, 4 from_wide(a64), 5 from_bits(a32), 6 neg
void hc_sc_op(int op, const uint8_t* a, const uint8_t* b32, uint8_t* out32) {
    sc x, y, r;
    u32 w[16];
    if (op == 4) {
        ld(w, a, 16);
        r = sc_from_wide(w);
    } else if (op == 5) {
        ld(w, a, 8);
        r = sc_from_bits(w);
    } else {
        ld(x.v, a, 8);
        ld(y.v, b32, 8);
        switch (op) {
            case 0: r = sc_add(x, y); break;
            case 1: r = sc_sub(x, y); break;
            case 2: r = sc_mul(x, y); break;
            case 3: r = sc_invert(x); break;
            case 7: r = sc_invert_fermat(x); break;
            default: r = sc_neg(x); break;
        }
    }
    sc_tobytes(out32, r);
}

int hc_sc_is_canonical(const uint8_t* a32) {
    u32 w[8];
    ld(w, a32, 8);
    return sc_is_canonical(w) ? 1 : 0;
}

// decode -> (op) -> encode.  op: 0 identity map (round trip), 1 double, 2 add(a,b), 3 sub(a,b),
// 4 madd(a, niels(b)), 5 msub(a, niels(b)).  Returns 0 if a decode failed.
int hc_ge_op(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
    u32 w[8];
    ge a, b, r;
    ld(w, a32, 8);
    if (!ge_decode_words(a, w)) return 0;
    ld(w, b32, 8);
    if (op >= 2 && !ge_decode_words(b, w)) return 0;
    switch (op) {
        case 0: r = a; break;
        case 1: r = ge_dbl(a); break;
        case 2: r = ge_add(a, b); break;
        case 3: r = ge_sub(a, b); break;
        case 4: r = ge_madd(a, ge_to_niels(b, fe_invert(b.Z))); break;
        default: r = ge_msub(a, ge_to_niels(b, fe_invert(b.Z))); break;
    }
    ge_encode(out32, r);
    return 1;
}

void hc_from_uniform(const uint8_t* in64, uint8_t* out32) {
    u32 w[16];
    ld(w, in64, 16);
    ge_encode(out32, ge_from_uniform_words(w));
}

void hc_basepoint(uint8_t* out32) { ge_encode(out32, ge_basepoint()); }

// scalar * point by double-and-add (test helper)
int hc_scalarmult(const uint8_t* s32, const uint8_t* p32, uint8_t* out32) {
    u32 w[8], s[8];
    ge p;
    ld(w, p32, 8);
    if (!ge_decode_words(p, w)) return 0;
    ld(s, s32, 8);
    ge acc = ge_identity();
    for (int i = 255; i >= 0; i--) {
        acc = ge_dbl(acc);
        if ((s[i >> 5] >> (i & 31)) & 1u) acc = ge_add(acc, p);
    }
    ge_encode(out32, acc);
    return 1;
}

// The prover's gates a_L | a_R | a_O of one proof on the host, from the product's own code (csrc/witness.h): the compiled gadget
// program interpreted (circuit.h compile + witness_gates_interpret) and the gadget wiring written out (witness_gates_native).
// in_raw: d, k, y, y_inv, q, z_img, seed (7 x 32 B) || N items (32 B each) || toggle (u64), as Proof::prove's inputs reach the engine;
// mimc: the 90 round constants (32 B each).  out_*: 3 * n_mul scalars each (a_L, then a_R, then a_O).  Returns n_mul, or -1 / -2 when
// the two forms do not count the same multipliers / the buffers are too small.
int hc_witness_gates(uint32_t n_items, const uint8_t* in_raw, const uint8_t* mimc, uint8_t* out_interp, uint8_t* out_native, uint32_t cap_mul) {
    const circuit::Compiled c = circuit::compile(n_items);
    if (c.n_mul > cap_mul) return -2;
    std::vector<sc> cst(circuit::cst_count(n_items)), v(4 + n_items);
    u32 w[8];
    sc s7[7];
    for (int i = 0; i < 7; i++) {
        ld(w, in_raw + 32 * i, 8);
        s7[i] = sc_reduce256(w);
    }
    cst[circuit::CST_ONE] = sc_one();
    cst[circuit::CST_ZERO] = sc_zero();
    for (int i = 0; i < circuit::MIMC_ROUNDS; i++) {
        ld(w, mimc + 32 * i, 8);
        cst[circuit::CST_MIMC0 + i] = sc_reduce256(w);
    }
    cst[circuit::CST_SEED] = s7[6];
    cst[circuit::CST_ZIMG] = s7[5];
    cst[circuit::CST_Q] = s7[4];
    for (uint32_t i = 0; i < n_items; i++) {
        ld(w, in_raw + 224 + 32 * i, 8);
        cst[circuit::CST_ITEM0 + i] = sc_from_bits(w);  // bid.rs:27
    }
    uint64_t toggle;
    memcpy(&toggle, in_raw + 224 + 32 * (size_t)n_items, 8);
    v[0] = s7[0];
    v[1] = s7[1];
    v[2] = s7[2];
    v[3] = s7[3];
    for (uint32_t i = 0; i < n_items; i++) v[4 + i] = (uint64_t)i == toggle ? sc_one() : sc_zero();
    std::vector<sc> a(3 * (size_t)c.n_mul), b(3 * (size_t)c.n_mul);
    witness_gates_interpret(c.n_mul, c.w_terms.data(), c.w_loff.data(), c.w_roff.data(), cst.data(), v.data(), a.data(), a.data() + c.n_mul,
                            a.data() + 2 * (size_t)c.n_mul);
    const u32 wrote = witness_gates_native(n_items, cst.data(), v.data(), b.data(), b.data() + c.n_mul, b.data() + 2 * (size_t)c.n_mul);
    if (wrote != c.n_mul) return -1;
    for (size_t i = 0; i < a.size(); i++) {
        memcpy(out_interp + 32 * i, a[i].v, 32);
        memcpy(out_native + 32 * i, b[i].v, 32);
    }
    return (int)c.n_mul;
}

// The row-layout descriptor of the verify calls (csrc/verify_rows.h), built by its own constructors -- kind 0: uniform(B, N, rec_ver),
// 1: mixed(B, ns, vers), 2: of_rounds(B, R, round_ns, table, round_of) -- and cut to rows [lo, hi) when lo <= hi <= B (lo > hi: the
// call itself).  out_n / out_ver: one entry per row; out_off: one more (offsets()).  info: 0 B, 1 rec_ver, 2 vers kept, 3 mixed front
// end, 4 front_n (uniform front end only), 5 R, 6 the table pointer, 7 table_bytes, 8 round_of kept, 9 round_of's distance from the
// caller's array in entries, 10 first_n (B > 0 only).
void hc_verify_rows(int kind, uint32_t B, uint32_t N, uint32_t rec_ver, const uint32_t* ns, const uint8_t* vers, uint32_t R, const uint32_t* round_ns,
                    const uint8_t* table, const uint32_t* round_of, uint32_t lo, uint32_t hi, uint32_t* out_n, uint32_t* out_ver, uint64_t* out_off,
                    uint64_t* info) {
    VerifyRows v = kind == 0 ? VerifyRows::uniform(B, N, rec_ver) : kind == 1 ? VerifyRows::mixed(B, ns, vers) : VerifyRows::of_rounds(B, R, round_ns, table, round_of);
    if (lo <= hi) v = v.slice(lo, hi);
    const std::vector<size_t> off = v.offsets();
    for (uint32_t i = 0; i < v.B; i++) {
        out_n[i] = v.n_of(i);
        out_ver[i] = v.ver_of(i);
        if (off[i + 1] - off[i] != v.row_bytes(i)) out_n[i] = 0xffffffffu;  // reported as a wrong N
    }
    for (size_t i = 0; i < off.size(); i++) out_off[i] = off[i];
    info[0] = v.B;
    info[1] = v.rec_ver;
    info[2] = v.vers != nullptr;
    info[3] = v.mixed_front();
    info[4] = v.mixed_front() ? 0 : v.front_n();
    info[5] = v.R;
    info[6] = (uint64_t)(uintptr_t)v.rounds;
    info[7] = v.table_bytes();
    info[8] = v.round_of != nullptr;
    info[9] = v.round_of ? (uint64_t)(v.round_of - round_of) : 0;
    info[10] = v.B ? v.first_n() : 0;
}

// The row sizes of the prove side and the staging layout of one host-pointer prove call with its two ring siblings
// (csrc/prove_io.h).  sizes: 0 prove_in_bytes, 1 prove_in_words, 2 PROVE_IN_Q, 3 PROVE_IN_LIST, 4 PROVE_IN_LIST_WORD, 5 prove_in_toggle,
// 6 prove_in_toggle_word, 7 entropy_row_bytes, 8 verify_tail_bytes, 9 verify_tail_words, 10 VERIFY_TAIL_LIST_WORD, 11 ROUND_BID_BYTES,
// 12 round_table_bytes.  lay: the ProveStaging of (B, N, round, check, dev_draw) -- 0 in_stride, 1 ent_stride, 2 rec, 3 res_stride,
// 4 in_first_bytes, 5 in_tab, 6 in_tab_bytes, 7 in_scratch, 8 in_rows, 9 in_upload, 10 in_cap, 11 rs.end, 12 rs.rb, 13 ent_drawn,
// 14 ent_up_off, 15 ent_up_bytes, 16 ent_cap, 17 ent_check(first), 18 out_recs, 19 out_info, 20 out_status, 21 out_mask, 22 out_fail_n,
// 23 out_fail_idx, 24 out_tog, 25 out_pass_st, 26 out_fetch, 27 out_cap, 28 chk_vstatus, 29 chk_bytes, 30 h_in_bytes, 31 h_out_bytes.
// rings: CheckRing(B, N) -- 0 vstatus, 1 scratch_bytes, 2 mask, 3 bytes; RoundRing(B, N, false).bytes at 4; RoundRing(B, N, true) --
// 5 rows, 6 recs, 7 bytes.
void hc_prove_staging(uint32_t B, uint32_t N, int round, int check, int dev_draw, uint32_t first, uint64_t* sizes, uint64_t* lay, uint64_t* rings) {
    const uint64_t sz[13] = {prove_in_bytes(N), prove_in_words(N), PROVE_IN_Q, PROVE_IN_LIST, PROVE_IN_LIST_WORD, prove_in_toggle(N), prove_in_toggle_word(N),
                             entropy_row_bytes(N), verify_tail_bytes(N), verify_tail_words(N), VERIFY_TAIL_LIST_WORD, ROUND_BID_BYTES, round_table_bytes(N)};
    memcpy(sizes, sz, sizeof sz);
    const ProveStaging L(B, N, round != 0, check != 0, dev_draw != 0);
    const uint64_t lv[32] = {L.in_stride, L.ent_stride, L.rec, L.res_stride, L.in_first_bytes, L.in_tab, L.in_tab_bytes, L.in_scratch, L.in_rows, L.in_upload, L.in_cap,
                             L.rs.end, L.rs.rb, L.ent_drawn, L.ent_up_off, L.ent_up_bytes, L.ent_cap, L.ent_check(first), L.out_recs, L.out_info, L.out_status,
                             L.out_mask, L.out_fail_n, L.out_fail_idx, L.out_tog, L.out_pass_st, L.out_fetch, L.out_cap, L.chk_vstatus, L.chk_bytes, L.h_in_bytes,
                             L.h_out_bytes};
    memcpy(lay, lv, sizeof lv);
    const CheckRing c(B, N);
    const RoundRing r0(B, N, false), r1(B, N, true);
    const uint64_t rv[8] = {c.vstatus, c.scratch_bytes, c.mask, c.bytes, r0.bytes, r1.rows, r1.recs, r1.bytes};
    memcpy(rings, rv, sizeof rv);
}

// The plan of one prove call (csrc/prove_plan.h).  knobs: n_knobs (environment name, text) pairs applied over the defaults through
// ProveKnobs::set, clamps included; -1: a name is no prove knob.  state (in and out): deep_mode, deep_idle_seen, force_deep, last_sliced,
// calls.  busy: what sliced_busy answers.  out: 0 call, 1 deep, 2 behind_sliced, 3 dual, 4 open_stream, 5 par, 6 coop, 7 chain, 8 prefix_form,
// 9 serial_blk, 10 cblk, 11 cblk_wave, 12 rotate, 13 heavy_stream, 14 slices, 15 times sliced_busy was asked, 16..20 the slice bounds
// (slices + 1 of them), then plan_heavy(knobs, B): 21 tw, 22 tgrid, 23 wide_ipa, 24 split_T, 25 tail_from, 26 stagger_after.
// trace: trace_line(call, B, inflight).
int hc_prove_plan(const char* const* knobs, int n_knobs, int32_t* state, uint32_t B, int inflight, int busy, int64_t* out, char* trace, size_t trace_cap) {
    ProveKnobs k;
    for (int i = 0; i < n_knobs; i++)
        if (!k.set(knobs[2 * i], knobs[2 * i + 1])) return -1;
    ProveRuleState st;
    st.deep_mode = state[0], st.deep_idle_seen = state[1], st.force_deep = state[2], st.last_sliced = state[3], st.calls = (uint32_t)state[4];
    int asked = 0;
    const ProvePlan p = plan_prove(k, st, B, inflight, [&] { asked++; return busy != 0; });
    state[0] = st.deep_mode, state[1] = st.deep_idle_seen, state[2] = st.force_deep, state[3] = st.last_sliced, state[4] = (int32_t)st.calls;
    const int64_t plan[16] = {p.call, p.deep, p.behind_sliced, p.dual, p.open_stream, p.par, p.coop, p.chain, p.prefix_form, p.serial_blk, p.cblk, p.cblk_wave(),
                              p.rotate, p.heavy_stream, p.slices, asked};
    memcpy(out, plan, sizeof plan);
    for (uint32_t i = 0; i < 5; i++) out[16 + i] = i <= p.slices && p.slices ? (int64_t)p.slice_first(B, i) : -1;
    const HeavyPlan h = plan_heavy(k, B);
    out[21] = h.tw, out[22] = h.tgrid, out[23] = h.wide_ipa, out[24] = h.split_T, out[25] = h.tail_from, out[26] = h.stagger_after;
    snprintf(trace, trace_cap, "%s", p.trace_line(p.call, B, inflight).c_str());
    return 0;
}
// one knob as ProveKnobs::from_env reads it from an environment that holds name=text (the variable is set for the call only)
int hc_prove_knob_from_env(const char* name, const char* text, int which) {
    setenv(name, text, 1);
    const ProveKnobs k = ProveKnobs::from_env();
    unsetenv(name);
    const int v[] = {k.slices, k.rotate_below, k.rotate_deep_max, k.deep_from, k.mixed_from, k.dual_open_below, k.rng_coop, k.rng_coop_below, k.rng_coop_idle_below,
                     k.rng_dpp, k.rng_block, k.serial_block, k.serial_lds, k.tr_wave_below, k.ipa_wide_below, k.commit_split_below, k.witness_native,
                     k.tail_small_below, k.tail_round, k.stagger_mode, k.trace_prove};
    return v[which];
}

// The plan of one MSM launch (csrc/msm_plan.h).  knobs: n_knobs (environment name, text) pairs applied over the defaults through
// MsmKnobs::set, clamps included; -1: a name is no MSM knob.  out: 0 split, 1 n_sub, 2 n_work, 3 geom, 4 sort, 5 sort_cap, 6 fold,
// 7 reduce, 8 K, 9 W, 10 the recoding's width.
int hc_msm_plan(const char* const* knobs, int n_knobs, uint32_t n_msm, uint32_t n_terms, int device_sized, int64_t* out) {
    MsmKnobs k;
    for (int i = 0; i < n_knobs; i++)
        if (!k.set(knobs[2 * i], knobs[2 * i + 1])) return -1;
    const MsmPlan p = plan_msm(k, n_msm, n_terms, device_sized != 0);
    const int64_t v[11] = {p.split, p.n_sub, p.n_work, p.geom, p.sort, p.sort_cap, p.fold, p.reduce, p.K(), p.W(), p.naf()};
    memcpy(out, v, sizeof v);
    return 0;
}
// one knob as MsmKnobs::from_env reads it from an environment that holds name=text (the variable is set for the call only; the two
// split knobs are the process's, read once: they show their defaults here)
int hc_msm_knob_from_env(const char* name, const char* text, int which) {
    MsmKnobs::process();
    setenv(name, text, 1);
    const MsmKnobs k = MsmKnobs::from_env();
    unsetenv(name);
    const int v[] = {k.sort_staged, k.fold_half_from, k.msm_small, (int)k.split_below, (int)k.split_target};
    return v[which];
}
// The plan of one verify device call (csrc/verify_plan.h).  knobs: n_knobs (environment name, text) pairs applied over the defaults
// through VerifyKnobs::set, clamps included; -1: a name is no verify knob.  The rows as hc_verify_rows takes them (kind 0 uniform, 1
// mixed, 2 rounds).  dims: n_dims circuits of (m, n_mul, n_cons, n_cst), widened into one VerifyDims as mixed_prepare does.
// geo: 0 front, 1 mixed, 2 rounds, 3 np, 4 npa, 5 Q, 6 vb2, 7 one_phase, 8 vstride, 9 zstride, 10 zchunks, 11 n_tgt, 12 vtw, 13 ng,
// 14 agg_flag, 15 rd_S, 16 rd_nof, 17 rd_too_large, 18..21 the dims, then (grid, block) of fill_mimc, round_consts, vrows, parse,
// transcript, powers_z, powers_yinv, flatten, vscalars, per_row, group_sum, group_final, vb.prep, vb.sum, vb.lanes, compact from 22.
// lay: (offset, bytes) of misc's twelve regions in the order of the struct, misc.bytes; of agg's four, agg.bytes; of agg_io's two,
// agg_io.bytes.  rd_off: R + 1 entries (rounds only).
int hc_verify_plan(const char* const* knobs, int n_knobs, int kind, uint32_t B, uint32_t N, uint32_t rec_ver, const uint32_t* ns, const uint8_t* vers,
                   uint32_t R, const uint32_t* round_ns, const uint32_t* round_of, const uint32_t* dims, int n_dims, uint32_t G, int tr_wave_below,
                   int64_t* geo, uint64_t* lay, uint32_t* rd_off) {
    VerifyKnobs k;
    for (int i = 0; i < n_knobs; i++)
        if (!k.set(knobs[2 * i], knobs[2 * i + 1])) return -1;
    const VerifyRows v = kind == 0 ? VerifyRows::uniform(B, N, rec_ver) : kind == 1 ? VerifyRows::mixed(B, ns, vers) : VerifyRows::of_rounds(B, R, round_ns, nullptr, round_of);
    VerifyDims d;
    for (int i = 0; i < n_dims; i++) d.widen(VerifyDims{dims[4 * i], dims[4 * i + 1], dims[4 * i + 2], dims[4 * i + 3]});
    const VerifyPlan p = plan_verify(v, d, G, k, tr_wave_below);
    const int64_t g[22] = {p.front, p.mixed, p.rounds, p.vb.np, p.vb.npa, p.vb.Q, p.vb.vb2, p.vb.one_phase, p.vstride, p.zstride, p.zchunks, p.n_tgt, p.vtw, p.ng,
                           p.agg_flag, p.rd_S, p.rd_nof, p.rd_too_large, p.d.m, p.d.n_mul, p.d.n_cons, p.d.n_cst};
    memcpy(geo, g, sizeof g);
    const VLaunch ls[16] = {p.fill_mimc, p.round_consts, p.vrows, p.parse, p.transcript, p.powers_z, p.powers_yinv, p.flatten, p.vscalars, p.per_row,
                            p.group_sum, p.group_final, p.vb.prep, p.vb.sum, p.vb.lanes, p.compact};
    for (int i = 0; i < 16; i++) geo[22 + 2 * i] = ls[i].grid, geo[23 + 2 * i] = ls[i].block;
    const VerifyPlan::Misc& m = p.misc;
    const VRegion rs[18] = {m.vpts, m.vchal, m.vs, m.tab, m.var, m.fixed, m.sp, m.rows, m.ns, m.rof, m.rblk, m.rflag,
                            p.agg.vsg, p.agg.fixedg, p.agg.varsum, p.agg.gstatus, p.agg_io.fixed, p.agg_io.idx};
    const size_t totals[3] = {m.bytes, p.agg.bytes, p.agg_io.bytes};
    for (int i = 0, o = 0; i < 18; i++) {
        lay[o++] = rs[i].off, lay[o++] = rs[i].bytes;
        if (i == 11 || i == 15 || i == 17) lay[o++] = totals[i == 11 ? 0 : i == 15 ? 1 : 2];
    }
    for (size_t i = 0; i < p.rd_off.size(); i++) rd_off[i] = p.rd_off[i];
    return 0;
}
// The staging layout of one host-pointer verify call (VerifyStaging).  out: 0 in_bytes, 1 tab_off, 2 tab_bytes, 3 ent_up_bytes,
// 4 ent_drawn, 5 out_bytes, 6 fetch_bytes, 7 group, 8 n_chunks, 9 chunk, 10 row_off[B - 1]; 11, 12: sizeof(ge), sizeof(VRow).
void hc_verify_staging(int kind, uint32_t B, uint32_t N, uint32_t rec_ver, const uint32_t* ns, const uint8_t* vers, uint32_t R, const uint32_t* round_ns,
                       const uint32_t* round_of, uint32_t group, uint32_t ctx_group, int dev_draw, uint32_t host_chunk, uint64_t* out) {
    const VerifyRows v = kind == 0 ? VerifyRows::uniform(B, N, rec_ver) : kind == 1 ? VerifyRows::mixed(B, ns, vers) : VerifyRows::of_rounds(B, R, round_ns, nullptr, round_of);
    const VerifyStaging s(v, group, ctx_group, dev_draw != 0, host_chunk);
    const uint64_t o[13] = {s.in_bytes, s.tab_off, s.tab_bytes, s.ent_up_bytes, s.ent_drawn, s.out_bytes, s.fetch_bytes, s.group, s.n_chunks, s.chunk,
                            B ? s.row_off[B - 1] : 0, sizeof(ge), sizeof(VRow)};
    memcpy(out, o, sizeof o);
}
// one knob as the engine reads it from an environment that holds name=text (the variable is set for the call only): which 0..2 the
// context's (VerifyKnobs::from_env), 3, 4 the process's as adopt_process hands them on (read once, before the variable is set: they
// show their defaults here), 5 the per-call chunk (host_chunk_now)
int hc_verify_knob_from_env(const char* name, const char* text, int which) {
    VerifyKnobs::process();
    setenv(name, text, 1);
    VerifyKnobs k = VerifyKnobs::from_env();
    k.adopt_process();
    const int chunk = (int)VerifyKnobs::host_chunk_now();
    unsetenv(name);
    const int v[] = {k.varbase_lanes, k.overlap, k.group, k.varbase_v1, k.fence, chunk};
    return v[which];
}
// ---- the batch buffer (csrc/batch_layout.h) and the MSM base-index lists (csrc/msm_index.h) --------------------------------------
static const circuit::Compiled& hc_compiled(uint32_t N) {  // compiled once per N
    static std::map<uint32_t, circuit::Compiled> cache;
    auto it = cache.find(N);
    if (it == cache.end()) it = cache.emplace(N, circuit::compile(N)).first;
    return it->second;
}
// the sizes alone: sizeof(sc), sizeof(ge), sizeof(merlin_transcript)
void hc_batch_elem_sizes(uint64_t* out3) { out3[0] = sizeof(sc), out3[1] = sizeof(ge), out3[2] = sizeof(merlin_transcript); }
// (m, n_mul, n_cons, n_cst) of circuit N, as circuit_get fills a CircuitDev
void hc_circuit_dims(uint32_t N, uint32_t* out4) {
    const circuit::Compiled& c = hc_compiled(N);
    out4[0] = c.m, out4[1] = c.n_mul, out4[2] = c.n_cons, out4[3] = circuit::cst_count(N);
}
// The carve of B proofs of dimensions dims (m, n_mul, n_cons, n_cst).  Per array, in list order: its byte offset, its stride in
// elements, its element size; names: the field names, space separated.  Returns the number of arrays; *total: the reservation.
int hc_batch_layout(uint32_t B, const uint32_t* dims, uint64_t* off, uint64_t* stride, uint64_t* elem, uint64_t* total, char* names, size_t names_cap) {
    const BatchDims d{dims[0], dims[1], dims[2], dims[3]};
    const BatchOffsets o = batch_offsets(B, d);
    const BatchStrides s = batch_strides(d);
    int n = 0;
    std::string all;
#define X(name, T, count) off[n] = o.name, stride[n] = s.name, elem[n] = sizeof(T), all += (n ? " " : ""), all += #name, n++;
    BBP_BATCH_ARRAYS(X)
#undef X
    *total = o.bytes;
    snprintf(names, names_cap, "%s", all.c_str());
    return n;
}
// batch_view(batch_carve(base, B, dims), dims, first): every pointer's distance from `base` in bytes (the base is never dereferenced)
int hc_batch_view(uint32_t B, const uint32_t* dims, uint32_t first, uint64_t* delta) {
    const BatchDims d{dims[0], dims[1], dims[2], dims[3]};
    u8* const base = reinterpret_cast<u8*>((uintptr_t)1 << 40);
    const BatchDev v = batch_view(batch_carve(base, batch_offsets(B, d)), d, first);
    int n = 0;
#define X(name, T, count) delta[n++] = (uint64_t)(reinterpret_cast<uintptr_t>(v.name) - reinterpret_cast<uintptr_t>(base));
    BBP_BATCH_ARRAYS(X)
#undef X
    return n;
}
// ProvePlan::slice_first of a call cut into `slices`
uint32_t hc_slice_first(uint32_t B, uint32_t slices, uint32_t i) {
    ProvePlan p;
    p.slices = slices;
    return p.slice_first(B, i);
}
// the encoding and point blocks of one proof: 0 enc_words, 1 enc_V(0), 2 enc_V(m - 1), 3 enc_A, 4 enc_T, 5..15 enc_LR(r = 1..11), 16 pts_count, 17 pts_T
void hc_enc_slots(uint32_t m, uint64_t* out18) {
    out18[0] = enc_words(m), out18[1] = enc_V(0), out18[2] = enc_V(m - 1), out18[3] = enc_A(m), out18[4] = enc_T(m);
    for (uint32_t r = 1; r <= IPA_ROUNDS; r++) out18[4 + r] = enc_LR(m, r);
    out18[16] = pts_count(m), out18[17] = pts_T(m);
}
// the base-index lists of circuit N.  which: 0 idx_ai, 1 idx_s1, 2 idx_ao, 3 idx_ipa, 4 idx_ver.  Returns the length (the first `cap`
// entries are written); *n_ai_terms: index_ai's count (which 0 only)
int hc_index_lists(uint32_t N, int which, uint32_t* out, uint32_t cap, uint32_t* n_ai_terms) {
    const circuit::Compiled& c = hc_compiled(N);
    const std::vector<u32> v = which == 0 ? index_ai(c, n_ai_terms) : which == 1 ? index_s1(c) : which == 2 ? index_ao(c) : which == 3 ? index_ipa(c) : index_ver();
    for (size_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}
// the gadget program of circuit N.  which: 0 w_terms, 1 w_loff, 2 w_roff; as hc_index_lists
int hc_circuit_wires(uint32_t N, int which, uint32_t* out, uint32_t cap) {
    const circuit::Compiled& c = hc_compiled(N);
    const std::vector<u32>& v = which == 0 ? c.w_terms : which == 1 ? c.w_loff : c.w_roff;
    for (size_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

// msm_split over every launch of n_msm = 1..max_msm MSMs of n_terms = 1..max_terms terms under the default knobs: how many
// (n_msm, n_terms) break a rule -- the sub-MSMs cover the terms, none lies wholly past the end, at most MSM_SPLIT_MAX of them, a
// split MSM's sub-MSMs have 128 terms or more; first_bad: the first such pair.  *max_split: the largest split seen.
int hc_msm_split_sweep(uint32_t max_msm, uint32_t max_terms, uint32_t* first_bad, uint32_t* max_split) {
    const MsmKnobs k;
    int bad = 0;
    *max_split = 0;
    for (uint32_t m = 1; m <= max_msm; m++)
        for (uint32_t n = 1; n <= max_terms; n++) {
            const MsmPlan p = plan_msm(k, m, n, false);
            const bool ok = p.split >= 1 && p.split == msm_split(k, m, n) && (uint64_t)p.split * p.n_sub >= n && (uint64_t)(p.split - 1) * p.n_sub < n &&
                            p.split <= 16 && (p.split == 1 || p.n_sub >= 128) && p.n_work == m * p.split;
            if (p.split > *max_split) *max_split = p.split;
            if (!ok && !bad++) first_bad[0] = m, first_bad[1] = n;
        }
    return bad;
}
// entries per bucket (|d| + 1) / 2 of n scalars under the product's recoder (width 12 or 9), and how many of them are negative digits;
// -1: a digit fell outside buckets 1..K
int hc_msm_histogram(int width, uint32_t n, const uint8_t* scalars, uint32_t K, uint32_t* hist, uint32_t* neg_hist) {
    int rc = 0;
    for (uint32_t i = 0; i < n; i++) {
        u32 w[8];
        ld(w, scalars + 32 * (size_t)i, 8);
        auto emit = [&](u32, u32 mag, u32 neg) {
            const u32 b = (mag + 1) >> 1;
            if (b < 1 || b > K) { rc = -1; return; }
            hist[b]++;
            neg_hist[b] += neg;
        };
        if (width == 12) sc_for_each_naf_digit<12>(w, emit);
        else sc_for_each_naf_digit<9>(w, emit);
    }
    return rc;
}

// The bit-interleaved form the one-wavefront Keccak keeps its words in (keccak_wave.h): even / odd bits of x as two 32-bit halves.
// 1 when the halves join back to x AND rotl64(x, r) is what the halves give under the rule kw_setup derives its lane shifts from
// (even r: both halves rotate by r / 2; odd r: the halves change places, odd -> even by (r + 1) / 2, even -> odd by (r - 1) / 2).
int hc_kw_interleave(uint64_t x, int r) {
    const u32 e = kw_half(x, 0), o = kw_half(x, 1);
    if (kw_join(e, o) != x) return 0;
    auto rotl32 = [](u32 v, int k) { k &= 31; return k ? (u32)((v << k) | (v >> (32 - k))) : v; };
    u32 e2, o2;
    if (r % 2 == 0) {
        e2 = rotl32(e, r / 2);
        o2 = rotl32(o, r / 2);
    } else {
        e2 = rotl32(o, (r + 1) / 2);
        o2 = rotl32(e, (r - 1) / 2);
    }
    const uint64_t want = r ? (x << r) | (x >> (64 - r)) : x;
    return kw_join(e2, o2) == want ? 1 : 0;
}

// Host MODEL of the one-wavefront Keccak (keccak_wave.h BBP_KW_ROUND, instruction for instruction on arrays of 64 lanes): the lane
// tables of kw_setup / kw_iota_setup are the product's own, the cross-lane operations are restated from the ISA (DPP row shifts with
// bound_ctrl / bank masks, v_permlane16_swap, v_permlane32_swap, ds_bpermute).  What the CPU tier can say about the kernel: the
// layout, the shift amounts, the gather addresses and the order of operations permute like Keccak-f[1600].
struct KwVec {
    u32 v[64];
};
static KwVec kw_dpp_shl(const KwVec& a, int n) {  // row_shl:n bound_ctrl: lane i reads lane i + n of its 16-lane row, 0 past the row
    KwVec r;
    for (int L = 0; L < 64; L++) r.v[L] = (L & 15) + n < 16 ? a.v[L + n] : 0u;
    return r;
}
static KwVec kw_dpp_shr(const KwVec& a, int n) {
    KwVec r;
    for (int L = 0; L < 64; L++) r.v[L] = (L & 15) - n >= 0 ? a.v[L - n] : 0u;
    return r;
}
static u32 kw_rotr32(u32 x, u32 s) { s &= 31; return s ? (x >> s) | (x << (32 - s)) : x; }  // v_alignbit_b32 x, x, s
void hc_kw_keccak_f(uint8_t* st200) {
    u64 st[25];
    memcpy(st, st200, 200);
    kw_lane c[64];
    kw_iota k[64];
    KwVec x;
    for (u32 L = 0; L < 64; L++) {
        c[L] = kw_setup(L);
        k[L] = kw_iota_setup(L);
        x.v[L] = c[L].live ? kw_half(st[c[L].word], c[L].half) : 0u;
    }
    for (int r = 0; r < 24; r++) {
        KwVec t0, t1, t2, t3, t4;
        for (int L = 0; L < 64; L++) t0.v[L] = x.v[L] ^ k[L].v[r];                      // a = x ^ pending iota
        const KwVec s5 = kw_dpp_shl(x, 5), s10 = kw_dpp_shl(x, 10), r5 = kw_dpp_shr(x, 5), r10 = kw_dpp_shr(x, 10);
        for (int L = 0; L < 64; L++) {
            t1.v[L] = x.v[L] ^ s5.v[L] ^ r10.v[L];
            t2.v[L] = s10.v[L];
            t3.v[L] = r5.v[L];
            t4.v[L] = t1.v[L] ^ t2.v[L] ^ t3.v[L];
            t1.v[L] = t4.v[L];
        }
        // v_permlane16_swap t1, t4: rows (a0, a1, a2, a3), (b0, b1, b2, b3) -> (a0, b0, a2, b2), (a1, b1, a3, b3)
        KwVec A = t1, Bv = t4;
        for (int L = 0; L < 16; L++) {
            t1.v[16 + L] = Bv.v[L];       t4.v[L] = A.v[16 + L];
            t1.v[48 + L] = Bv.v[32 + L];  t4.v[32 + L] = A.v[48 + L];
        }
        for (int L = 0; L < 64; L++) {
            t2.v[L] = t1.v[L] ^ t4.v[L] ^ k[L].cp[r];                                  // C of this lane's half
            t3.v[L] = kw_rotr32(t2.v[L], c[L].sh_theta);
        }
        KwVec um = kw_dpp_shr(t2, 1), nx = kw_dpp_shl(t3, 1);
        for (int L = 0; L < 64; L++) {
            const int pos = L & 15;
            if (pos < 4) um.v[L] = t2.v[L + 4];   // row_shl:4 bank_mask:0x1 (source always inside the row)
            if (pos >= 8) nx.v[L] = t3.v[L - 4];  // row_shr:4 bank_mask:0xc
        }
        // v_permlane32_swap t4 (= nx), t2 (= copy): (lo, hi), (lo', hi') -> (lo, lo'), (hi, hi')
        KwVec P = nx, Q = nx;
        for (int L = 0; L < 32; L++) {
            P.v[32 + L] = nx.v[L];  // vdst upper half <- src lower half
            Q.v[L] = nx.v[32 + L];  // src lower half <- vdst upper half
        }
        for (int L = 0; L < 64; L++) {
            const u32 d = um.v[L] ^ nx.v[L] ^ P.v[L] ^ Q.v[L];
            t0.v[L] = kw_rotr32(t0.v[L] ^ (d & c[L].live), c[L].sh_rho);
        }
        for (int L = 0; L < 64; L++) {
            const u32 b0 = t0.v[c[L].s0 / 4], b1 = t0.v[c[L].s1 / 4], b2 = t0.v[c[L].s2 / 4];
            x.v[L] = b0 ^ (~b1 & b2);
        }
    }
    for (u32 L = 0; L < 32; L++)
        if (c[L].live) st[c[L].word] = kw_join(x.v[L] ^ k[L].v[24], x.v[L + 32] ^ k[L + 32].v[24]);
    memcpy(st200, st, 200);
}

uint64_t hc_rotl64(uint64_t x, int n) { return rotl64(x, n); }

void hc_keccak_f(uint8_t* st200) {
    u64 s[25];
    memcpy(s, st200, 200);
    keccak_f1600(s);
    memcpy(st200, s, 200);
}

// merlin: Transcript(label) ; append_message(l1, m1) ; challenge_bytes(l2, n)
void hc_merlin_kat(const uint8_t* label, int label_len, const uint8_t* l1, int l1_len, const uint8_t* m1, int m1_len,
                   const uint8_t* l2, int l2_len, uint8_t* out, int n) {
    merlin_transcript t;
    merlin_init(t, label, label_len);
    merlin_append(t, l1, l1_len, m1, m1_len);
    merlin_challenge(t, l2, l2_len, out, n);
}

// bulk 64-byte draws vs the generic byte-wise path: out_generic / out_bulk = (1 + count + 1) * 64 bytes each
int hc_merlin_rng_bulk(const uint8_t* w, int w_len, const uint8_t* ent32, int count, uint8_t* out_generic, uint8_t* out_bulk) {
    merlin_transcript t;
    merlin_init(t, (const uint8_t*)"BlindBidProofGadget", 19);
    merlin_transcript a = t;
    merlin_rng_rekey(a, (const uint8_t*)"v_blinding", 10, w, w_len);
    merlin_rng_finalize(a, ent32);
    merlin_transcript b = a;
    for (int i = 0; i < count + 2; i++) merlin_rng_fill(a, out_generic + 64 * i, 64);
    merlin_rng_fill(b, out_bulk, 64);
    u32* words = new u32[16 * count];
    bool ok = merlin_rng_fill64_bulk(b, count, words);
    memcpy(out_bulk + 64, words, 64 * (size_t)count);
    delete[] words;
    merlin_rng_fill(b, out_bulk + 64 * (count + 1), 64);
    return ok ? 1 : 0;
}

// TranscriptRng: Transcript(label); rng = build_rng().rekey(wl, w).finalize(ent32); fill n bytes twice
void hc_merlin_rng(const uint8_t* label, int label_len, const uint8_t* wl, int wl_len, const uint8_t* w, int w_len,
                   const uint8_t* ent32, uint8_t* out, int n) {
    merlin_transcript t;
    merlin_init(t, label, label_len);
    merlin_transcript r = t;
    merlin_rng_rekey(r, wl, wl_len, w, w_len);
    merlin_rng_finalize(r, ent32);
    merlin_rng_fill(r, out, n);
    merlin_rng_fill(r, out + n, n);
}

// ---- radix-16 scalar multiplication (csrc/scalarmul.h): the host twins of device_check.hip's dc_comb, dc_comb_table, dc_tail,
// dc_tail_pair and dc_straus, same arguments, same outputs.  What a wavefront does with shuffles on the device (commit_group_sum, the
// 32-lane sum of k_varsum) is a loop over the lanes' partial sums here.  Returns 0, or 1 for an index, a piece range
// or a scalar the product never feeds these functions (non-canonical: the 8-entry tables are indexed by digit magnitude).
static bool hc_canonical(const uint8_t* s32, size_t n) {
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        ld(w, s32 + 32 * i, 8);
        if (!sc_is_canonical(w)) return false;
    }
    return true;
}
static bool hc_below(const uint32_t* idx, size_t n, int bound) {
    for (size_t i = 0; i < n; i++)
        if (idx[i] >= (uint32_t)bound) return false;
    return true;
}
static sc hc_scalar(const uint8_t* s32) {
    sc s;
    ld(s.v, s32, 8);
    return s;
}
static std::vector<ge> hc_points(int np, const uint8_t* pts32, int32_t* ok) {
    std::vector<ge> pts((size_t)np);
    for (int i = 0; i < np; i++) {
        u32 w[8];
        ld(w, pts32 + 32 * (size_t)i, 8);
        ok[i] = ge_decode_words(pts[i], w) ? 1 : 0;
    }
    return pts;
}
static std::vector<niels_packed> hc_comb_tables(const std::vector<ge>& bases) {
    std::vector<niels_packed> comb(64 * 8 * bases.size());
    for (size_t b = 0; b < bases.size(); b++)
        for (u32 j = 0; j < 64; j++) comb_build_column(bases[b], j, comb.data() + (b * 64 + j) * 8);
    return comb;
}
static std::vector<ge> hc_tail_tables(const std::vector<ge>& pts) {
    std::vector<ge> tab((size_t)TAIL_TAB * pts.size());
    for (size_t i = 0; i < pts.size(); i++) tail_table_build(pts[i], tab.data() + i * TAIL_TAB);
    return tab;
}

int hc_comb(int nb, const uint8_t* bases32, int n, const uint32_t* idx0, const uint32_t* idx1, const uint8_t* v32, const uint8_t* b32,
            uint8_t* out_one32, uint8_t* out_split32, int32_t* base_ok) {
    if (nb <= 0 || n <= 0 || !hc_below(idx0, (size_t)n, nb) || !hc_below(idx1, (size_t)n, nb)) return 1;
    if (!hc_canonical(v32, (size_t)n) || !hc_canonical(b32, (size_t)n)) return 1;
    const std::vector<niels_packed> comb = hc_comb_tables(hc_points(nb, bases32, base_ok));
    for (int i = 0; i < n; i++) {
        const sc v = hc_scalar(v32 + 32 * (size_t)i), b = hc_scalar(b32 + 32 * (size_t)i);
        const niels_packed *c0 = comb.data() + (size_t)idx0[i] * 64 * 8, *c1 = comb.data() + (size_t)idx1[i] * 64 * 8;
        ge_encode(out_one32 + 32 * (size_t)i, comb_mul_add(comb_mul_add(ge_identity(), c0, v), c1, b));
        ge part[COMMIT_L];
        for (u32 q = 0; q < (u32)COMMIT_L; q++) part[q] = comb_mul_add_part(comb_mul_add_part(ge_identity(), c0, v, q), c1, b, q);
        for (int d = COMMIT_L / 2; d >= 1; d >>= 1)  // commit_group_sum: lane q adds lane q + d
            for (int q = 0; q < d; q++) part[q] = ge_add(part[q], part[q + d]);
        ge_encode(out_split32 + 32 * (size_t)i, part[0]);
    }
    return 0;
}

int hc_comb_table(int nb, const uint8_t* bases32, uint8_t* out32, int32_t* base_ok) {
    if (nb <= 0) return 1;
    const std::vector<niels_packed> comb = hc_comb_tables(hc_points(nb, bases32, base_ok));
    for (size_t i = 0; i < comb.size(); i++) {
        ge_niels e;
        BBP_COMB_LOAD(e, comb.data() + i);
        ge_encode(out32 + 32 * i, ge_from_niels(e));
    }
    return 0;
}

int hc_tail_pieces() { return TAIL_PIECES; }

int hc_tail(int np, const uint8_t* pts32, int n, const uint32_t* pidx, const uint8_t* s32, const int32_t* k_lo, const int32_t* k_hi,
            uint8_t* out32, int32_t* pt_ok) {
    if (np <= 0 || n <= 0 || !hc_below(pidx, (size_t)n, np) || !hc_canonical(s32, (size_t)n)) return 1;
    for (int i = 0; i < n; i++)
        if (k_lo[i] < 0 || k_lo[i] > k_hi[i] || k_hi[i] > TAIL_PIECES) return 1;
    const std::vector<ge> tab = hc_tail_tables(hc_points(np, pts32, pt_ok));
    for (int i = 0; i < n; i++)
        ge_encode(out32 + 32 * (size_t)i, ge_scalarmul_pieces(hc_scalar(s32 + 32 * (size_t)i), tab.data() + (size_t)pidx[i] * TAIL_TAB, k_lo[i], k_hi[i]));
    return 0;
}

int hc_tail_pair(int np, const uint8_t* pts32, int n, const uint32_t* pidx1, const uint8_t* s1, const uint32_t* pidx2, const uint8_t* s2,
                 uint8_t* out32, int32_t* pt_ok) {
    if (np <= 0 || n <= 0 || !hc_below(pidx1, (size_t)n, np) || !hc_below(pidx2, (size_t)n, np)) return 1;
    if (!hc_canonical(s1, (size_t)n) || !hc_canonical(s2, (size_t)n)) return 1;
    const std::vector<ge> tab = hc_tail_tables(hc_points(np, pts32, pt_ok));
    for (int i = 0; i < n; i++)
        ge_encode(out32 + 32 * (size_t)i, ge_scalarmul_pieces_pair(hc_scalar(s1 + 32 * (size_t)i), tab.data() + (size_t)pidx1[i] * TAIL_TAB,
                                                                    hc_scalar(s2 + 32 * (size_t)i), tab.data() + (size_t)pidx2[i] * TAIL_TAB));
    return 0;
}

int hc_straus(int np, const uint8_t* pts32, int n, const int32_t* cnt, const uint32_t* pidx, const uint8_t* s32, uint8_t* out_top32,
              uint8_t* out_lane32, uint32_t* sp_out, int32_t* pt_ok) {
    constexpr int STRAUS_MAX = 4;
    if (np <= 0 || n <= 0 || !hc_below(pidx, (size_t)n * STRAUS_MAX, np) || !hc_canonical(s32, (size_t)n * STRAUS_MAX)) return 1;
    for (int i = 0; i < n; i++)
        if (cnt[i] < 0 || cnt[i] > STRAUS_MAX) return 1;
    const std::vector<ge> pts = hc_points(np, pts32, pt_ok);
    std::vector<ge> tab(8 * pts.size());
    for (size_t i = 0; i < pts.size(); i++) straus_table(tab.data() + 8 * i, pts[i]);
    memset(sp_out, 0, 32 * (size_t)n * STRAUS_MAX);
    for (int i = 0; i < n; i++) {
        const size_t pt0 = (size_t)i * STRAUS_MAX;
        for (int a = 0; a < cnt[i]; a++) straus_recode(sp_out + 8 * (pt0 + a), hc_scalar(s32 + 32 * (pt0 + a)));
        ge acc = ge_identity();  // as k_varbase
        for (int j = 63; j >= 0; j--) {
            if (j != 63)
                for (int k = 0; k < 4; k++) acc = ge_dbl(acc);
            for (int a = 0; a < cnt[i]; a++) acc = straus_digit_step(acc, tab.data() + (size_t)pidx[pt0 + a] * 8, sp_out + 8 * (pt0 + a), j);
        }
        ge_encode(out_top32 + 32 * (size_t)i, acc);
        // as k_varsum: lane l's partial sum S_l over digits 2l + 1 and 2l; the kernel then doubles S_l 8 l times and adds the 32 lanes up
        // with shuffles -- here sum_l 2^(8 l) S_l is taken by Horner's rule from the top lane down (the same group element, 248 doublings)
        ge lanes = ge_identity();
        for (int lane = 31; lane >= 0; lane--) {
            ge l = ge_identity();
            for (int hi = 1; hi >= 0; hi--) {
                if (!hi)
                    for (int k = 0; k < 4; k++) l = ge_dbl(l);
                const u32 j = 2 * (u32)lane + (u32)hi;
                for (int a = 0; a < cnt[i]; a++) l = straus_digit_step(l, tab.data() + (size_t)pidx[pt0 + a] * 8, sp_out + 8 * (pt0 + a), j);
            }
            if (lane != 31)
                for (int k = 0; k < 8; k++) lanes = ge_dbl(lanes);
            lanes = ge_add(lanes, l);
        }
        ge_encode(out_lane32 + 32 * (size_t)i, lanes);
    }
    return 0;
}
}
