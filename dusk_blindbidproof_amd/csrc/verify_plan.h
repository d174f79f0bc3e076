// How one verify call is laid out and launched: the knobs, what the plan needs of the circuits, the plan that plan_verify decides
// from them (front end, launch geometry, round offsets, the three scratch layouts) and the staging layout of one host-pointer call.
// verifier.inc and capi_verify.hip execute these values; nothing else decides (DESIGN.md section 4 "The plan of a verify call").
// Host arithmetic only, no HIP calls: the CPU test tier compiles it too (tests/host_check.cpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_layout.h"
#include "point.h"
#include "prove_io.h"
#include "scalar.h"
#include "verify_rows.h"

namespace bbp {

constexpr u32 VERIFY_MSM_TERMS = 4098;  // generator scalars of one proof's (or one group's) check, the same list for every N
constexpr int VC_U = 0, VC_UI = 11, VC_TX = 22, VC_TXB = 23, VC_EBL = 24, VC_A = 25, VC_B = 26, VC_COUNT = 27;  // a proof's vchal block
constexpr u32 VROWS_BLK = 1024;  // the one workgroup of k_vrows / k_vrows_rounds
constexpr int VS_BLK = 256;      // k_vscalars: one workgroup per proof
constexpr u32 GS_BLK = 256;      // k_group_sum
constexpr u32 ROUND_TABLE_MAX = 0x7fffffffu;  // scalars of a call's reduced round table at the most

struct VRow {  // one row of a mixed call: byte offset of its input row, N, m = 4 + N, record layout (0 compact, 1 two-phase)
    u64 off;
    u32 n;
    uint16_t m, ver;
};

inline u32 cdiv(u32 a, u32 b) { return (a + b - 1) / b; }

struct VerifyKnobs {
    int varbase_lanes = 65536;  // BBP_VARBASE_LANES (>= 64): lanes the variable-base kernel is launched with, about one wave per SIMD
    int overlap = 1;            // BBP_VERIFY_OVERLAP: lane 0's variable-base kernels on a side stream (no measurable difference with four lanes)
    int group = 0;              // BBP_VERIFY_AGGREGATE=G: the host API checks proofs in groups of G with per-proof fallback; up to 1 = off
    int varbase_v1 = -1;        // BBP_VARBASE_V1: 1 / 0 forces k_varbase / k_varprep + k_varsum; unset (-1) = by size (process)
    int fence = 0;              // BBP_V_FENCE (experiment): the transcript replay reserves its CUs like the prover's opening kernels (process)
    int host_chunk = 32768;     // BBP_HOST_CHUNK_VERIFY (>= 1): proofs per engine call of a host-pointer call (read at every call)
#ifdef BBP_EXPERIMENTS
    // BBP_KO_VERIFY, knock-out mask (timing experiments, WRONG results): skip 1 the MSM, 2 k_varbase, 4 k_vtranscript, 8 k_flatten,
    // 16 k_vscalars, 32 k_powers -- what a kernel costs the pipeline is what the step loses without it.  It changes VERDICTS (k_vfinal
    // would judge whatever an earlier call left in the lane's buffers), so it exists only in experiment builds (tools/build_variant.py
    // NAME -DBBP_EXPERIMENTS); in the product library it is the constant 0 and the name is not even a string in the binary
    // (tests/test_capi_symbols.py::test_no_verdict_changing_knobs_in_the_product).  Read once per process.
    int ko = 0;
#endif

    // the one list of environment names, by when the engine reads them; a null clamp takes the number as it is
    enum When { CONTEXT, PROCESS, CALL };  // at bbp_init | once per process | at every call
    struct Env {
        const char* name;
        int VerifyKnobs::*member;
        int (*clamp)(int);
        When when;
    };
    template <class F>
    static void each_env(F&& f) {
        static const Env table[] = {
            {"BBP_VARBASE_LANES", &VerifyKnobs::varbase_lanes, [](int v) { return v < 64 ? 64 : v; }, CONTEXT},
            {"BBP_VERIFY_OVERLAP", &VerifyKnobs::overlap, [](int v) { return v != 0 ? 1 : 0; }, CONTEXT},
            {"BBP_VERIFY_AGGREGATE", &VerifyKnobs::group, [](int v) { return v > 1 ? v : 0; }, CONTEXT},
            {"BBP_VARBASE_V1", &VerifyKnobs::varbase_v1, [](int v) { return v != 0 ? 1 : 0; }, PROCESS},
            {"BBP_V_FENCE", &VerifyKnobs::fence, nullptr, PROCESS},
            {"BBP_HOST_CHUNK_VERIFY", &VerifyKnobs::host_chunk, [](int v) { return v >= 1 ? v : 32768; }, CALL},
#ifdef BBP_EXPERIMENTS
            {"BBP_KO_VERIFY", &VerifyKnobs::ko, nullptr, PROCESS},
#endif
        };
        for (const Env& e : table) f(e);
    }
    // one knob from its environment text, clamped; false: the name is no verify knob
    bool set(const char* name, const char* text) {
        bool found = false;
        each_env([&](const Env& e) {
            if (strcmp(e.name, name)) return;
            this->*e.member = e.clamp ? e.clamp(atoi(text)) : atoi(text);
            found = true;
        });
        return found;
    }
    void read(When when) {
        each_env([&](const Env& e) {
            const char* text = e.when == when ? getenv(e.name) : nullptr;
            if (text) set(e.name, text);
        });
    }
    // BBP_VARBASE_V1, BBP_V_FENCE (and the experiment builds' knock-out mask): read once, by the first verify call of the process
    static const VerifyKnobs& process() {
        static const VerifyKnobs once = [] {
            VerifyKnobs k;
            k.read(PROCESS);
            return k;
        }();
        return once;
    }
    // ... which hands them to its context's knobs (every verify call does: a few assignments)
    void adopt_process() {
        const VerifyKnobs& p = process();
        each_env([&](const Env& e) {
            if (e.when == PROCESS) this->*e.member = p.*e.member;
        });
    }
    // a context's knobs at bbp_init: the per-context ones as the environment has them now; the process's are not looked at yet
    static VerifyKnobs from_env() {
        VerifyKnobs k;
        k.read(CONTEXT);
        return k;
    }
    static u32 host_chunk_now() {
        VerifyKnobs k;
        k.read(CALL);
        return (u32)k.host_chunk;
    }
#ifdef BBP_EXPERIMENTS
    int knocked_out() const { return ko; }
#else
    static constexpr int knocked_out() { return 0; }
#endif
};

// What the plan needs of the circuit is what the batch buffer needs (batch_layout.h): the prover passes a circuit's, a mixed front end
// the largest of each over the call's N.
using VerifyDims = BatchDims;

struct VLaunch {
    u32 grid = 0, block = 0;
};
// a byte range of a scratch buffer; a region the call does not use is {0, 0}
struct VRegion {
    size_t off = 0, bytes = 0;
};
struct VCarve {
    size_t end = 0;
    VRegion take(size_t bytes) {
        if (!bytes) return VRegion();
        const VRegion r{end, bytes};
        end += align256(bytes);
        return r;
    }
};

// The variable-base launches of B rows whose largest row has m commitments (the strides): np point slots per row, npa of them
// active (a compact record leaves three empty).  vb2: k_varprep + k_varsum, one sum per row; else k_varbase on Q lanes per row with
// Q sums.  one_phase: the uniform kernels' record layout.  verify_batch_dev and bbp_debug_varbase share it.
struct VarbaseGeom {
    u32 B = 0, m = 0, np = 0, npa = 0, Q = 1, one_phase = 1;
    bool vb2 = true;
    VLaunch prep, sum, lanes;
};
inline VarbaseGeom varbase_geom(u32 B, u32 m, bool two_phase, bool vb2, u32 Q) {
    VarbaseGeom g;
    g.B = B, g.m = m, g.np = 6 + m + 5 + 22, g.npa = g.np - (two_phase ? 0u : 3u);
    g.vb2 = vb2, g.Q = vb2 ? 1u : Q, g.one_phase = two_phase ? 0u : 1u;
    g.prep = {cdiv(B * g.npa, 64), 64}, g.sum = {cdiv(B, 2), 64}, g.lanes = {cdiv(B * g.Q, 64), 64};
    return g;
}

// L.agg_io of an aggregated call (the fallback's outputs): sized from B alone, reserved before the group pass is enqueued
struct AggIoLayout {
    VRegion fixed, idx;
    size_t bytes;
    explicit AggIoLayout(u32 B) {
        VCarve c;
        fixed = c.take((size_t)B * sizeof(ge)), idx = c.take(4 * (size_t)B);
        bytes = c.end;
    }
};

struct VerifyPlan {
    enum Front { UNIFORM, MIXED, ROUND1, ROUNDS_MX };  // k_vparse | k_vparse_mx | k_vparse_round | k_vparse_rounds_mx
    Front front = UNIFORM;
    bool mixed = false, rounds = false;  // the _mx kernels run | the call takes seed and list from a round table
    u32 B = 0, G = 0, R = 0;
    VerifyDims d;
    VarbaseGeom vb;         // m, np, npa, Q, vb2, one_phase and the variable-base grids
    u32 vstride = 0;        // words of a row's point slots: np * 8
    u32 zstride = 0;        // z powers per row: n_cons + 1
    u32 zchunks = 0;        // ... in chunks of 32
    u32 n_tgt = 0;          // flatten targets per row: 3 n_mul + m
    u32 vtw = 0;            // 1: the transcript replay runs one proof per wavefront
    u32 ng = 0;             // groups of an aggregated pass: ceil(B / G)
    u32 agg_flag = 0;       // what the kernels that weight a proof are told: 1 when G > 0
    VLaunch fill_mimc, round_consts, vrows, parse, transcript, powers_z, powers_yinv, flatten, vscalars,
        per_row /* k_vfinal, k_var_sum, k_fallback_final */, group_sum /* x; y = ng */, group_final, compact /* k_compact_failing */;
    // rounds: scalar offset of every round in the reduced table (1 + N scalars each), the total at [R]
    std::vector<u32> rd_off;
    u32 rd_S = 0, rd_nof = 0;  // the total | entries of round_of on the device (several rounds only)
    bool rd_too_large = false;
    struct Misc {
        VRegion vpts, vchal, vs, tab, var, fixed, sp, rows, ns /* Ns, then the version bytes */, rof /* round_of, then rd_off */, rblk, rflag;
        size_t bytes = 0;
    } misc;
    struct Agg {
        VRegion vsg, fixedg, varsum, gstatus;
        size_t bytes = 0;
    } agg;
    AggIoLayout agg_io{0};
};

// a rounds call whose reduced table would hold more than ROUND_TABLE_MAX scalars is refused
inline bool round_table_too_large(const VerifyRows& v) {
    u64 total = 0;
    for (u32 r = 0; v.kind == VerifyRows::ROUNDS && r < v.R; r++) total += 1 + (u64)v.round_ns[r];
    return total > ROUND_TABLE_MAX;
}
// scalars of the reduced round table of a rounds call, and every round's offset in it
inline u64 round_offsets(const VerifyRows& v, std::vector<u32>& off) {
    off.assign((size_t)v.R + 1, 0);
    u64 total = 0;
    for (u32 r = 0; r < v.R; r++) {
        off[r] = (u32)total;
        total += 1 + (u64)v.round_ns[r];
    }
    off[v.R] = (u32)total;
    return total;
}

// The one place that decides.  G: 0 plain, else the group size of the aggregated pass.  tr_wave_below: ProveKnobs' (the replay takes
// the prover's rule).
inline VerifyPlan plan_verify(const VerifyRows& v, const VerifyDims& d, u32 G, const VerifyKnobs& k, int tr_wave_below) {
    VerifyPlan p;
    const u32 B = v.B;
    p.B = B, p.G = G, p.d = d;
    p.mixed = v.mixed_front(), p.rounds = v.kind == VerifyRows::ROUNDS;
    p.front = p.mixed ? (p.rounds ? VerifyPlan::ROUNDS_MX : VerifyPlan::MIXED) : (p.rounds ? VerifyPlan::ROUND1 : VerifyPlan::UNIFORM);
    if (p.rounds) {
        p.R = v.R;
        p.rd_too_large = round_table_too_large(v);
        round_offsets(v, p.rd_off);
        p.rd_S = p.rd_off[v.R];
        p.rd_nof = p.mixed ? B : 0;
    }
    // lanes per proof in k_varbase: as few as still give the launch varbase_lanes lanes (fewer lanes = more points per lane sharing
    // one doubling chain).  k_varprep + k_varsum (half a wavefront per proof, shared doublings, one partial sum per proof) for calls
    // below 4096 proofs: above, the machine is throughput-bound either way and the first version's shorter chain wins (8192 per
    // call: 40.8 vs 42.2 ms, aggregated 14.8 vs 16.3 ms).  BBP_VARBASE_V1=1 / 0 forces one or the other.
    const u32 npa = 6 + d.m + 5 + 22 - (v.rec_ver ? 0u : 3u);
    u32 Q = B ? (u32)k.varbase_lanes / B : 1;
    Q = Q < 1 ? 1 : Q > npa ? npa : Q;
    p.vb = varbase_geom(B, d.m, v.rec_ver != 0, k.varbase_v1 < 0 ? B < 4096 : k.varbase_v1 == 0, Q);
    const u32 np = p.vb.np;
    p.vstride = np * 8, p.zstride = d.n_cons + 1, p.zchunks = cdiv(d.n_cons + 1, 32), p.n_tgt = 3 * d.n_mul + d.m;
    p.vtw = B <= (u32)tr_wave_below ? 1u : 0u;  // the replay of a few proofs: a wavefront each (as the prover's transcript kernels)
    p.ng = G ? cdiv(B, G) : 0, p.agg_flag = G ? 1u : 0u;

    p.fill_mimc = {cdiv(B * BBP_MIMC_ROUNDS, 64), 64};
    p.round_consts = {cdiv(p.rd_S, 64), 64};
    p.vrows = {1, VROWS_BLK};
    p.parse = {cdiv(B, 64), 64};
    p.transcript = {p.vtw ? B : cdiv(B, 64), 64};
    p.powers_z = {cdiv(B * p.zchunks, 64), 64};
    p.powers_yinv = {cdiv(B * cdiv(IPA_N, 32), 64), 64};
    p.flatten = {cdiv(B * p.n_tgt, 128), 128};
    p.vscalars = {B, (u32)VS_BLK};
    p.per_row = {cdiv(B, 64), 64};
    p.group_sum = {cdiv(VERIFY_MSM_TERMS, GS_BLK), GS_BLK};
    p.group_final = {cdiv(p.ng, 64), 64};
    p.compact = {1, 1024};

    const size_t b = B, S = sizeof(sc);
    VCarve c;
    VerifyPlan::Misc& m = p.misc;
    m.vpts = c.take(b * np * 32), m.vchal = c.take(b * VC_COUNT * 32), m.vs = c.take(b * VERIFY_MSM_TERMS * 32);
    m.tab = c.take(b * np * 8 * sizeof(ge)), m.var = c.take(b * np * sizeof(ge)), m.fixed = c.take(b * sizeof(ge)), m.sp = c.take(b * np * 32);
    m.rows = c.take(p.mixed ? b * sizeof(VRow) : 0), m.ns = c.take(p.mixed && !p.rounds ? b * 5 : 0);
    m.rof = c.take(p.rounds ? 4 * ((size_t)p.rd_nof + p.R + 1) : 0), m.rblk = c.take((size_t)p.rd_S * S), m.rflag = c.take(4 * (size_t)p.R);
    m.bytes = c.end;
    if (G) {
        VCarve a;
        const size_t ng = p.ng;
        p.agg.vsg = a.take(ng * VERIFY_MSM_TERMS * 32), p.agg.fixedg = a.take(ng * sizeof(ge)), p.agg.varsum = a.take(b * sizeof(ge));
        p.agg.gstatus = a.take(ng * 4);
        p.agg.bytes = a.end;
        p.agg_io = AggIoLayout(B);
    }
    return p;
}

// The staging slot of one host-pointer verify call (context.h IoSlot; the counterpart of prove_io.h's ProveStaging).  `in`: the rows
// at 0, a rounds call's table behind them; `ent`: 32 bytes per row, uploaded or drawn on the device; `out`: B statuses and the
// aggregated engine's fallback counter.  group: the caller's; ctx_group: the context's (BBP_VERIFY_AGGREGATE).
struct VerifyStaging {
    std::vector<size_t> row_off;  // byte offset of every row in `in`
    size_t in_bytes, tab_off, tab_bytes;
    size_t ent_up_bytes, ent_drawn;  // one of the two is 0
    size_t out_bytes, fetch_bytes;   // B + 1 words reserved; the counter is fetched by an aggregated call only
    u32 group;                       // the effective group size: 0 = plain
    u32 n_chunks, chunk;             // engine calls, and rows of each but the last

    VerifyStaging(const VerifyRows& rows, u32 group_, u32 ctx_group, bool dev_draw, u32 host_chunk) : row_off(rows.offsets()) {
        const size_t B = rows.B;
        in_bytes = row_off[B], tab_bytes = rows.table_bytes(), tab_off = align256(in_bytes);
        ent_up_bytes = dev_draw ? 0 : 32 * B, ent_drawn = dev_draw ? 32 * B : 0;
        // the aggregated path takes compact records only: one two-phase row and the call runs plain; the context's group size
        // applies to calls of at least two groups
        group = rows.rec_ver ? 0 : group_;
        if (group == 0 && rows.rec_ver == 0 && ctx_group > 1 && rows.B >= 2 * ctx_group) group = ctx_group;
        out_bytes = 4 * (B + 1), fetch_bytes = 4 * (B + (group > 1 ? 1 : 0));
        n_chunks = (rows.B + host_chunk - 1) / host_chunk, chunk = n_chunks ? (rows.B + n_chunks - 1) / n_chunks : 0;  // bounded scratch for any B
    }
};

}  // namespace bbp
