// The device-resident circuit tables, the batch buffer's entry points (prover and verifier share them) and the engine's calls that the
// C-API units make (prover.hip and verifier.inc define them and see these declarations too), with small load/store helpers.
// The batch buffer itself -- BatchDev, its carve, views and strides -- is batch_layout.h's one table (DESIGN.md "The batch buffer").
#pragma once
#include <functional>

#include "batch_layout.h"
#include "circuit.h"
#include "context.h"
#include "keccak.h"

namespace bbp {

struct CircuitDev {  // compiled circuit tables resident on the device (one per bid-list length N)
    u32 n_items = 0, m = 0, n_mul = 0, n_cons = 0, padded = 0, n_cst = 0;
    u32 *w_terms = nullptr, *w_loff = nullptr, *w_roff = nullptr, *f_off = nullptr, *f_ent = nullptr, *c_q = nullptr, *c_cst = nullptr;
    u32 n_cterms = 0;
    u32* idx_ai = nullptr;   // base indices of A_I1's terms: B_blinding, G[0..n1), H[0..n1), equal-valued inputs merged (msm_index.h)
    u32* idx_s1 = nullptr;   // the same layout unmerged, for S1 (independent random scalars)
    u32 n_ai_terms = 0;      // terms of A_I1 that are not skipped
    u32* idx_ao = nullptr;   // B_blinding, G[0..n1)
    u32* idx_ipa = nullptr;  // [IPA_ROUNDS][2 (L,R)][IPA_TERMS]
    u32* idx_ver = nullptr;  // verifier fixed part: G[0..2048), H[0..2048), B, B_blinding
    BatchDims dims() const { return BatchDims{m, n_mul, n_cons, n_cst}; }  // what the batch buffer needs of the circuit
};

__device__ __forceinline__ sc ld_sc(const sc* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    return BBP_SC_LIT(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}
__device__ __forceinline__ void st_sc(sc* p, const sc& s) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(s.v[0], s.v[1], s.v[2], s.v[3]);
    q[1] = make_uint4(s.v[4], s.v[5], s.v[6], s.v[7]);
}

// prover.hip / verifier.hip
int32_t circuit_get(bbp_ctx* ctx, uint32_t n_items, const CircuitDev** out);
int32_t batch_reserve(bbp_ctx* ctx, uint32_t B, const BatchDims& d, BatchDev& bd, int buf);
int32_t commit_launch(bbp_ctx* ctx, u32 count, const sc* values, const sc* blindings, u32 stride_v, u32 stride_b, u32 per_proof,
                      ge* out, u32 out_stride, hipStream_t s);
// prover.hip: the prove call on device pointers; open_hook: see the definition
int32_t prove_batch_dev(bbp_ctx* ctx, u32 B, u32 N, const u8* in_dev, const u8* ent_dev, u8* out_dev, hipStream_t s,
                        const std::function<int32_t(hipStream_t)>* open_hook = nullptr);
int32_t debug_read_misc(bbp_ctx* ctx, u32 B, u32 N, u32 proof, uint8_t* out);
// verifier.inc: the plain and the aggregated driver; what the rows are travels in the descriptor (verify_rows.h)
int32_t verify_batch_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s);
int32_t verify_batch_agg_dev(bbp_ctx* ctx, const VerifyRows& v, u32 G, const u8* in_dev, const u8* ent_dev, int32_t* status_dev, hipStream_t s,
                             u32* n_fallback, u32* total_out_dev = nullptr);
int32_t debug_varbase(bbp_ctx* ctx, u32 form, u32 B, u32 Q, u32 agg, const u32* ns, const u8* vers, const u8* pts, const u8* scal, const u8* wv,
                      const u8* uj, u8* sums_out, u32* digits_out, int32_t* status_out);
// verifier.inc: k_round_consts for one round (the prove side's table reduction)
int32_t round_consts_launch(bbp_ctx* ctx, u32 N, const u8* round_dev, const u32* roff_dev, sc* rblk, int32_t* rflag, hipStream_t s);

}  // namespace bbp
