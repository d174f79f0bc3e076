// The device-resident circuit tables and the batch buffer's entry points (prover and verifier share them), with small load/store helpers.
// The batch buffer itself -- BatchDev, its carve, views and strides -- is batch_layout.h's one table (DESIGN.md "The batch buffer").
#pragma once
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

}  // namespace bbp
