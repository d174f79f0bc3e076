// Test-only shim, the device twin of host_check.cpp: compiles the PRODUCT's limb arithmetic, scalar, point and Keccak headers for
// gfx950 with the product's own hipcc flags, so the gpu test tier can compare the code the library actually runs (inline-asm
// multiply chains, v_alignbit rotations, the one-wavefront permutation, the MSM row loads) with the big-int oracle at its edges.
// Nothing in the shipped library calls this.  Built twice by __graft_entry__.build_devcheck: as shipped, and with -DBBP_FE_NO_CHAIN.
//
// Every entry point is batched: allocate, copy in, launch ONE kernel on the default stream, synchronise, copy out, free; the return
// value is the first hipError_t met (0 = hipSuccess).  One item per thread (one wavefront per state for the wave Keccak); every
// device store lands in the item's own fixed slot, so a wrong kernel gives a wrong answer, never an out-of-bounds write.
#define BBP_KECCAK_WAVE 1  // as prover.hip: keccak_f1600_wave and the merlin_transcript::wave path
#include <hip/hip_runtime.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/keccak_wave.h"
#include "../dusk_blindbidproof_amd/csrc/point.h"
#include "../dusk_blindbidproof_amd/csrc/scalar.h"
#include "../dusk_blindbidproof_amd/csrc/scalarmul.h"

using namespace bbp;

namespace {

constexpr int BLOCK = 64;
constexpr int NAF_SLOT = 32;  // digits kept per item by dc_sc_naf (widths 12 and 9 need at most 22 / 29)

// device buffers of one call, freed on every path; after the first error nothing more is allocated, copied or launched
struct Call {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 1);
        if (err == hipSuccess) {
            ptrs.push_back(d);
            err = hipMemset(d, 0, bytes ? bytes : 1);
        }
        return err == hipSuccess ? d : nullptr;
    }
    template <class T>
    T* in(const void* host, size_t bytes) {
        void* d = alloc(bytes);
        if (err == hipSuccess && bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return static_cast<T*>(d);
    }
    template <class T>
    T* out(size_t bytes) { return static_cast<T*>(alloc(bytes)); }
    template <class K, class... A>
    void launch(K kernel, u32 blocks, u32 threads, A... args) {
        if (err != hipSuccess || blocks == 0) return;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, 0, args...);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    void back(void* host, const void* dev, size_t bytes) {
        if (err == hipSuccess && bytes) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
    }
    ~Call() {
        for (void* p : ptrs) (void)hipFree(p);
    }
};

u32 blocks_for(int n) { return n > 0 ? (u32)((n + BLOCK - 1) / BLOCK) : 0u; }

__device__ __forceinline__ int item() { return (int)(blockIdx.x * blockDim.x + threadIdx.x); }

__device__ __forceinline__ void ld_words(u32* w, const u8* b, int nwords) {
    for (int i = 0; i < nwords; i++) w[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
}

__device__ __forceinline__ fe ld_limbs(const i32* p) {
    fe r;
    for (int i = 0; i < 10; i++) r.v[i] = p[i];
    return r;
}

// ---- field -------------------------------------------------------------------------------------------------------------------
// op: as host_check.cpp hc_fe_op 0..10
__global__ void k_fe_op(int op, int n, const u8* a32, const u8* b32, u8* out32) {
    const int i = item();
    if (i >= n) return;
    u32 wa[8], wb[8];
    ld_words(wa, a32 + 32 * (size_t)i, 8);
    ld_words(wb, b32 + 32 * (size_t)i, 8);
    fe a = fe_fromwords(wa), b = fe_fromwords(wb), r;
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
        case 10: {
            fe m1 = fe_mul(a, b), m2 = fe_sq(b), m3 = fe_mul(b, fe_sq(a));
            fe s = fe_add(fe_add(m1, m1), m2), d = fe_sub(fe_sub(m3, m2), m1);
            r = fe_mul(s, d);
            r = fe_sq(fe_sub(fe_add(r, m1), m3));
            break;
        }
        default: r = fe_zero(); break;
    }
    fe_tobytes(out32 + 32 * (size_t)i, r);
}

// raw signed limbs in, raw limbs and canonical bytes out.  op: 0 mul(a, b), 1 sq(a), 2 sq2(a), 3 mul_small(a, b[0]),
// 4 mul(a + b, a - b), 5 towords(a), 6 iszero(a), 7 isneg(a), 8 eq(a, b).  Ops 0..4 write the result's limbs and bytes;
// ops 5..8 write the bytes of a and the predicate as limb 0 of the output (the other nine zero).
__global__ void k_fe_limbs(int op, int n, const i32* a10, const i32* b10, i32* out10, u8* out32) {
    const int i = item();
    if (i >= n) return;
    const fe a = ld_limbs(a10 + 10 * (size_t)i), b = ld_limbs(b10 + 10 * (size_t)i);
    fe r = fe_zero();
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
    i32* o = out10 + 10 * (size_t)i;
    for (int k = 0; k < 10; k++) o[k] = r.v[k];
    fe_tobytes(out32 + 32 * (size_t)i, op >= 5 ? a : r);
}

// ---- scalars -----------------------------------------------------------------------------------------------------------------
// op as hc_sc_op: 0 add, 1 sub, 2 mul, 3 invert (safegcd), 4 from_wide(a64), 5 from_bits(a32), 6 neg, 7 invert_fermat.
// a is read at a 64-byte stride for every op (only op 4 uses all of it).
__global__ void k_sc_op(int op, int n, const u8* a64, const u8* b32, u8* out32) {
    const int i = item();
    if (i >= n) return;
    sc x, y, r;
    u32 w[16];
    ld_words(w, a64 + 64 * (size_t)i, 16);
    if (op == 4) {
        r = sc_from_wide(w);
    } else if (op == 5) {
        r = sc_from_bits(w);
    } else {
        for (int k = 0; k < 8; k++) x.v[k] = w[k];
        ld_words(y.v, b32 + 32 * (size_t)i, 8);
        switch (op) {
            case 0: r = sc_add(x, y); break;
            case 1: r = sc_sub(x, y); break;
            case 2: r = sc_mul(x, y); break;
            case 3: r = sc_invert(x); break;
            case 7: r = sc_invert_fermat(x); break;
            default: r = sc_neg(x); break;
        }
    }
    sc_tobytes(out32 + 32 * (size_t)i, r);
}

__global__ void k_sc_is_canonical(int n, const u8* a32, i32* out) {
    const int i = item();
    if (i >= n) return;
    u32 w[8];
    ld_words(w, a32 + 32 * (size_t)i, 8);
    out[i] = sc_is_canonical(w) ? 1 : 0;
}

// NAF recoding: item i writes at most NAF_SLOT (position, digit) pairs into its slot; count[i] is the number of digits produced,
// which may exceed the slot (the test then fails on the count, not on memory)
template <int WID>
__global__ void k_sc_naf(int n, const u8* a32, i32* pos, i32* dig, i32* count) {
    const int i = item();
    if (i >= n) return;
    u32 w[8];
    ld_words(w, a32 + 32 * (size_t)i, 8);
    i32* p = pos + NAF_SLOT * (size_t)i;
    i32* d = dig + NAF_SLOT * (size_t)i;
    int k = 0;
    sc_for_each_naf_digit<WID>(w, [&](u32 at, u32 mag, u32 neg) {
        if (k < NAF_SLOT) {
            p[k] = (i32)at;
            d[k] = neg ? -(i32)mag : (i32)mag;
        }
        k++;
    });
    count[i] = k;
}

// ---- points ------------------------------------------------------------------------------------------------------------------
// decode -> op -> encode, as hc_ge_op: 0 round trip, 1 double, 2 add(a, b), 3 sub(a, b), 4 madd(a, niels(b)), 5 msub(a, niels(b)).
// status 1 when every decode the op needs succeeded (out then holds the encoding), 0 otherwise.
__global__ void k_ge_op(int op, int n, const u8* a32, const u8* b32, u8* out32, i32* status) {
    const int i = item();
    if (i >= n) return;
    u32 w[8];
    ge a, b, r;
    ld_words(w, a32 + 32 * (size_t)i, 8);
    bool ok = ge_decode_words(a, w);
    ld_words(w, b32 + 32 * (size_t)i, 8);
    if (op >= 2) ok = ge_decode_words(b, w) && ok;
    switch (op) {
        case 0: r = a; break;
        case 1: r = ge_dbl(a); break;
        case 2: r = ge_add(a, b); break;
        case 3: r = ge_sub(a, b); break;
        case 4: r = ge_madd(a, ge_to_niels(b, fe_invert(b.Z))); break;
        default: r = ge_msub(a, ge_to_niels(b, fe_invert(b.Z))); break;
    }
    status[i] = ok ? 1 : 0;
    if (ok) ge_encode(out32 + 32 * (size_t)i, r);
}

__global__ void k_from_uniform(int n, const u8* in64, u8* out32) {
    const int i = item();
    if (i >= n) return;
    u32 w[16];
    ld_words(w, in64 + 64 * (size_t)i, 16);
    ge_encode(out32 + 32 * (size_t)i, ge_from_uniform_words(w));
}

// the MSM accumulate step: acc (decoded, then doubled twice so that Z != 1) +/- the row of pt, the row built by niels_to_row
// into this item's 128-byte slot of `rows` and read back by load_row_at, as msm.hip reads its table
constexpr int ROW_DOUBLINGS = 2;
__global__ void k_madd_row(int n, const u8* acc32, const u8* pt32, u32 neg, niels_row* rows, u8* out32, i32* status) {
    const int i = item();
    if (i >= n) return;
    u32 w[8];
    ge acc, q;
    ld_words(w, acc32 + 32 * (size_t)i, 8);
    bool ok = ge_decode_words(acc, w);
    ld_words(w, pt32 + 32 * (size_t)i, 8);
    ok = ge_decode_words(q, w) && ok;
    for (int k = 0; k < ROW_DOUBLINGS; k++) acc = ge_dbl(acc);
    rows[i] = niels_to_row(ge_to_niels(q, fe_invert(q.Z)));
    const row_regs rr = load_row_at(rows + i, neg & 1u);
    status[i] = ok ? 1 : 0;
    if (ok) ge_encode(out32 + 32 * (size_t)i, ge_madd_row(acc, rr, (neg & 1u) != 0));
}

// ---- Keccak ------------------------------------------------------------------------------------------------------------------
__global__ void k_rotl64(int n, const u64* x, int amount, u64* out) {
    const int i = item();
    if (i >= n) return;
    out[i] = rotl64(x[i], amount);
}

template <int... K>
__device__ __forceinline__ void rotl64_literals(u64 x, u64* o, std::integer_sequence<int, K...>) {
    ((o[K] = rotl64(x, K)), ...);
}
__global__ void k_rotl64_const(int n, const u64* x, u64* out) {  // out: 64 per item, [k] = rotl64(x, k) with k a literal
    const int i = item();
    if (i >= n) return;
    rotl64_literals(x[i], out + 64 * (size_t)i, std::make_integer_sequence<int, 64>{});
}

__global__ void k_keccak_f(int n, u64* st) {  // in place, 25 words per item
    const int i = item();
    if (i >= n) return;
    u64 s[25];
    for (int k = 0; k < 25; k++) s[k] = st[25 * (size_t)i + k];
    keccak_f1600(s);
    for (int k = 0; k < 25; k++) st[25 * (size_t)i + k] = s[k];
}

// one 64-lane block per state: every lane enters keccak_f1600_wave holding the same state (as the prover's transcript kernels do)
// and writes the state it leaves with into its own 25-word slot: out[(state * 64 + lane) * 25 + k]
__global__ void k_keccak_f_wave(int n, const u64* st, u64* out) {
    const int j = (int)blockIdx.x;
    if (j >= n) return;  // uniform over the block
    u64 s[25];
    for (int k = 0; k < 25; k++) s[k] = st[25 * (size_t)j + k];
    keccak_f1600_wave(s);
    u64* o = out + 25 * ((size_t)j * 64 + threadIdx.x);
    for (int k = 0; k < 25; k++) o[k] = s[k];
}

// TranscriptRng draws as hc_merlin_rng_bulk, one transcript per item: out_generic / out_bulk get (count + 2) * 64 bytes per item,
// byte-wise STROBE fills and merlin_rng_fill64_bulk (written straight into the item's slot) respectively
__global__ void k_merlin_rng_bulk(int n, const u8* w, int w_len, const u8* ent32, int count, u8* out_generic, u8* out_bulk, i32* ok) {
    const int i = item();
    if (i >= n) return;
    const size_t slot = 64 * (size_t)(count + 2) * i;
    merlin_transcript t;
    merlin_init(t, (const uint8_t*)"BlindBidProofGadget", 19);
    merlin_transcript a = t;
    merlin_rng_rekey(a, (const uint8_t*)"v_blinding", 10, w + (size_t)w_len * i, (u32)w_len);
    merlin_rng_finalize(a, ent32 + 32 * (size_t)i);
    merlin_transcript b = a;
    for (int k = 0; k < count + 2; k++) merlin_rng_fill(a, out_generic + slot + 64 * k, 64);
    merlin_rng_fill(b, out_bulk + slot, 64);
    const bool good = merlin_rng_fill64_bulk(b, (u32)count, reinterpret_cast<u32*>(out_bulk + slot + 64));
    merlin_rng_fill(b, out_bulk + slot + 64 * (size_t)(count + 1), 64);
    ok[i] = good ? 1 : 0;
}

// ---- radix-16 scalar multiplication (csrc/scalarmul.h) -------------------------------------------------------------------------
// Points come in as Ristretto encodings and are decoded once per DISTINCT point (ok[i] = 1 when point i decoded); the tables are
// built on the device by the product's own builders; an item names its points by index.  Indices and piece ranges are checked on
// the host before anything is launched.
constexpr int STRAUS_MAX = 4;  // points per dc_straus item

__device__ __forceinline__ bool ld_point(ge& P, const u8* p32) {
    u32 w[8];
    ld_words(w, p32, 8);
    return ge_decode_words(P, w);
}
__device__ __forceinline__ sc ld_scalar(const u8* s32) {
    sc s;
    ld_words(s.v, s32, 8);
    return s;
}

// thread (b, j): column j of base b's comb, as setup.hip k_build_comb
__global__ void k_comb_tables(int nb, const u8* bases32, niels_packed* comb, i32* ok) {
    const int t = item();
    if (t >= nb * 64) return;
    const int b = t / 64, j = t % 64;
    ge P;
    const bool good = ld_point(P, bases32 + 32 * (size_t)b);
    if (j == 0) ok[b] = good ? 1 : 0;
    comb_build_column(P, (u32)j, comb + ((size_t)b * 64 + j) * 8);
}
// one lane per commitment, as prover.hip k_commit
__global__ void k_comb_one(int n, const niels_packed* comb, const u32* idx0, const u32* idx1, const u8* v32, const u8* b32, u8* out32) {
    const int i = item();
    if (i >= n) return;
    ge acc = comb_mul_add(ge_identity(), comb + (size_t)idx0[i] * 64 * 8, ld_scalar(v32 + 32 * (size_t)i));
    acc = comb_mul_add(acc, comb + (size_t)idx1[i] * 64 * 8, ld_scalar(b32 + 32 * (size_t)i));
    ge_encode(out32 + 32 * (size_t)i, acc);
}
// COMMIT_L lanes per commitment, as prover.hip k_commit_split: whole wavefronts, the last group clamped
__global__ __launch_bounds__(64) void k_comb_split(u32 n, const niels_packed* comb, const u32* idx0, const u32* idx1, const u8* v32, const u8* b32, u8* out32) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, g = t / COMMIT_L, q = t % COMMIT_L;
    const u32 gi = g < n ? g : n - 1;  // whole wavefronts reach the shuffles
    ge acc = comb_mul_add_part(ge_identity(), comb + (size_t)idx0[gi] * 64 * 8, ld_scalar(v32 + 32 * (size_t)gi), q);
    acc = comb_mul_add_part(acc, comb + (size_t)idx1[gi] * 64 * 8, ld_scalar(b32 + 32 * (size_t)gi), q);
    acc = commit_group_sum(acc);
    if (q == 0 && g < n) ge_encode(out32 + 32 * (size_t)g, acc);
}
// thread per table entry: loaded as comb_mul_add loads it, back to a point, encoded
__global__ void k_comb_unpack(int n_entries, const niels_packed* comb, u8* out32) {
    const int i = item();
    if (i >= n_entries) return;
    ge_niels e;
    BBP_COMB_LOAD(e, comb + i);
    ge_encode(out32 + 32 * (size_t)i, ge_from_niels(e));
}

// thread per point, as prover.hip k_tail_tables
__global__ void k_tail_tabs(int np, const u8* pts32, ge* tab, i32* ok) {
    const int t = item();
    if (t >= np) return;
    ge P;
    ok[t] = ld_point(P, pts32 + 32 * (size_t)t) ? 1 : 0;
    tail_table_build(P, tab + (size_t)t * TAIL_TAB);
}
__global__ void k_tail(int n, const ge* tab, const u32* pidx, const u8* s32, const i32* k_lo, const i32* k_hi, u8* out32) {
    const int i = item();
    if (i >= n) return;
    ge_encode(out32 + 32 * (size_t)i, ge_scalarmul_pieces(ld_scalar(s32 + 32 * (size_t)i), tab + (size_t)pidx[i] * TAIL_TAB, k_lo[i], k_hi[i]));
}
__global__ void k_tail_pair(int n, const ge* tab, const u32* pidx1, const u8* s1, const u32* pidx2, const u8* s2, u8* out32) {
    const int i = item();
    if (i >= n) return;
    ge_encode(out32 + 32 * (size_t)i, ge_scalarmul_pieces_pair(ld_scalar(s1 + 32 * (size_t)i), tab + (size_t)pidx1[i] * TAIL_TAB,
                                                                ld_scalar(s2 + 32 * (size_t)i), tab + (size_t)pidx2[i] * TAIL_TAB));
}

// thread per point: 1P..8P; thread per (item, slot): the digit words
__global__ void k_straus_tabs(int np, const u8* pts32, ge* tab, i32* ok) {
    const int t = item();
    if (t >= np) return;
    ge P;
    ok[t] = ld_point(P, pts32 + 32 * (size_t)t) ? 1 : 0;
    straus_table(tab + (size_t)t * 8, P);
}
__global__ void k_straus_recode(int n, const i32* cnt, const u8* s32, u32* sp) {
    const int t = item();
    if (t >= n * STRAUS_MAX) return;
    if (t % STRAUS_MAX < cnt[t / STRAUS_MAX]) straus_recode(sp + 8 * (size_t)t, ld_scalar(s32 + 32 * (size_t)t));
}
// digits 63..0 with four doublings between, as k_varbase
__global__ void k_straus_top(int n, const i32* cnt, const ge* tab, const u32* pidx, const u32* sp, u8* out32) {
    const int i = item();
    if (i >= n) return;
    ge acc = ge_identity();
    for (int j = 63; j >= 0; j--) {
        if (j != 63) {
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
            acc = ge_dbl(acc);
        }
        for (int a = 0; a < cnt[i]; a++) {
            const size_t pt = (size_t)i * STRAUS_MAX + a;
            acc = straus_digit_step(acc, tab + (size_t)pidx[pt] * 8, sp + pt * 8, j);
        }
    }
    ge_encode(out32 + 32 * (size_t)i, acc);
}
// half a wavefront per item, as k_varsum: lane l takes digits 2l + 1 and 2l of every point, 8 l doublings, then the 32-lane sum
__global__ __launch_bounds__(64) void k_straus_lanes(u32 n, const i32* cnt, const ge* tab, const u32* pidx, const u32* sp, u8* out32) {
    const u32 lane = threadIdx.x & 31u;
    const u32 i = blockIdx.x * 2 + (threadIdx.x >> 5);
    const bool live = i < n;  // (an odd n leaves the second half of the last wavefront without an item: it still takes part in the shuffles)
    ge acc = ge_identity();
    if (live) {
#pragma unroll 1
        for (int hi = 1; hi >= 0; hi--) {
            if (!hi) {
#pragma unroll 1
                for (int k = 0; k < 4; k++) acc = ge_dbl(acc);
            }
            const u32 j = 2 * lane + (u32)hi;
#pragma unroll 1
            for (int a = 0; a < cnt[i]; a++) {
                const size_t pt = (size_t)i * STRAUS_MAX + a;
                acc = straus_digit_step(acc, tab + (size_t)pidx[pt] * 8, sp + pt * 8, j);
            }
        }
#pragma unroll 1
        for (u32 k = 0; k < 8 * lane; k++) acc = ge_dbl(acc);
    }
#pragma unroll 1
    for (int d = 16; d >= 1; d >>= 1) {
        ge other;
        const u32* w = reinterpret_cast<const u32*>(&acc);
        u32* o = reinterpret_cast<u32*>(&other);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(ge) / 4); k++) o[k] = (u32)__shfl_down((int)w[k], d, 32);
        if (lane < (u32)d) acc = ge_add(acc, other);
    }
    if (live && lane == 0) ge_encode(out32 + 32 * (size_t)i, acc);
}

// ---- the engine's resident tables (bbp_debug_table): read in place, through device pointers of the same process -------------------
// thread per point of a ge array (gens, btab): encoded
__global__ void k_points_encode(int n, const ge* pts, u8* out32) {
    const int i = item();
    if (i >= n) return;
    ge_encode(out32 + 32 * (size_t)i, pts[i]);
}

// exact equality of two points in extended coordinates (not the coset equality of ge_eq: a table row is the point itself)
__device__ __forceinline__ bool same_point(const ge& p, const ge& q) {
    return fe_eq(fe_mul(p.X, q.Z), fe_mul(q.X, p.Z)) && fe_eq(fe_mul(p.Y, q.Z), fe_mul(q.Y, p.Z));
}

// one lane per base: P, 2P, .. 2^(n_pos - 1) P by ge_dbl; at each bit the row is consumed as msm.hip consumes it, load_row_at +
// ge_madd_row, in both signs, onto two accumulators: the identity (T = 0: the sum is the row's point itself, from y+x and y-x alone,
// and must be +P and -P) and P (T != 0, so the row's 2dxy takes part: P + row must be 2P, P - row the identity).  bad[i]: mismatching
// checks of base i (up to four per bit), first[i]: the first mismatching bit (n_pos when there is none)
__global__ void k_ptable_walk(int n_bases, int n_pos, const ge* gens, const niels_row* table, u32* bad, u32* first) {
    const int i = item();
    if (i >= n_bases) return;
    ge p = gens[i];
    u32 n_bad = 0, at = (u32)n_pos;
#pragma unroll 1
    for (int b = 0; b < n_pos; b++) {
        const niels_row* row = table + (size_t)i * n_pos + b;
        const row_regs rp = load_row_at(row, 0u), rm = load_row_at(row, 1u);
        const ge next = ge_dbl(p);
        const ge plus = ge_madd_row(ge_identity(), rp, false), minus = ge_madd_row(ge_identity(), rm, true);
        const ge sum = ge_madd_row(p, rp, false), diff = ge_madd_row(p, rm, true);
        const u32 miss = (same_point(plus, p) ? 0u : 1u) + (same_point(minus, ge_neg(p)) ? 0u : 1u) + (same_point(sum, next) ? 0u : 1u) +
                         (same_point(diff, ge_identity()) ? 0u : 1u);
        if (miss && at == (u32)n_pos) at = (u32)b;
        n_bad += miss;
        p = next;
    }
    bad[i] = n_bad;
    first[i] = at;
}

// thread per sampled row: identity + row and basepoint + row (an accumulator with T != 0: the row's 2dxy takes part), encoded
__global__ void k_ptable_rows(int n, const niels_row* table, const u32* row_idx, u8* out32, u8* out_b32) {
    const int i = item();
    if (i >= n) return;
    const row_regs r = load_row_at(table + row_idx[i], 0u);
    ge_encode(out32 + 32 * (size_t)i, ge_madd_row(ge_identity(), r, false));
    ge_encode(out_b32 + 32 * (size_t)i, ge_madd_row(ge_basepoint(), r, false));
}

// thread per comb entry: loaded as comb_mul_add loads it; the point from y+x and y-x, encoded, and whether the entry's third field
// is 2d x y of that point (ge_from_niels does not read it, a mixed addition onto T != 0 does)
__global__ void k_comb_entries(int n_entries, const niels_packed* comb, u8* out32, i32* xy2d_ok) {
    const int i = item();
    if (i >= n_entries) return;
    ge_niels e;
    BBP_COMB_LOAD(e, comb + i);
    const ge p = ge_from_niels(e);  // Z = 1
    ge_encode(out32 + 32 * (size_t)i, p);
    xy2d_ok[i] = fe_eq(e.xy2d, fe_mul(p.T, fe_d2())) ? 1 : 0;
}

// the 8-entry tables are indexed by digit magnitude: only canonical scalars (digits within [-8, 8]) may reach a kernel
bool all_canonical(const uint8_t* s32, size_t n) {
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        memcpy(w, s32 + 32 * i, 32);
        if (!sc_is_canonical(w)) return false;
    }
    return true;
}
bool indices_below(const u32* idx, size_t n, int bound) {
    for (size_t i = 0; i < n; i++)
        if (idx[i] >= (u32)bound) return false;
    return true;
}

}  // namespace

extern "C" {

int dc_fe_op(int op, int n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
    Call c;
    const size_t sz = 32 * (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(a32, sz);
    const u8* b = c.in<const u8>(b32, sz);
    u8* o = c.out<u8>(sz);
    c.launch(k_fe_op, blocks_for(n), BLOCK, op, n, a, b, o);
    c.back(out32, o, sz);
    return (int)c.err;
}

int dc_fe_limbs(int op, int n, const int32_t* a10, const int32_t* b10, int32_t* out10, uint8_t* out32) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0), sz = 40 * m;
    const i32* a = c.in<const i32>(a10, sz);
    const i32* b = c.in<const i32>(b10, sz);
    i32* ol = c.out<i32>(sz);
    u8* ob = c.out<u8>(32 * m);
    c.launch(k_fe_limbs, blocks_for(n), BLOCK, op, n, a, b, ol, ob);
    c.back(out10, ol, sz);
    c.back(out32, ob, 32 * m);
    return (int)c.err;
}

int dc_sc_op(int op, int n, const uint8_t* a64, const uint8_t* b32, uint8_t* out32) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(a64, 64 * m);
    const u8* b = c.in<const u8>(b32, 32 * m);
    u8* o = c.out<u8>(32 * m);
    c.launch(k_sc_op, blocks_for(n), BLOCK, op, n, a, b, o);
    c.back(out32, o, 32 * m);
    return (int)c.err;
}

int dc_sc_is_canonical(int n, const uint8_t* a32, int32_t* out) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(a32, 32 * m);
    i32* o = c.out<i32>(4 * m);
    c.launch(k_sc_is_canonical, blocks_for(n), BLOCK, n, a, o);
    c.back(out, o, 4 * m);
    return (int)c.err;
}

// pos / dig: n * 32 entries each (item i's digits at [32 i, 32 i + min(count[i], 32)))
int dc_sc_naf(int width, int n, const uint8_t* a32, int32_t* pos, int32_t* dig, int32_t* count) {
    if (width != 12 && width != 9) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(a32, 32 * m);
    i32* p = c.out<i32>(4 * NAF_SLOT * m);
    i32* d = c.out<i32>(4 * NAF_SLOT * m);
    i32* k = c.out<i32>(4 * m);
    if (width == 12) c.launch(k_sc_naf<12>, blocks_for(n), BLOCK, n, a, p, d, k);
    else c.launch(k_sc_naf<9>, blocks_for(n), BLOCK, n, a, p, d, k);
    c.back(pos, p, 4 * NAF_SLOT * m);
    c.back(dig, d, 4 * NAF_SLOT * m);
    c.back(count, k, 4 * m);
    return (int)c.err;
}

int dc_ge_op(int op, int n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32, int32_t* status) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(a32, 32 * m);
    const u8* b = c.in<const u8>(b32, 32 * m);
    u8* o = c.out<u8>(32 * m);
    i32* s = c.out<i32>(4 * m);
    c.launch(k_ge_op, blocks_for(n), BLOCK, op, n, a, b, o, s);
    c.back(out32, o, 32 * m);
    c.back(status, s, 4 * m);
    return (int)c.err;
}

int dc_from_uniform(int n, const uint8_t* in64, uint8_t* out32) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(in64, 64 * m);
    u8* o = c.out<u8>(32 * m);
    c.launch(k_from_uniform, blocks_for(n), BLOCK, n, a, o);
    c.back(out32, o, 32 * m);
    return (int)c.err;
}

int dc_madd_row(int n, const uint8_t* acc32, const uint8_t* pt32, int neg, uint8_t* out32, int32_t* status) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u8* a = c.in<const u8>(acc32, 32 * m);
    const u8* p = c.in<const u8>(pt32, 32 * m);
    niels_row* rows = c.out<niels_row>(sizeof(niels_row) * m);  // hipMalloc: at least 256-byte aligned
    u8* o = c.out<u8>(32 * m);
    i32* s = c.out<i32>(4 * m);
    c.launch(k_madd_row, blocks_for(n), BLOCK, n, a, p, (u32)(neg & 1), rows, o, s);
    c.back(out32, o, 32 * m);
    c.back(status, s, 4 * m);
    return (int)c.err;
}

int dc_rotl64(int n, const uint64_t* x, int amount, uint64_t* out) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u64* a = c.in<const u64>(x, 8 * m);
    u64* o = c.out<u64>(8 * m);
    c.launch(k_rotl64, blocks_for(n), BLOCK, n, a, amount, o);
    c.back(out, o, 8 * m);
    return (int)c.err;
}

int dc_rotl64_const(int n, const uint64_t* x, uint64_t* out64) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u64* a = c.in<const u64>(x, 8 * m);
    u64* o = c.out<u64>(8 * 64 * m);
    c.launch(k_rotl64_const, blocks_for(n), BLOCK, n, a, o);
    c.back(out64, o, 8 * 64 * m);
    return (int)c.err;
}

int dc_keccak_f(int n, uint8_t* st200) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    u64* s = c.in<u64>(st200, 200 * m);
    c.launch(k_keccak_f, blocks_for(n), BLOCK, n, s);
    c.back(st200, s, 200 * m);
    return (int)c.err;
}

// out: n * 64 * 200 bytes, the state every lane of the state's wavefront left with
int dc_keccak_f_wave(int n, const uint8_t* st200, uint8_t* out) {
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0);
    const u64* s = c.in<const u64>(st200, 200 * m);
    u64* o = c.out<u64>(200 * 64 * m);
    c.launch(k_keccak_f_wave, (u32)m, 64, n, s, o);
    c.back(out, o, 200 * 64 * m);
    return (int)c.err;
}

// w: n * w_len bytes, ent32: n * 32 bytes; out_generic / out_bulk: n * (count + 2) * 64 bytes each; ok: n flags
int dc_merlin_rng_bulk(int n, const uint8_t* w, int w_len, const uint8_t* ent32, int count, uint8_t* out_generic, uint8_t* out_bulk,
                       int32_t* ok) {
    if (count < 0 || w_len < 0) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)(n > 0 ? n : 0), per = 64 * (size_t)(count + 2);
    const u8* dw = c.in<const u8>(w, (size_t)w_len * m);
    const u8* de = c.in<const u8>(ent32, 32 * m);
    u8* g = c.out<u8>(per * m);
    u8* b = c.out<u8>(per * m);
    i32* k = c.out<i32>(4 * m);
    c.launch(k_merlin_rng_bulk, blocks_for(n), BLOCK, n, dw, w_len, de, count, g, b, k);
    c.back(out_generic, g, per * m);
    c.back(out_bulk, b, per * m);
    c.back(ok, k, 4 * m);
    return (int)c.err;
}

// ---- radix-16 scalar multiplication ------------------------------------------------------------------------------------------
// bases32: nb encodings; item i commits v[i] to base idx0[i] and b[i] to base idx1[i]: out_one32 through comb_mul_add, out_split32
// through comb_mul_add_part + commit_group_sum; base_ok: nb decode flags
int dc_comb(int nb, const uint8_t* bases32, int n, const uint32_t* idx0, const uint32_t* idx1, const uint8_t* v32, const uint8_t* b32,
            uint8_t* out_one32, uint8_t* out_split32, int32_t* base_ok) {
    if (nb <= 0 || n <= 0 || !indices_below(idx0, (size_t)n, nb) || !indices_below(idx1, (size_t)n, nb)) return (int)hipErrorInvalidValue;
    if (!all_canonical(v32, (size_t)n) || !all_canonical(b32, (size_t)n)) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)n;
    const u8* db = c.in<const u8>(bases32, 32 * (size_t)nb);
    niels_packed* comb = c.out<niels_packed>(sizeof(niels_packed) * 64 * 8 * (size_t)nb);
    i32* ok = c.out<i32>(4 * (size_t)nb);
    const u32 *i0 = c.in<const u32>(idx0, 4 * m), *i1 = c.in<const u32>(idx1, 4 * m);
    const u8 *v = c.in<const u8>(v32, 32 * m), *b = c.in<const u8>(b32, 32 * m);
    u8 *o1 = c.out<u8>(32 * m), *o2 = c.out<u8>(32 * m);
    c.launch(k_comb_tables, blocks_for(nb * 64), BLOCK, nb, db, comb, ok);
    c.launch(k_comb_one, blocks_for(n), BLOCK, n, comb, i0, i1, v, b, o1);
    c.launch(k_comb_split, blocks_for(n * COMMIT_L), 64, (u32)n, comb, i0, i1, v, b, o2);
    c.back(out_one32, o1, 32 * m);
    c.back(out_split32, o2, 32 * m);
    c.back(base_ok, ok, 4 * (size_t)nb);
    return (int)c.err;
}

// out32: nb * 64 * 8 encodings, entry [b][j][m - 1] of base b's comb as a point
int dc_comb_table(int nb, const uint8_t* bases32, uint8_t* out32, int32_t* base_ok) {
    if (nb <= 0) return (int)hipErrorInvalidValue;
    Call c;
    const size_t entries = 64 * 8 * (size_t)nb;
    const u8* db = c.in<const u8>(bases32, 32 * (size_t)nb);
    niels_packed* comb = c.out<niels_packed>(sizeof(niels_packed) * entries);
    i32* ok = c.out<i32>(4 * (size_t)nb);
    u8* o = c.out<u8>(32 * entries);
    c.launch(k_comb_tables, blocks_for(nb * 64), BLOCK, nb, db, comb, ok);
    c.launch(k_comb_unpack, blocks_for((int)entries), BLOCK, (int)entries, comb, o);
    c.back(out32, o, 32 * entries);
    c.back(base_ok, ok, 4 * (size_t)nb);
    return (int)c.err;
}

int dc_tail_pieces() { return TAIL_PIECES; }

// item i: the partial product of s[i] and point pidx[i] over pieces k_lo[i] <= k < k_hi[i] of the point's tail table
int dc_tail(int np, const uint8_t* pts32, int n, const uint32_t* pidx, const uint8_t* s32, const int32_t* k_lo, const int32_t* k_hi,
            uint8_t* out32, int32_t* pt_ok) {
    if (np <= 0 || n <= 0 || !indices_below(pidx, (size_t)n, np) || !all_canonical(s32, (size_t)n)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; i++)
        if (k_lo[i] < 0 || k_lo[i] > k_hi[i] || k_hi[i] > TAIL_PIECES) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)n;
    const u8* dp = c.in<const u8>(pts32, 32 * (size_t)np);
    ge* tab = c.out<ge>(sizeof(ge) * TAIL_TAB * (size_t)np);
    i32* ok = c.out<i32>(4 * (size_t)np);
    const u32* pi = c.in<const u32>(pidx, 4 * m);
    const u8* s = c.in<const u8>(s32, 32 * m);
    const i32 *lo = c.in<const i32>(k_lo, 4 * m), *hi = c.in<const i32>(k_hi, 4 * m);
    u8* o = c.out<u8>(32 * m);
    c.launch(k_tail_tabs, blocks_for(np), BLOCK, np, dp, tab, ok);
    c.launch(k_tail, blocks_for(n), BLOCK, n, tab, pi, s, lo, hi, o);
    c.back(out32, o, 32 * m);
    c.back(pt_ok, ok, 4 * (size_t)np);
    return (int)c.err;
}

// item i: s1[i] * point pidx1[i] + s2[i] * point pidx2[i] on one doubling chain
int dc_tail_pair(int np, const uint8_t* pts32, int n, const uint32_t* pidx1, const uint8_t* s1, const uint32_t* pidx2, const uint8_t* s2,
                 uint8_t* out32, int32_t* pt_ok) {
    if (np <= 0 || n <= 0 || !indices_below(pidx1, (size_t)n, np) || !indices_below(pidx2, (size_t)n, np)) return (int)hipErrorInvalidValue;
    if (!all_canonical(s1, (size_t)n) || !all_canonical(s2, (size_t)n)) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)n;
    const u8* dp = c.in<const u8>(pts32, 32 * (size_t)np);
    ge* tab = c.out<ge>(sizeof(ge) * TAIL_TAB * (size_t)np);
    i32* ok = c.out<i32>(4 * (size_t)np);
    const u32 *p1 = c.in<const u32>(pidx1, 4 * m), *p2 = c.in<const u32>(pidx2, 4 * m);
    const u8 *a = c.in<const u8>(s1, 32 * m), *b = c.in<const u8>(s2, 32 * m);
    u8* o = c.out<u8>(32 * m);
    c.launch(k_tail_tabs, blocks_for(np), BLOCK, np, dp, tab, ok);
    c.launch(k_tail_pair, blocks_for(n), BLOCK, n, tab, p1, a, p2, b, o);
    c.back(out32, o, 32 * m);
    c.back(pt_ok, ok, 4 * (size_t)np);
    return (int)c.err;
}

// item i: sum of s[4 i + a] * point pidx[4 i + a], a < cnt[i] <= 4: out_top32 digit by digit from the top, out_lane32 with the digits
// spread over 32 lanes; sp_out: the 8 digit words of every (item, slot) (zero for unused slots)
int dc_straus(int np, const uint8_t* pts32, int n, const int32_t* cnt, const uint32_t* pidx, const uint8_t* s32, uint8_t* out_top32,
              uint8_t* out_lane32, uint32_t* sp_out, int32_t* pt_ok) {
    if (np <= 0 || n <= 0 || !indices_below(pidx, (size_t)n * STRAUS_MAX, np) || !all_canonical(s32, (size_t)n * STRAUS_MAX)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; i++)
        if (cnt[i] < 0 || cnt[i] > STRAUS_MAX) return (int)hipErrorInvalidValue;
    Call c;
    const size_t m = (size_t)n, slots = m * STRAUS_MAX;
    const u8* dp = c.in<const u8>(pts32, 32 * (size_t)np);
    ge* tab = c.out<ge>(sizeof(ge) * 8 * (size_t)np);
    i32* ok = c.out<i32>(4 * (size_t)np);
    const i32* dc = c.in<const i32>(cnt, 4 * m);
    const u32* pi = c.in<const u32>(pidx, 4 * slots);
    const u8* s = c.in<const u8>(s32, 32 * slots);
    u32* sp = c.out<u32>(32 * slots);
    u8 *o1 = c.out<u8>(32 * m), *o2 = c.out<u8>(32 * m);
    c.launch(k_straus_tabs, blocks_for(np), BLOCK, np, dp, tab, ok);
    c.launch(k_straus_recode, blocks_for((int)slots), BLOCK, n, dc, s, sp);
    c.launch(k_straus_top, blocks_for(n), BLOCK, n, dc, tab, pi, sp, o1);
    c.launch(k_straus_lanes, (u32)((n + 1) / 2), 64, (u32)n, dc, tab, pi, sp, o2);
    c.back(out_top32, o1, 32 * m);
    c.back(out_lane32, o2, 32 * m);
    c.back(sp_out, sp, 32 * slots);
    c.back(pt_ok, ok, 4 * (size_t)np);
    return (int)c.err;
}
// ---- the engine's resident tables ---------------------------------------------------------------------------------------------
// `dev` is a device pointer of this process (bbp_debug_table) holding at least the stated number of elements; nothing is written to it
// n points of 160 bytes -> n encodings
int dc_points_encode(const void* dev, int n, uint8_t* out32) {
    if (!dev || n <= 0) return (int)hipErrorInvalidValue;
    Call c;
    u8* o = c.out<u8>(32 * (size_t)n);
    c.launch(k_points_encode, blocks_for(n), BLOCK, n, static_cast<const ge*>(dev), o);
    c.back(out32, o, 32 * (size_t)n);
    return (int)c.err;
}

// n comb entries of 96 bytes -> n encodings and n flags (k_comb_entries)
int dc_comb_entries(const void* dev, int n, uint8_t* out32, int32_t* xy2d_ok) {
    if (!dev || n <= 0) return (int)hipErrorInvalidValue;
    Call c;
    u8* o = c.out<u8>(32 * (size_t)n);
    i32* f = c.out<i32>(4 * (size_t)n);
    c.launch(k_comb_entries, blocks_for(n), BLOCK, n, static_cast<const niels_packed*>(dev), o, f);
    c.back(out32, o, 32 * (size_t)n);
    c.back(xy2d_ok, f, 4 * (size_t)n);
    return (int)c.err;
}

// gens: n_bases points in gens_bytes; table: n_bases * n_pos rows in table_bytes.  bad / first: n_bases entries each (k_ptable_walk)
int dc_ptable_walk(const void* gens_dev, uint64_t gens_bytes, const void* table_dev, uint64_t table_bytes, int n_bases, int n_pos, uint32_t* bad,
                   uint32_t* first) {
    if (!gens_dev || !table_dev || n_bases <= 0 || n_pos <= 0) return (int)hipErrorInvalidValue;
    if (sizeof(ge) * (uint64_t)n_bases > gens_bytes || sizeof(niels_row) * (uint64_t)n_bases * (uint64_t)n_pos > table_bytes) return (int)hipErrorInvalidValue;
    Call c;
    u32 *b = c.out<u32>(4 * (size_t)n_bases), *f = c.out<u32>(4 * (size_t)n_bases);
    c.launch(k_ptable_walk, blocks_for(n_bases), BLOCK, n_bases, n_pos, static_cast<const ge*>(gens_dev), static_cast<const niels_row*>(table_dev), b, f);
    c.back(bad, b, 4 * (size_t)n_bases);
    c.back(first, f, 4 * (size_t)n_bases);
    return (int)c.err;
}

// rows row_idx[0..n) of a table of n_rows rows, each added to the identity (out32) and to the basepoint (out_b32) and encoded
int dc_ptable_rows(const void* table_dev, uint64_t n_rows, int n, const uint32_t* row_idx, uint8_t* out32, uint8_t* out_b32) {
    if (!table_dev || n <= 0) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n; i++)
        if (row_idx[i] >= n_rows) return (int)hipErrorInvalidValue;
    Call c;
    const u32* ri = c.in<const u32>(row_idx, 4 * (size_t)n);
    u8 *o = c.out<u8>(32 * (size_t)n), *ob = c.out<u8>(32 * (size_t)n);
    c.launch(k_ptable_rows, blocks_for(n), BLOCK, n, static_cast<const niels_row*>(table_dev), ri, o, ob);
    c.back(out32, o, 32 * (size_t)n);
    c.back(out_b32, ob, 32 * (size_t)n);
    return (int)c.err;
}

// n words of a device array (the base-index lists)
int dc_read_u32(const void* dev, int n, uint32_t* out) {
    if (!dev || n <= 0) return (int)hipErrorInvalidValue;
    return (int)hipMemcpy(out, dev, 4 * (size_t)n, hipMemcpyDeviceToHost);
}
}
