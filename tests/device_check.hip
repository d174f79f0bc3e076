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
}
