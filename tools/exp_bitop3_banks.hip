// Experiment (GPU box): what a LONE wavefront pays for v_bitop3_b32 with three VGPR sources, by where the sources sit -- the one-lane
// Keccak round (csrc/keccak.h) is 120 of them, and its chain ran at 5.5 cycles per instruction where tools/exp_wave_latency.hip
// prices one at 5.1.  Registers are named in the asm text, so the register numbers are what is measured: sources numbered
// 1, 2, 3 mod 4; two of them equal mod 4; all three equal mod 4; and one source register used twice.  Four independent
// instructions per step (no result is read again inside a step), as in the round, whose compiled loop has two dependent pairs.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/exp_bitop3_banks.hip -o /tmp/exp_bitop3_banks && /tmp/exp_bitop3_banks
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef unsigned int u32;

#define REP4(x) x x x x
#define REP32(x) REP4(REP4(x)) REP4(REP4(x))
#define CLOBBERS "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59"
#define SEED_REGS                                                                                                               \
    "v_mov_b32 v41, %1\n v_mov_b32 v42, %2\n v_mov_b32 v43, %1\n v_mov_b32 v45, %2\n v_mov_b32 v46, %1\n v_mov_b32 v47, %2\n"  \
    "v_mov_b32 v49, %1\n v_mov_b32 v50, %2\n v_mov_b32 v51, %1\n v_mov_b32 v53, %2\n v_mov_b32 v54, %1\n v_mov_b32 v55, %2\n"  \
    "v_mov_b32 v57, %1\n v_mov_b32 v58, %2\n v_mov_b32 v59, %1\n"

#define KERNEL(name, STEP)                                                                          \
    __global__ void name(u32* out, u32 iters, u32 seed) {                                           \
        u32 a = seed ^ threadIdx.x, b = seed * 3u + threadIdx.x, r = 0;                             \
        asm volatile(SEED_REGS : "+v"(r) : "v"(a), "v"(b) : CLOBBERS);                              \
        for (u32 i = 0; i < iters; i++) { asm volatile(REP32(STEP) : "+v"(r) : : CLOBBERS); }       \
        asm volatile("v_bitop3_b32 %0, v40, v44, v48 bitop3:0x96\n v_xor_b32 %0, %0, v52\n" : "+v"(r) : : CLOBBERS); \
        if (r == 0x12345u) out[0] = r;                                                              \
    }

// destinations v40, v44, v48, v52 throughout; only the sources move
KERNEL(k_src_mod4_123, "v_bitop3_b32 v40, v41, v42, v43 bitop3:0x96\n v_bitop3_b32 v44, v45, v46, v47 bitop3:0x96\n"
                       "v_bitop3_b32 v48, v49, v50, v51 bitop3:0x96\n v_bitop3_b32 v52, v53, v54, v55 bitop3:0x96\n")
KERNEL(k_src_mod4_112, "v_bitop3_b32 v40, v41, v45, v42 bitop3:0x96\n v_bitop3_b32 v44, v45, v49, v46 bitop3:0x96\n"
                       "v_bitop3_b32 v48, v49, v53, v50 bitop3:0x96\n v_bitop3_b32 v52, v53, v57, v54 bitop3:0x96\n")
KERNEL(k_src_mod4_111, "v_bitop3_b32 v40, v41, v45, v49 bitop3:0x96\n v_bitop3_b32 v44, v45, v49, v53 bitop3:0x96\n"
                       "v_bitop3_b32 v48, v49, v53, v57 bitop3:0x96\n v_bitop3_b32 v52, v53, v57, v41 bitop3:0x96\n")
KERNEL(k_src_same_reg, "v_bitop3_b32 v40, v41, v41, v42 bitop3:0x96\n v_bitop3_b32 v44, v45, v45, v46 bitop3:0x96\n"
                       "v_bitop3_b32 v48, v49, v49, v50 bitop3:0x96\n v_bitop3_b32 v52, v53, v53, v54 bitop3:0x96\n")
KERNEL(k_xor_mod4_12, "v_xor_b32 v40, v41, v42\n v_xor_b32 v44, v45, v46\n v_xor_b32 v48, v49, v50\n v_xor_b32 v52, v53, v54\n")
KERNEL(k_xor_mod4_11, "v_xor_b32 v40, v41, v45\n v_xor_b32 v44, v45, v49\n v_xor_b32 v48, v49, v53\n v_xor_b32 v52, v53, v57\n")
KERNEL(k_alignbit_mod4_12, "v_alignbit_b32 v40, v41, v42, 7\n v_alignbit_b32 v44, v45, v46, 7\n v_alignbit_b32 v48, v49, v50, 7\n v_alignbit_b32 v52, v53, v54, 7\n")
KERNEL(k_alignbit_mod4_11, "v_alignbit_b32 v40, v41, v45, 7\n v_alignbit_b32 v44, v45, v49, 7\n v_alignbit_b32 v48, v49, v53, 7\n v_alignbit_b32 v52, v53, v57, 7\n")

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)

template <typename K> static int run(const char* name, K k, u32* d, double ghz) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const u32 iters = 20000;
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d, 100u, 7u);
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d, iters, 7u);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    const double ns = ms * 1e6 / (32.0 * 4.0 * iters);
    printf("%-20s %6.3f ns per instruction = %5.2f cycles\n", name, ns, ns * ghz);
    return 0;
}

int main() {
    u32* d;
    CK(hipMalloc(&d, 64));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    const double ghz = p.clockRate / 1e6;
    printf("device clock %.2f GHz\n", ghz);
#define RUN(k) if (run(#k, k, d, ghz)) return 2;
    RUN(k_src_mod4_123) RUN(k_src_mod4_112) RUN(k_src_mod4_111) RUN(k_src_same_reg)
    RUN(k_xor_mod4_12) RUN(k_xor_mod4_11) RUN(k_alignbit_mod4_12) RUN(k_alignbit_mod4_11)
    return 0;
}
