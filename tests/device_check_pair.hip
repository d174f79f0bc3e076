// tests only: the pair form of Keccak-f[1600] (csrc/keccak.h keccak_f1600_pair: two adjacent lanes per state, half a state each) as
// hipcc compiles it for gfx950, behind one C entry point in the manner of tests/device_check.hip's dc_keccak_f.  A library of its own so
// that device_check.hip and its two builds stay as they are.
//
// Allocate, copy in, launch ONE kernel on the default stream, synchronise, copy out, free; the return value is the first hipError_t
// met (0 = hipSuccess).  Every lane loads and stores only the 25 words of its own half of its own state: a wrong kernel gives a wrong
// answer, never an out-of-bounds access.
#include <hip/hip_runtime.h>

#include "../dusk_blindbidproof_amd/csrc/keccak.h"

using namespace bbp;

namespace {

// lanes 2p and 2p + 1 have state p: both are live or both return, so the partner reads of a live pair always find an active lane
__global__ void k_keccak_f_pair(int n, u32* st) {  // in place, 50 words per state: word 2i low, word 2i + 1 high
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, p = t >> 1, odd = t & 1u;
    if (p >= (u32)n) return;
    u32* s = st + 50 * (size_t)p + odd;
    u32 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = s[2 * i];
    keccak_f1600_pair(a, odd ? ~0u : 0u);
#pragma unroll
    for (int i = 0; i < 25; i++) s[2 * i] = a[i];
}

}  // namespace

extern "C" int dc_keccak_f_pair(int n, uint8_t* st200) {
    if (n <= 0) return 0;
    const size_t bytes = 200 * (size_t)n;
    u32* d = nullptr;
    hipError_t err = hipMalloc(&d, bytes);
    if (err != hipSuccess) return (int)err;
    err = hipMemcpy(d, st200, bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_keccak_f_pair, dim3((2 * (u32)n + 63) / 64), dim3(64), 0, 0, n, d);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(st200, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return (int)err;
}
