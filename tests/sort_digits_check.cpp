// Host tier of the staged MSM sort's one-walk recoding: csrc/scalar.h's packed digits (naf_pack / naf_packed_* / sc_naf_digits_packed)
// compiled for the CPU next to the recoder they restate (sc_for_each_naf_digit), and the bounds csrc/msm_plan.h states for them.
// -> tests/_build/libsortcheck.so (tests/test_sort_digits_host.py, tests/test_gpu_sort_one_walk.py)
#include <stdint.h>
#include <string.h>

#include "../dusk_blindbidproof_amd/csrc/msm_plan.h"
#include "../dusk_blindbidproof_amd/csrc/scalar.h"

using namespace bbp;

namespace {

struct Digit {
    u32 pos, mag, neg;
};

template <int WID>
int64_t roundtrip() {
    int64_t checked = 0;
    for (u32 pos = 0; pos <= 253; pos++)
        for (u32 mag = 1; mag < (1u << (WID - 1)); mag += 2)
            for (u32 neg = 0; neg < 2; neg++) {
                const u32 p = naf_pack(pos, mag, neg);
                if (p > 0xffffu) return -1 - checked;
                if (naf_packed_pos(p, pos / 32) != pos || naf_packed_bucket(p) != (mag + 1) / 2 || naf_packed_neg(p) != neg) return -1 - checked;
                checked++;
            }
    return checked;
}

// 0: the slots of sc_naf_digits_packed hold exactly the digits sc_for_each_naf_digit calls back with, in the same order; else 1 + index
// of the first scalar that differs.  most: the most digits any of the scalars has.
template <int WID>
int compare(uint32_t n, const uint8_t* scalars, uint32_t* most) {
    constexpr int P = naf_slots<WID>::P, N = naf_slots<WID>::N;
    *most = 0;
    for (uint32_t i = 0; i < n; i++) {
        u32 s[8];
        memcpy(s, scalars + 32 * (size_t)i, 32);
        Digit want[64];
        uint32_t n_want = 0;
        sc_for_each_naf_digit<WID>(s, [&](u32 pos, u32 mag, u32 neg) {
            if (n_want < 64) want[n_want] = Digit{pos, mag, neg};
            n_want++;
        });
        u32 dig[naf_slots<WID>::WORDS], valid;
        uint32_t n_each = 0;
        bool each_ok = true;
        sc_naf_digits_packed<WID>(s, dig, valid, [&](u32 p) {  // the digits as they are found: the same ones, in order
            each_ok = each_ok && n_each < n_want && n_each < 64 && naf_packed_bucket(p) == (want[n_each].mag + 1) / 2;
            n_each++;
        });
        if (!each_ok || n_each != n_want) return 1 + (int)i;
        uint32_t got = 0;
        for (int t = 0; t < N; t++) {
            const u32 p = naf_slot<WID>(dig, t);
            if (!(valid >> t & 1)) {
                if (p != 0) return 1 + (int)i;  // an unused slot stays clear
                continue;
            }
            if (got >= n_want || got >= 64) return 1 + (int)i;
            const Digit& d = want[got++];
            if (naf_packed_pos(p, (u32)(t / P)) != d.pos || naf_packed_bucket(p) != (d.mag + 1) / 2 || naf_packed_neg(p) != d.neg) return 1 + (int)i;
        }
        if (got != n_want) return 1 + (int)i;
        if (n_want > *most) *most = n_want;
    }
    return 0;
}

}  // namespace

extern "C" {

// every (position, |digit|, sign) the width-`width` recoding can emit through the packed form and back: how many were checked, negative
// at the first that does not come back
int64_t sd_roundtrip(int width) { return width == 12 ? roundtrip<12>() : width == 9 ? roundtrip<9>() : -1; }

int sd_compare(int width, uint32_t n, const uint8_t* scalars, uint32_t* most) {
    return width == 12 ? compare<12>(n, scalars, most) : width == 9 ? compare<9>(n, scalars, most) : -1;
}

// what the kernels and the plan rely on: [0] MSM_W, [1] SMALL_W, [2] slots at width 12, [3] slots at width 9, [4] SORT_STAGED_MAX_TERMS
void sd_bounds(uint32_t* out) {
    out[0] = MSM_W, out[1] = SMALL_W, out[2] = naf_slots<12>::N, out[3] = naf_slots<9>::N, out[4] = SORT_STAGED_MAX_TERMS;
}
}
