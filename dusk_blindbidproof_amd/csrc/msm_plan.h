// Which kernels one MSM launch takes: the knobs and the plan that plan_msm decides from them.  msm.hip executes a plan; nothing else
// decides (DESIGN.md section 4 "The plan of an MSM launch").  Host-only, no HIP types: the CPU test tier compiles it too
// (tests/host_check.cpp), and the GPU tests ask it which path a shape takes (tests/msm_cases.py).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

namespace bbp {

// ---- MSM geometry (see DESIGN.md "K1") ---------------------------------------------------------------
constexpr int MSM_NAF = 12;               // scalar recoding: width-12 NAF, odd digits |d| < 2048
constexpr int MSM_W = 22;                 // most digits one scalar can have (positions >= 12 apart, last <= 253)
constexpr int MSM_K = 1 << (MSM_NAF - 2); // 1024 buckets: bucket k holds the digit magnitude 2k - 1
// Geometry of SPLIT MSMs (round 4; small batches: an MSM is cut into sub-MSMs of a few hundred terms, one workgroup each, so that a
// launch of a handful of MSMs fills the GPU): width-9 NAF digits into 128 buckets.  A sub-MSM of 128 terms has no use for 1024 buckets
// (2.5 entries each), and the bucket FOLD -- 38 dependent point additions over 1024 buckets on 128 lanes, 160 us -- is the longest
// link of a single proof's heavy chain; over 128 buckets it is 21.  More additions per term (25.6 against 19.85) in an accumulate
// launch that takes 40 us.
constexpr int SMALL_NAF = 9;
constexpr int SMALL_K = 1 << (SMALL_NAF - 2);  // 128
constexpr int SMALL_W = 29;                    // most digits one scalar can have at width 9 (context.h FOLD_W: the same recoding)

// The staged sort's LDS image (msm.hip k_msm_sort_staged), in entries of 4 bytes
#ifndef BBP_SORT_CAP
#define BBP_SORT_CAP 21504  // two windows for a 2049-term MSM (40.7 k entries), three for 2933 terms; 16 384 (three / four, two workgroups per CU) measured 0.5 % slower per batch
#endif
constexpr uint32_t SORT_CAP_WIDE = 32768;  // ... of MSMs with more than SORT_WIDE_FROM terms (one workgroup per CU then)
constexpr uint32_t SORT_WIDE_FROM = 3000;
constexpr uint32_t SORT_STAGED_MAX_TERMS = 5120;  // the staged sort keeps every digit in registers, at most five scalars on each of its 1024 lanes: longer (sub-)MSMs take the plain scatter (the API's longest MSM has 4098 terms)
constexpr uint32_t MSM_SPLIT_MAX = 16;     // sub-MSMs per MSM at the most (k_msm_reduce: sixteen lanes per output)

struct MsmKnobs {
    int sort_staged = 3;          // BBP_SORT_STAGED (0..7): bit 0: generic MSMs, bit 1: the generator-fold pass sort with the scatter staged through LDS, bit 2: MSMs wider than SORT_WIDE_FROM too (128 KB image)
    int fold_half_from = 512;     // BBP_FOLD_HALF_FROM (>= 1): launches with at least this many MSMs fold on half a wavefront per MSM (k_msm_fold_half)
    int msm_small = 1;            // BBP_MSM_SMALL: split MSMs use width-9 digits and 128 buckets (msm_geom<2>); 0: 1024 like the others
    uint32_t split_below = 128;   // BBP_MSM_SPLIT_BELOW: launches with fewer MSMs than this are split ...
    uint32_t split_target = 512;  // BBP_MSM_SPLIT_TARGET: ... into about this many workgroups

    // one knob from its environment text, clamped; false: the name is no MSM knob
    bool set(const char* name, const char* text) {
        const int v = atoi(text);
        if (!strcmp(name, "BBP_SORT_STAGED")) sort_staged = v & 7;
        else if (!strcmp(name, "BBP_FOLD_HALF_FROM")) fold_half_from = v < 1 ? 1 : v;
        else if (!strcmp(name, "BBP_MSM_SMALL")) msm_small = v != 0;
        else if (!strcmp(name, "BBP_MSM_SPLIT_BELOW")) split_below = (uint32_t)v;
        else if (!strcmp(name, "BBP_MSM_SPLIT_TARGET")) split_target = (uint32_t)v;
        else return false;
        return true;
    }
    // the two split knobs belong to the process (callers without a context size scratch by them: msm_scratch_bytes): read once
    static const MsmKnobs& process() {
        static const MsmKnobs once = [] {
            MsmKnobs k;
            for (const char* name : {"BBP_MSM_SPLIT_BELOW", "BBP_MSM_SPLIT_TARGET"})
                if (const char* text = getenv(name)) k.set(name, text);
            return k;
        }();
        return once;
    }
    // a context's knobs: the process's split knobs, the others as the environment has them now
    static MsmKnobs from_env() {
        MsmKnobs k = process();
        for (const char* name : {"BBP_SORT_STAGED", "BBP_FOLD_HALF_FROM", "BBP_MSM_SMALL"})
            if (const char* text = getenv(name)) k.set(name, text);
        return k;
    }
};

// how many workgroups an MSM of n terms is cut into when the launch has only n_msm of them (fills the GPU for small batches).
// Every sub-MSM pays a bucket fold of its own (k_msm_fold), so splitting only pays while the GPU would otherwise be mostly empty.
inline uint32_t msm_split(const MsmKnobs& k, uint32_t n_msm, uint32_t n_terms) {
    if (n_msm >= k.split_below) return 1;
    uint32_t s = k.split_target / n_msm;
    if (s > MSM_SPLIT_MAX) s = MSM_SPLIT_MAX;
    while (s > 1 && n_terms / s < 128) s--;
    return s ? s : 1;
}
inline uint32_t msm_split(uint32_t n_msm, uint32_t n_terms) { return msm_split(MsmKnobs::process(), n_msm, n_terms); }

struct MsmPlan {
    enum Geom { LARGE, SMALL };               // msm_geom<0>: width-12 digits, 1024 buckets | msm_geom<2>: width 9, 128 buckets
    enum Sort { PLAIN, STAGED, STAGED_WIDE };  // k_msm_sort | k_msm_sort_staged with the ordinary image | ... with the 128 KB image
    enum Fold { LANES128, HALF, SMALL_FOLD };  // k_msm_fold<0> | k_msm_fold_half | k_msm_fold<2>
    uint32_t split = 1;     // sub-MSMs per MSM
    uint32_t n_sub = 0;     // terms of a sub-MSM (the last one of an MSM may have fewer)
    uint32_t n_work = 0;    // workgroups of the sort and fold launches: n_msm * split
    Geom geom = LARGE;
    Sort sort = PLAIN;
    uint32_t sort_cap = 0;  // entries of the staged sort's image; 0: plain scatter
    Fold fold = LANES128;
    bool reduce = false;    // k_msm_reduce sums the sub-MSMs' results

    uint32_t K() const { return geom == SMALL ? SMALL_K : MSM_K; }  // buckets
    uint32_t W() const { return geom == SMALL ? SMALL_W : MSM_W; }  // sorted entries reserved per term
    uint32_t naf() const { return geom == SMALL ? SMALL_NAF : MSM_NAF; }
};

// The one place that decides.  device_sized: n_msm is only the upper bound of how many MSMs there are (the count lives on the
// device); such launches are never split.
inline MsmPlan plan_msm(const MsmKnobs& k, uint32_t n_msm, uint32_t n_terms, bool device_sized) {
    MsmPlan p;
    p.split = device_sized ? 1u : msm_split(k, n_msm, n_terms);
    p.n_sub = (n_terms + p.split - 1) / p.split;
    p.n_work = n_msm * p.split;
    p.reduce = p.split > 1;
    if (p.split > 1 && k.msm_small) {  // BBP_MSM_SMALL=0: split MSMs keep the 1024-bucket geometry
        p.geom = MsmPlan::SMALL;
        p.fold = MsmPlan::SMALL_FOLD;
        return p;
    }
    // staged scatter: 84 KB image for the prover's 2049- / 2933-term MSMs (two / three windows); wider MSMs (the verifier's 4098
    // terms = 81 k entries) get a 128 KB image with bit 2 of the knob.  With the re-walking sort that form measured 3 % slower than
    // the plain scatter; with the one-walk sort it measures FASTER (bench.py --workload verify, knob 3 against 7 alternated, five
    // runs each, profiles/r16_sort_ab_verify*.jsonl): 8192 proofs 210.5-212.1 k -> 219.0-220.0 k verifications/s (x 1.034, ranges
    // apart), 1024 proofs 180.1-190.0 k -> 188.3-195.0 k (medians x 1.031, ranges overlap).  The default stays 3 for now: the
    // path tests pin the plain scatter as the default plan of the 4097-term launches, and prove batches at N >= 20 would move too
    // and have not been measured.
    const bool wide = p.n_sub > SORT_WIDE_FROM;
    if ((k.sort_staged & 1) && (!wide || (k.sort_staged & 4)) && p.n_sub <= SORT_STAGED_MAX_TERMS) {
        p.sort = wide ? MsmPlan::STAGED_WIDE : MsmPlan::STAGED;
        p.sort_cap = wide ? SORT_CAP_WIDE : (uint32_t)BBP_SORT_CAP;
    }
    // many MSMs: the fold on half a wavefront per MSM (fewer wave-instructions); few: the 128-lane fold (shorter chain)
    p.fold = p.n_work >= (uint32_t)k.fold_half_from ? MsmPlan::HALF : MsmPlan::LANES128;
    return p;
}

}  // namespace bbp
