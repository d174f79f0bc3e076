// How one prove call is scheduled: the knobs, the state the rules carry from call to call, and the plan that plan_prove decides
// from them.  prover.hip executes a plan; nothing else decides (DESIGN.md section 4 "The plan of a prove call", where the
// measurements behind each rule are).  Host-only, no HIP types: the CPU test tier compiles it too (tests/host_check.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

namespace bbp {

constexpr int FOLD_ROUND = 7;  // first IPA round on explicit folded generators: vectors of length 32 (context.h "IPA tail")
constexpr int PROVE_MAX_SLICES = 4;  // heavy-stage slices of one call, one stream each (slice 0 = the caller's stream)
#ifndef BBP_PROVE_BUFS
#define BBP_PROVE_BUFS 5
#endif
constexpr int PROVE_BUFS = BBP_PROVE_BUFS;  // batch buffers: a dual-opening call uses buffer call % PROVE_BUFS, any other call & 1
// -DBBP_SERIAL_PAIR=0 (experiment): the whole-chain form of k_open_serial on one lane per proof, as before round 27.  Shipped: two
// adjacent lanes per proof, half a Keccak state each (keccak.h "pair form").
#ifndef BBP_SERIAL_PAIR
#define BBP_SERIAL_PAIR 1
#endif
constexpr uint32_t SERIAL_CHAIN_LANES = BBP_SERIAL_PAIR ? 2 : 1;  // lanes per proof of the whole serial draw chain

struct ProveKnobs {
    int slices = 3;                   // BBP_SLICES (1..4): heavy-stage slices of a call that is not rotated
    int rotate_below = 1023;          // BBP_ROTATE_BELOW: calls of at most this many proofs run their heavy stage unsliced on a rotating internal stream; 0 = never
    int rotate_deep_max = 4096;       // BBP_ROTATE_DEEP_MAX: ... and calls up to this size while the caller is in deep mode; 0 = never (never with BBP_SLICES=1)
    int deep_from = 3;                // BBP_ROTATE_DEEP_FROM (>= 2): earlier prove calls in flight that put the caller in deep mode
    int mixed_from = 512;             // BBP_ROTATE_MIXED_FROM: a call of at least this many proofs that finds a sliced heavy stage in flight is sliced too; 0 = never
    int dual_open_below = 1024;       // BBP_DUAL_OPEN_BELOW: calls smaller than this open on alternating streams; 0 = never
    int rng_coop = -1;                // BBP_RNG_COOP: 0 / 1 forces the single-lane / cooperative draw chain; unset (-1) = by size:
    int rng_coop_below = 768;         // BBP_RNG_COOP_BELOW: cooperative up to this many proofs
    int rng_coop_idle_below = 2300;   // BBP_RNG_COOP_IDLE_BELOW: ... and up to this many when no earlier prove call is in flight; 0 = never
    int rng_dpp = 2;                  // BBP_RNG_DPP: cooperative chain 2 = half-word per lane (k_open_bulk50), 1 = word per lane (k_open_bulk8), 0 = 25 lanes (k_open_bulk)
    int rng_block = 0;                // BBP_RNG_BLOCK (64..1024, power of two): threads per cooperative workgroup; 0 = by size: 64 up to 128 proofs, 128 up to 256, 256 above
    int serial_block = 64;            // BBP_SERIAL_BLOCK (64, 128 or 256): PROOFS per workgroup of the serial opening kernels.  The whole draw chain puts
                                      // SERIAL_CHAIN_LANES lanes on a proof (ProvePlan::serial_chain_lanes()), so by default its workgroup is 128 lanes = two
                                      // wavefronts, which a CU places on two SIMDs: a lone wavefront each, as before, and a 1024-proof call still fences
                                      // 16 CUs (8 / 16 / 32 fenced CUs measured alike).  Counting lanes would have fenced 32.
    int serial_lds = 160 * 1024;      // BBP_SERIAL_LDS (0..160 KiB): LDS those kernels reserve to keep their CU to themselves; 0 = off
    int tr_wave_below = 32;           // BBP_TR_WAVE_BELOW: launches of at most this many proofs run the transcript kernels one proof per wavefront; 0 = never
    int ipa_wide_below = 32;          // BBP_IPA_WIDE_BELOW: launches of at most this many proofs run k_ipa_round on 1024 lanes per proof; 0 = never
    int commit_split_below = 1024;    // BBP_COMMIT_SPLIT_BELOW: commitment launches of at most this many commitments put each on eight lanes; 0 = never
    int witness_native = 1;           // BBP_WITNESS_NATIVE: 0 = the cooperative opening launches interpret the compiled gadget program
    int tail_small_below = 65;        // BBP_TAIL_SMALL_BELOW: heavy stages of fewer proofs keep all eleven IPA rounds on the fixed-base MSM kernels; 0 = never
    int tail_round = FOLD_ROUND;      // BBP_TAIL_ROUND: first IPA round on folded generators; anything but FOLD_ROUND = 12 = none
    int stagger_mode = 0;             // BBP_STAGGER: 0 = slices start together, 1 / 3 = the next slice starts after this slice's first / third MSM
    int trace_prove = 0;              // BBP_TRACE_PROVE (present = on): one stderr line per prove call with its plan
    int open_on_chain = -1;           // BBP_OPEN_ON_CHAIN: a rotating call's opening stage runs on the stream of its heavy stage: 0 never, 1 every rotating call, unset (-1) = the calls of a deep pipeline, by hw_queues
    int hw_queues = 4;                // no environment name of its own: the hardware queues the process's HIP runtime was given, filled in by bbp_init (HIP's default)
    int blinding_draw = 0;            // no environment name: the context's bbp_set_blinding_draw setting (include/bbp.h), 0 = MERLIN, 1 = EXPANDED

    // the one list of environment names; a null clamp takes the number as it is
    struct Env {
        const char* name;
        int ProveKnobs::*member;
        int (*clamp)(int);
    };
    template <class F>
    static void each_env(F&& f) {
        static const Env table[] = {
            {"BBP_SLICES", &ProveKnobs::slices, [](int v) { return v < 1 ? 1 : v > PROVE_MAX_SLICES ? PROVE_MAX_SLICES : v; }},
            {"BBP_ROTATE_BELOW", &ProveKnobs::rotate_below, nullptr},
            {"BBP_ROTATE_DEEP_MAX", &ProveKnobs::rotate_deep_max, nullptr},
            {"BBP_ROTATE_DEEP_FROM", &ProveKnobs::deep_from, [](int v) { return v < 2 ? 2 : v; }},
            {"BBP_ROTATE_MIXED_FROM", &ProveKnobs::mixed_from, nullptr},
            {"BBP_DUAL_OPEN_BELOW", &ProveKnobs::dual_open_below, nullptr},
            {"BBP_RNG_COOP", &ProveKnobs::rng_coop, [](int v) { return v != 0 ? 1 : 0; }},
            {"BBP_RNG_COOP_BELOW", &ProveKnobs::rng_coop_below, nullptr},
            {"BBP_RNG_COOP_IDLE_BELOW", &ProveKnobs::rng_coop_idle_below, nullptr},
            {"BBP_RNG_DPP", &ProveKnobs::rng_dpp, nullptr},
            {"BBP_RNG_BLOCK", &ProveKnobs::rng_block, [](int v) { return v >= 1024 ? 1024 : v >= 512 ? 512 : v >= 256 ? 256 : v >= 128 ? 128 : 64; }},
            {"BBP_SERIAL_BLOCK", &ProveKnobs::serial_block, [](int v) { return v == 64 ? 64 : v == 128 ? 128 : 256; }},
            {"BBP_SERIAL_LDS", &ProveKnobs::serial_lds, [](int v) { return v < 0 ? 0 : v > 160 * 1024 ? 160 * 1024 : v; }},
            {"BBP_TR_WAVE_BELOW", &ProveKnobs::tr_wave_below, nullptr},
            {"BBP_IPA_WIDE_BELOW", &ProveKnobs::ipa_wide_below, nullptr},
            {"BBP_COMMIT_SPLIT_BELOW", &ProveKnobs::commit_split_below, nullptr},
            {"BBP_WITNESS_NATIVE", &ProveKnobs::witness_native, [](int v) { return v != 0 ? 1 : 0; }},
            {"BBP_TAIL_SMALL_BELOW", &ProveKnobs::tail_small_below, nullptr},
            {"BBP_TAIL_ROUND", &ProveKnobs::tail_round, [](int v) { return v == FOLD_ROUND ? FOLD_ROUND : 12; }},
            {"BBP_STAGGER", &ProveKnobs::stagger_mode, nullptr},
            {"BBP_TRACE_PROVE", &ProveKnobs::trace_prove, [](int) { return 1; }},
            {"BBP_OPEN_ON_CHAIN", &ProveKnobs::open_on_chain, [](int v) { return v < 0 ? -1 : v ? 1 : 0; }},
        };
        for (const Env& e : table) f(e);
    }
    // one knob from its environment text, clamped; false: the name is no prove knob
    bool set(const char* name, const char* text) {
        bool found = false;
        each_env([&](const Env& e) {
            if (strcmp(e.name, name)) return;
            this->*e.member = e.clamp ? e.clamp(atoi(text)) : atoi(text);
            found = true;
        });
        return found;
    }
    static ProveKnobs from_env() {
        ProveKnobs k;
        each_env([&](const Env& e) {
            if (const char* text = getenv(e.name)) k.set(e.name, text);
        });
        return k;
    }

    // a call of B proofs may take the rotating path in deep mode
    bool deep_eligible(uint32_t B) const { return slices > 1 && rotate_deep_max > 0 && B <= (uint32_t)rotate_deep_max; }
    // a rotating call runs as one chain, opening stage and heavy stage on one stream: with fewer than seven hardware queues the five
    // internal streams that a deep pipeline keeps busy in the two-stream form (side, side2, lane[1..3]) cannot all have a queue apart
    // from the caller's stream's.  Unset, the rule holds for calls planned `deep` only: a caller that mixes rotating and sliced calls
    // without being in deep mode (two host threads) would find every third chain on side, where its sliced calls open
    bool chain_rule(bool deep) const { return open_on_chain == 1 || (open_on_chain < 0 && deep && hw_queues < 7); }
    // launches that must stay off the CUs the serial opening kernels reserve carry a token 64 bytes of LDS (prover.hip "LAUNCH")
    unsigned lds_token() const { return serial_lds >= 160 * 1024 ? 64u : 0u; }
};

// What the rules remember between the prove calls of one context.
struct ProveRuleState {
    bool deep_mode = false;   // the caller keeps deep_from or more calls in flight: entered at once, left after six calls in a row that found fewer
    int deep_idle_seen = 0;   // ... how many of those in a row so far
    bool force_deep = false;  // bbp_reserve warming the rotating path's buffers: deep for this call, the hysteresis untouched
    bool last_sliced = false; // the last prove call's heavy stage ran as slices on the caller's stream + lanes
    uint32_t calls = 0;       // prove calls planned so far: the next call's index
};

// A heavy stage of B proofs: a rotated call, or one slice.
struct HeavyPlan {
    uint32_t tw = 0;         // 1: the transcript kernels run one proof per wavefront
    uint32_t tgrid = 0;      // ... and their grid
    bool wide_ipa = false;   // k_ipa_round on 1024 lanes per proof, k_flatten_split
    bool split_T = false;    // k_commit_T_split
    uint32_t tail_from = 12; // first IPA round on folded generators; 12 = none
    int stagger_after = 0;   // the stagger event is recorded after this stage's first (1) or third (3) MSM
};

inline HeavyPlan plan_heavy(const ProveKnobs& k, uint32_t B) {
    HeavyPlan h;
    h.tw = B <= (uint32_t)k.tr_wave_below ? 1u : 0u;
    h.tgrid = h.tw ? B : (B + 63) / 64;
    h.wide_ipa = B <= (uint32_t)k.ipa_wide_below;
    h.split_T = B * 5 <= (uint32_t)k.commit_split_below;
    h.tail_from = B < (uint32_t)(k.tail_small_below > 0 ? k.tail_small_below : 0) ? 12u : (uint32_t)k.tail_round;
    h.stagger_after = k.stagger_mode;
    return h;
}

// The streams of a context by role, in the order bbp_init creates them (hardware queues are handed out in that order).
enum StreamRole { ROLE_CALLER = 0, ROLE_SIDE, ROLE_LANE1, ROLE_LANE2, ROLE_LANE3, ROLE_COPY, ROLE_SIDE2, ROLE_COUNT };

struct ProvePlan {
    // the draw chain: k_open_serial alone | k_open_bulk | k_open_bulk8 | k_open_bulk50 | none: k_open_key, k_expand_draws, k_witness_gates
    // (bbp_set_blinding_draw(EXPANDED): coop, serial_blk, cblk and the rng_coop* knobs then play no part, and prefix_form is k_open_key's:
    // 2 = a wavefront per proof up to tr_wave_below proofs, 1 = a lane per proof)
    enum Chain { SERIAL, LANES25, WORD, HALFWORD, EXPANDED };
    uint32_t call = 0;           // this call's index
    bool deep = false;           // taken as a call of a caller in deep mode
    bool behind_sliced = false;  // not small, and the last call's slices are still on the device: sliced and stream-ordered behind them
    bool dual = false;           // opens on alternating streams, over all PROVE_BUFS buffers
    int open_stream = 0;         // 0: side, 1: side2
    int par = 0;                 // batch buffer
    bool coop = false;           // the draw chain runs on a wavefront (or half of one) per proof
    Chain chain = SERIAL;
    uint32_t prefix_form = 0;    // k_open_serial's last argument: 0 the whole chain, 1 / 2 the prefix of a cooperative chain on a lane / a wavefront per proof
    uint32_t serial_blk = 64;    // proofs per workgroup of the serial chain (and its witness workgroups); its lanes: serial_chain_lanes()
    uint32_t cblk = 64;          // workgroup of k_open_bulk; the wavefront-per-proof chains take cblk_wave()
    bool rotate = false;         // the heavy stage runs unsliced on lane[heavy_stream]
    int heavy_stream = 0;
    uint32_t slices = 0;         // 0 when rotating
    bool open_on_chain = false;  // rotating, and the opening stage runs on the heavy stage's stream: the call is one chain
    int chain_stream = -1;       // ... the role of that stream: heavy_stream 1 -> ROLE_LANE1, 2 -> ROLE_LANE2, 3 -> ROLE_SIDE; -1 otherwise

    // the stream the opening stage runs on, the one the rotated heavy stage runs on, the one slice i runs on
    int open_role() const { return open_on_chain ? chain_stream : open_stream ? ROLE_SIDE2 : ROLE_SIDE; }
    int heavy_role() const { return open_on_chain ? chain_stream : ROLE_LANE1 + heavy_stream - 1; }
    static int slice_role(uint32_t i) { return i == 0 ? ROLE_CALLER : ROLE_LANE1 + (int)i - 1; }
    // every stream the call enqueues on, as a mask of 1 << role (the caller's stream always: entry, join and completion events)
    uint32_t roles() const {
        uint32_t mask = 1u << ROLE_CALLER | 1u << open_role();
        if (rotate) mask |= 1u << heavy_role();
        for (uint32_t i = 0; i < slices; i++) mask |= 1u << slice_role(i);
        return mask;
    }
    // the draw buffer (bbp_ctx::raw) of the opening stage: one per stream that opens, so that stream order alone guards it
    int raw_index() const { return !open_on_chain ? open_stream : chain_stream == ROLE_SIDE ? 0 : 1 + heavy_stream; }
    // ... and its bytes for B proofs of n1 multipliers: every raw 64-byte draw, or under EXPANDED one 32-byte key per proof
    size_t raw_bytes(uint32_t B, uint32_t n1) const { return chain == EXPANDED ? (size_t)32 * B : (size_t)64 * B * (3 + 2 * (size_t)n1); }
    uint32_t cblk_wave() const { return 2 * cblk > 1024u ? 1024u : 2 * cblk; }
    uint32_t serial_chain_lanes() const { return SERIAL_CHAIN_LANES * serial_blk; }  // threads per workgroup of the whole-chain launch (at most 512)
    // slice i of a call of B proofs is [slice_first(B, i), slice_first(B, i + 1))
    uint32_t slice_first(uint32_t B, uint32_t i) const { return (uint32_t)(((uint64_t)B * i) / slices); }

    std::string trace_line(uint32_t call_, uint32_t B, int inflight) const {
        char buf[176];
        snprintf(buf, sizeof buf, "prove call %u: B %u inflight %d deep %d behind_sliced %d dual %d rotate %d par %d coop %d%s\n", call_, B, inflight,
                 (int)deep, (int)behind_sliced, (int)dual, (int)rotate, par, (int)coop, chain == EXPANDED ? " draw expanded" : "");
        return buf;
    }
};

// The one place that decides.  inflight: earlier prove calls still on the device.  sliced_busy(): whether the last call's heavy
// stage is; asked only of a call that the answer can move (a HIP query in the driver).  Advances `st` but for last_sliced, which the
// driver sets to !rotate once the call is enqueued.
template <class Busy>
ProvePlan plan_prove(const ProveKnobs& k, ProveRuleState& st, uint32_t B, int inflight, Busy&& sliced_busy) {
    ProvePlan p;
    p.call = st.calls++;
    if (inflight >= k.deep_from) {
        st.deep_mode = true;
        st.deep_idle_seen = 0;
    } else if (++st.deep_idle_seen >= 6) {
        st.deep_mode = false;
    }
    p.deep = (st.deep_mode || st.force_deep) && k.deep_eligible(B);
    p.behind_sliced = !p.deep && k.mixed_from > 0 && B >= (uint32_t)k.mixed_from && st.last_sliced && sliced_busy();
    p.dual = !p.behind_sliced && (p.deep || B < (uint32_t)(k.dual_open_below > 0 ? k.dual_open_below : 0));
    p.open_stream = p.dual ? (int)(p.call & 1u) : 0;
    p.par = p.dual ? (int)(p.call % (uint32_t)PROVE_BUFS) : (int)(p.call & 1u);
    p.coop = k.rng_coop < 0 ? B <= (uint32_t)k.rng_coop_below || (inflight == 0 && B <= (uint32_t)k.rng_coop_idle_below) : k.rng_coop != 0;
    p.chain = !p.coop ? ProvePlan::SERIAL : k.rng_dpp >= 2 ? ProvePlan::HALFWORD : k.rng_dpp ? ProvePlan::WORD : ProvePlan::LANES25;
    p.prefix_form = !p.coop ? 0u : B <= (uint32_t)k.tr_wave_below ? 2u : 1u;
    p.serial_blk = k.serial_lds > 0 ? (uint32_t)k.serial_block : 64u;
    p.cblk = k.rng_block > 0 ? (uint32_t)k.rng_block : (B <= 128 ? 64u : B <= 256 ? 128u : 256u);
    p.rotate = p.dual && ((k.rotate_below > 0 && B <= (uint32_t)k.rotate_below) || (p.deep && B > (uint32_t)k.rotate_below));
    p.heavy_stream = p.rotate ? 1 + (int)(p.call % (uint32_t)(PROVE_MAX_SLICES - 1)) : 0;
    p.slices = B >= 64u * (uint32_t)k.slices ? (uint32_t)k.slices : (B >= 128 ? 2u : 1u);
    if (p.dual && p.slices > 2) p.slices = 2;
    if (p.rotate) p.slices = 0;
    p.open_on_chain = p.rotate && k.chain_rule(p.deep);
    p.chain_stream = !p.open_on_chain ? -1 : p.heavy_stream == 3 ? (int)ROLE_SIDE : (int)ROLE_LANE1 + p.heavy_stream - 1;
    if (k.blinding_draw) {  // no draw chain: nothing of its form is decided; streams, rotation, slices, par and raw_index() stay as above
        p.chain = ProvePlan::EXPANDED;
        p.coop = false;
        p.prefix_form = B <= (uint32_t)k.tr_wave_below ? 2u : 1u;
    }
    return p;
}

}  // namespace bbp
