// What the rows of one verify call are: the one descriptor every verify path passes along, from the extern "C" entry points
// through the pool split and the host chunk loop down to the launches (include/bbp.h "bbp_verify_batch", "_mixed", "bbp_verify_rounds").
// Host-only, no HIP types: pool.cpp, the capi_*.hip units, verifier.inc and the CPU test tier (tests/host_check.cpp) include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/bbp.h"

namespace bbp {

// R1CSProof || commitments || t_c for list length n: layout 0 is the compact 1121-byte proof, 1 the two-phase one (three more points)
inline size_t proof_record_bytes(uint32_t n, uint32_t ver = 0) { return (ver ? BBP_R1CS_PROOF_BYTES + 96u : BBP_R1CS_PROOF_BYTES) + 32 * (4 + (size_t)n); }
// one row of bbp_verify_batch[_mixed]: record || score || z_img || seed || pub_list
inline size_t verify_row_bytes(uint32_t n, uint32_t ver = 0) { return proof_record_bytes(n, ver) + 96 + 32 * (size_t)n; }
// one row of bbp_verify_rounds: record || score || z_img (compact records only; seed and pub_list come from the row's round)
inline size_t round_row_bytes(uint32_t n) { return proof_record_bytes(n) + 64; }

struct VerifyRows {
    enum Kind : uint32_t {
        UNIFORM,  // B rows of list length N and record layout rec_ver
        MIXED,    // row i has list length ns[i] and layout vers[i] (vers null: compact rows); rows packed back to back
        ROUNDS    // row i is record || score || z_img of round round_of[i] (null: round 0, R == 1 only); round r of the table is
                  // seed || pub_list(round_ns[r]), packed back to back
    };
    Kind kind = UNIFORM;
    uint32_t B = 0;
    uint32_t N = 0;        // UNIFORM only
    uint32_t rec_ver = 0;  // every kind: 1 when a row of the call has a two-phase record.  Such a call is not aggregated.
    const uint32_t* ns = nullptr;  // MIXED: host memory, screened by the entry points, as round_ns and round_of
    const uint8_t* vers = nullptr;
    uint32_t R = 0;  // ROUNDS
    const uint32_t* round_ns = nullptr;
    const uint8_t* rounds = nullptr;  // the table: host memory on the way into the host path, device memory in the drivers
    const uint32_t* round_of = nullptr;

    // The constructors normalise.  mixed(): version bytes that are all 0 are dropped (the call the public mixed entry points make),
    // one that is not makes rec_ver 1.  A mixed call whose ns are all equal stays mixed.
    static VerifyRows uniform(uint32_t B, uint32_t N, uint32_t rec_ver = 0) {
        VerifyRows v;
        v.B = B, v.N = N, v.rec_ver = rec_ver ? 1u : 0u;
        return v;
    }
    static VerifyRows mixed(uint32_t B, const uint32_t* ns, const uint8_t* vers = nullptr) {
        VerifyRows v;
        v.kind = MIXED, v.B = B, v.ns = ns, v.vers = vers;
        v.rec_ver = v.any_two_phase();
        if (!v.rec_ver) v.vers = nullptr;
        return v;
    }
    static VerifyRows of_rounds(uint32_t B, uint32_t R, const uint32_t* round_ns, const uint8_t* rounds, const uint32_t* round_of) {
        VerifyRows v;
        v.kind = ROUNDS, v.B = B, v.R = R, v.round_ns = round_ns, v.rounds = rounds, v.round_of = round_of;
        return v;
    }

    uint32_t n_of(uint32_t i) const { return kind == UNIFORM ? N : kind == MIXED ? ns[i] : round_ns[round_of ? round_of[i] : 0]; }
    uint32_t ver_of(uint32_t i) const { return kind == UNIFORM ? rec_ver : vers && vers[i] ? 1u : 0u; }
    size_t row_bytes(uint32_t i) const { return kind == ROUNDS ? round_row_bytes(n_of(i)) : verify_row_bytes(n_of(i), ver_of(i)); }
    uint32_t first_n() const { return n_of(0); }  // any list length of the call
    // byte offset of every row, and the size of all rows at [B]
    std::vector<size_t> offsets() const {
        std::vector<size_t> off((size_t)B + 1, 0);
        for (uint32_t i = 0; i < B; i++) off[i + 1] = off[i] + row_bytes(i);
        return off;
    }
    size_t table_bytes() const {
        size_t t = 0;
        for (uint32_t r = 0; r < R; r++) t += 32 * (1 + (size_t)round_ns[r]);
        return t;
    }
    // Which front end runs: the mixed kernels (per-row N, strides of the largest) for a mixed call and for rounds with R > 1, even
    // when every N is the same; the uniform kernels for list length front_n() otherwise (one round: behind k_vparse_round).
    bool mixed_front() const { return kind == MIXED || (kind == ROUNDS && R > 1); }
    uint32_t front_n() const { return kind == ROUNDS ? round_ns[0] : N; }
    // Rows [lo, hi) as a call of their own (the host chunk loop, the pool's block split): the per-row arrays advance, the round table
    // stays whole.  The slice keeps the call's version bytes; its rec_ver is that of its own rows.
    VerifyRows slice(uint32_t lo, uint32_t hi) const {
        VerifyRows s = *this;
        s.B = hi - lo;
        if (ns) s.ns += lo;
        if (round_of) s.round_of += lo;
        if (vers) {
            s.vers += lo;
            s.rec_ver = s.any_two_phase();
        }
        return s;
    }

   private:
    uint32_t any_two_phase() const {
        for (uint32_t i = 0; vers && i < B; i++)
            if (vers[i]) return 1;
        return 0;
    }
};

}  // namespace bbp
