// The resident STARK (nlx_stark_build) as the prover (stark.hip) and the trace checker (stark_check.hip) see it.
#pragma once
#include <vector>
#include "air_vm.hpp"
#include "prove_common.hpp"

struct nlx_stark {
    nlx_ctx* ctx = nullptr;
    nlx_stark_desc d{};
    std::vector<uint64_t> program;  // canonicalised copy
    uint32_t qdb = 0, nq = 0, n_regs = 0, n_fri_rounds = 0;
    uint32_t n_rounds = 1, round_cols[3] = {0, 0, 0}, round_challenges[3] = {0, 0, 0}, round_values[3] = {0, 0, 0},
             n_round_challenges = 0;  // n_round_challenges: round values + challenges, i.e. the values array minus public inputs
    uint64_t air_digest[4] = {0, 0, 0, 0};  // the statement digest the transcript opens with (air_digest_host)
    uint64_t* d_program = nullptr;
    const nlx::AirGenEntry* gen = nullptr;   // a straight-line kernel generated from exactly this program (csrc/airgen/), or nullptr: the interpreter
    std::vector<uint32_t> seg;        // {first word, end word} per program segment
    std::vector<uint32_t> seg_after;  // constraints emitted after each segment
    std::vector<uint32_t> seg_regs;   // registers each segment uses (table sorted by this)
    std::vector<uint32_t> seg_group;  // first segment of each launch group
    uint32_t* d_seg = nullptr;
    uint64_t* d_small = nullptr;  // FRI coset tables (rate_bits) | quotient coset tables (qdb) | w_A^-i
    uint64_t *d_coset_base = nullptr, *d_q_coset_base = nullptr, *d_q_zh_inv = nullptr, *d_q_wR_inv = nullptr,
             *d_q_chunk_scale = nullptr, *d_wA_inv = nullptr;
    uint64_t* d_l_inv = nullptr;               // [2^qdb][n]
    uint64_t* d_periodic = nullptr;            // [n_periodic][2^qdb][period]
    std::vector<uint64_t> periodic;            // canonicalised host copy
    const uint64_t* d_q_inv_scale_br = nullptr;  // ctx-owned
    // the trace checker's (stark_check.hip): made by the first check, null in a STARK that is never checked
    uint32_t n_constraints = 0;                // what the program emits
    std::vector<uint32_t> seg_first;           // per row of the (sorted) segment table: index of the first constraint it emits
    uint32_t* d_seg_first = nullptr;
    uint64_t* d_periodic_rows = nullptr;       // [n_periodic][period]: `periodic` as it stands
    uint64_t* d_check = nullptr;               // the checker's counters and minimum (CheckBlock)
    // the verifier's (stark_verify.hip): made by the first verify, null in a STARK that is never verified
    uint64_t* d_verify = nullptr;              // [n_periodic][period]: coefficients of the periodic columns' interpolations
    nlx::StageClock clock;
};
