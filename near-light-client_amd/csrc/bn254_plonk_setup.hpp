// The result of nlx_bn254_plonk_setup (bn254_plonk_setup.hip owns it; bn254_plonk_solve.hip, the witness solver, reads it).
#pragma once
#include <cstdint>
#include <vector>
#include "ctx.hpp"

// The result: one device block [vals (8 + k) n x 32 B | cells | perm | sigma_cells, 3 n words each] and what the key's creation
// needs on the host.
struct nlx_bn254_plonk_setup {
    nlx_ctx* ctx = nullptr;
    uint32_t log_n = 0, k = 0;
    uint64_t n_variables = 0, n_public = 0, n_constraints = 0, occurring = 0, longest = 0;
    uint64_t* vals = nullptr;
    uint32_t *cells = nullptr, *perm = nullptr, *sigma_cells = nullptr;
    uint64_t k1[4], k2[4], shift[4];
    std::vector<uint64_t> counts;
    std::vector<uint32_t> committed_rows, commit_rows;
    // the solver's schedule is made on the host (bn254_plonk_solve.hpp): the constraints' cells and, per constraint, which of
    // ql qr qm qo qk are nonzero (bit s for selector s)
    std::vector<uint32_t> x[3];
    std::vector<uint8_t> nonzero;
};
