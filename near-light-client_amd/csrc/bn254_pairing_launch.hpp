// What bn254_pairing.hip's verifiers enqueue, reachable from the other verifier built on the pairing (bn254_plonk_verify.hip):
// the entry checks of points, the Miller / final-exponentiation pair of launches and the read-back of the result words.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "ctx.hpp"

namespace nlx {
namespace pairing {

// the value every status / result word is preset to; no kernel writes it, and the host answers NLX_E_HIP where it finds it
constexpr uint32_t WORD_UNSET = 0xFFFFFFFFu;
constexpr size_t MAX_PAIRS = (size_t)1 << 20;

// The entry checks of n pairs (either side may be NULL, device pointers): NLX_E_RANGE naming the first offending pair as
// "`what` i: ...".
int32_t check_points(nlx_ctx* ctx, Scratch& scratch, const uint64_t* d_g1, const uint64_t* d_g2, size_t n, const char* what);
// Miller loops of n_pairs pairs and the final exponentiations of n_checks checks: enqueues only.  d_first: n_checks + 1 offsets
// into the pairs (NULL: check i is pair i); checks below n_expected are compared with d_expected (48 Montgomery words), the
// others with 1.  d_result: n_checks words, preset here.
int32_t enqueue_checks(nlx_ctx* ctx, Scratch& scratch, const uint64_t* d_g1, const uint64_t* d_g2, size_t n_pairs, const uint32_t* d_first,
                       size_t n_checks, size_t n_expected, const uint64_t* d_expected, int montgomery, uint64_t* d_gt, uint32_t* d_result);
// the n result words to the host (synchronises; with `last`, drains it); NLX_E_HIP for a word no lane wrote
int32_t read_results(nlx_ctx* ctx, const uint32_t* d_result, size_t n, std::vector<uint32_t>& out, Scratch* last);

}  // namespace pairing
}  // namespace nlx
