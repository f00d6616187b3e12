// Where everything lies in a plonky2 ProofWithPublicInputs (util::serialization's to_bytes, as prover.hip writes it), computed
// from the circuit descriptor alone: the head of its own, and around it the part every proof with a FRI proof in it has
// (fri_proof_layout.hpp, with the parser).  Host only: no HIP include, so that a stand-alone program can run it under a sanitizer
// (tests/tools/layout_check.cpp).
//
//   caps: wires, Zs / partial products (/ lookup polynomials), quotient     (3 x 4 << cap_height words)
//   openings, extension elements, in wire order: constants, sigmas, wires, zs, zs_next, lookup_zs, lookup_zs_next,
//             partial products, quotient
//   FRI commit caps                                                         (n_layers caps)
//   per query:  per tree (constants_sigmas, wires, zs_partial, quotient)  row | path-length byte | siblings (4 words each)
//               per FRI layer   2 x arity words | path-length byte | siblings
//   final polynomial (2 x final_len words), proof-of-work witness
//   public-input count (write_usize: one word), public inputs
//
#pragma once
#include "fri_proof_layout.hpp"

namespace nlx {
namespace ppl {

constexpr uint32_t N_TREES = 4;     // constants_sigmas (the circuit's own cap), wires, zs_partial, quotient
// the parser and its findings are the common part's, under this format's name too
using fpl::parse; using fpl::Finding;
using fpl::SOUND; using fpl::BAD_LENGTH; using fpl::BAD_PUBLIC_INPUT_COUNT; using fpl::BAD_PATH_LENGTH; using fpl::BAD_WORD;
// the opening classes, in wire order
enum : uint32_t { O_CONSTANTS = 0, O_SIGMAS, O_WIRES, O_ZS, O_ZS_NEXT, O_LOOKUP_ZS, O_LOOKUP_ZS_NEXT, O_PARTIAL_PRODUCTS, O_QUOTIENT, N_OPENINGS };

// what the descriptor says
struct Shape {
    uint32_t degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits, n_queries, n_pis;
    uint32_t n_constants;     // selectors + lookup selectors + gate constants
    uint32_t n_sigmas;        // routed wires
    uint32_t n_wires;
    uint32_t n_challenges;
    uint32_t n_partial;       // num_challenges * num_partial_products
    uint32_t n_lookup_polys;  // num_challenges * (1 + S), or 0
    uint32_t n_quotient;      // num_challenges * quotient_degree_factor
};

// the common part (its trees: the four above), then the head of a plonky2 proof
struct Layout : fpl::Layout {
    Shape sh;
    size_t caps, openings[N_OPENINGS];       // byte offsets in the proof
    size_t w_caps, w_openings[N_OPENINGS];   // word offsets in the staging buffer
};

// false: a shape no proof has.  hasher: of the proof's trees (fpl::HASHER_*) - which words the parser checks as digests
inline bool make_layout(const Shape& s, Layout* out, uint32_t hasher = fpl::HASHER_GOLDILOCKS) {
    Layout& l = *out;
    memset(&l, 0, sizeof l);
    l.sh = s;
    if (s.degree_bits + s.rate_bits > 32 || s.arity_bits < 1) return false;
    const uint32_t tree_cols[N_TREES] = {s.n_constants + s.n_sigmas, s.n_wires, s.n_challenges + s.n_partial + s.n_lookup_polys, s.n_quotient};
    const uint32_t counts[N_OPENINGS] = {s.n_constants, s.n_sigmas, s.n_wires, s.n_challenges, s.n_challenges, s.n_lookup_polys,
                                         s.n_lookup_polys, s.n_partial, s.n_quotient};
    size_t w = 3 * ((size_t)4 << s.cap_height);   // the caps
    for (uint32_t c = 0; c < N_OPENINGS; c++) {
        l.w_openings[c] = w;
        l.openings[c] = 8 * w;
        w += 2 * (size_t)counts[c];
    }
    if (!fpl::fill(l, s.degree_bits, s.rate_bits, s.cap_height, s.arity_bits, s.final_poly_bits, s.n_queries, s.n_pis, N_TREES, tree_cols,
                   w, 0))
        return false;
    l.w_head_caps = l.w_caps;   // 0: the three caps open the proof
    l.n_head_cap_words = 3 * l.cap_words;
    l.hasher = hasher;
    return true;
}

}  // namespace ppl
}  // namespace nlx
