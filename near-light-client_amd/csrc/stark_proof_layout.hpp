// Where everything lies in a STARK proof (wire format: DESIGN.md section 8), computed from the descriptor alone: the head of its
// own, and around it the part every proof with a FRI proof in it has (fri_proof_layout.hpp, with the parser).  Host only: no HIP
// include, so that a stand-alone program can run it under a sanitizer (tests/tools/layout_check.cpp).
//
//   caps of the trace batches, then the quotient cap                (n_oracles x 4 << cap_height words)
//   openings: local, next (n_cols extension elements each), quotient (nq)
//   FRI commit caps                                                 (n_layers caps)
//   per query:  per commitment  row | path-length byte | siblings (4 words each)
//               per FRI layer   2 x arity words | path-length byte | siblings
//   final polynomial (2 x final_len words), proof-of-work witness
//   public-input count (one word), public inputs, round values
//
#pragma once
#include "fri_proof_layout.hpp"

namespace nlx {
namespace spl {

constexpr uint32_t MAX_ORACLES = fpl::MAX_TREES;   // NLX_STARK_MAX_ORACLES trace batches and the quotient
// the parser and its findings are the common part's, under this format's name too
using fpl::parse; using fpl::Finding;
using fpl::SOUND; using fpl::BAD_LENGTH; using fpl::BAD_PUBLIC_INPUT_COUNT; using fpl::BAD_PATH_LENGTH; using fpl::BAD_WORD;

// what the descriptor says
struct Shape {
    uint32_t degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits, n_queries;
    uint32_t n_cols, nq, n_pis, n_round_values;
    uint32_t n_oracles;                 // trace batches, then the quotient
    uint32_t oracle_cols[MAX_ORACLES];
};

// the common part (its trees: the oracles), then the head of a STARK proof and its round values
struct Layout : fpl::Layout {
    Shape sh;
    size_t caps, local, next, quotient, round_values;             // byte offsets in the proof
    size_t w_caps, w_local, w_next, w_quotient, w_round_values;   // word offsets in the staging buffer
};

// false: a shape no proof has (more commitments or layers than the format allows)
inline bool make_layout(const Shape& s, Layout* out) {
    Layout& l = *out;
    memset(&l, 0, sizeof l);
    l.sh = s;
    if (s.n_oracles == 0 || s.n_oracles > MAX_ORACLES) return false;
    const size_t capw = (size_t)4 << s.cap_height;
    l.w_caps = 0;
    l.w_local = s.n_oracles * capw;
    l.w_next = l.w_local + 2 * (size_t)s.n_cols;
    l.w_quotient = l.w_next + 2 * (size_t)s.n_cols;
    if (!fpl::fill(l, s.degree_bits, s.rate_bits, s.cap_height, s.arity_bits, s.final_poly_bits, s.n_queries, s.n_pis, s.n_oracles,
                   s.oracle_cols, l.w_quotient + 2 * (size_t)s.nq, s.n_round_values))
        return false;
    l.caps = 0;
    l.local = 8 * l.w_local;
    l.next = 8 * l.w_next;
    l.quotient = 8 * l.w_quotient;
    l.round_values = l.public_inputs + 8 * (size_t)s.n_pis;
    l.w_round_values = l.w_public_inputs + s.n_pis;
    return true;
}

}  // namespace spl
}  // namespace nlx
