// Where everything lies in a plonky2 ProofWithPublicInputs (util::serialization's to_bytes, as prover.hip writes it), computed
// from the circuit descriptor alone, and the parser that checks a proof's structure against it.  Host only: no HIP include, so
// that a stand-alone program can run it under a sanitizer (tests/tools/plonk_layout_check.cpp).  The sibling of
// stark_proof_layout.hpp.
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
// The path-length bytes leave every later 64-bit word unaligned.  parse() checks those bytes and copies the words into an
// aligned staging buffer - the proof without its path-length bytes, so a word's place there follows from the descriptor too.
// The device reads only that buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace nlx {
namespace ppl {

constexpr uint64_t FIELD_P = 0xFFFFFFFF00000001ULL;
constexpr uint32_t N_TREES = 4;     // constants_sigmas (the circuit's own cap), wires, zs_partial, quotient
constexpr uint32_t MAX_LAYERS = 16;
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

struct Layout {
    Shape sh;
    uint32_t log_L, n_layers, arity, final_len;
    uint32_t tree_cols[N_TREES], open_count[N_OPENINGS];
    uint32_t tree_plen, layer_plen[MAX_LAYERS];
    size_t cap_words;
    // byte offsets in the proof
    size_t caps, openings[N_OPENINGS], fri_caps, queries, query_bytes, final_poly, pow_witness, n_pis_word, public_inputs, total;
    // byte offsets within one query
    size_t row[N_TREES], path_len[N_TREES], path[N_TREES];
    size_t layer_evals[MAX_LAYERS], layer_path_len[MAX_LAYERS], layer_path[MAX_LAYERS];
    // word offsets in the staging buffer
    size_t w_caps, w_openings[N_OPENINGS], w_fri_caps, w_queries, w_query_words, w_final_poly, w_pow_witness, w_n_pis_word,
        w_public_inputs, w_total;
    // word offsets within one query of the staging buffer
    size_t w_row[N_TREES], w_path[N_TREES], w_layer_evals[MAX_LAYERS], w_layer_path[MAX_LAYERS];
};

// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits)
inline uint32_t num_layers(const Shape& s) {
    uint32_t degree_bits = s.degree_bits, r = 0;
    while (degree_bits > s.final_poly_bits && degree_bits + s.rate_bits >= s.cap_height + s.arity_bits) {
        if (degree_bits < s.arity_bits) break;
        degree_bits -= s.arity_bits;
        r++;
    }
    return r;
}

// false: a shape no proof has
inline bool make_layout(const Shape& s, Layout* out) {
    Layout& l = *out;
    memset(&l, 0, sizeof l);
    l.sh = s;
    l.log_L = s.degree_bits + s.rate_bits;
    l.n_layers = num_layers(s);
    if (l.n_layers > MAX_LAYERS || s.cap_height > l.log_L || l.log_L > 32 || s.arity_bits < 1 || s.arity_bits > 6) return false;
    l.arity = 1u << s.arity_bits;
    l.final_len = 1u << (s.degree_bits - l.n_layers * s.arity_bits);
    l.cap_words = (size_t)4 << s.cap_height;
    l.tree_plen = l.log_L - s.cap_height;
    l.tree_cols[0] = s.n_constants + s.n_sigmas;
    l.tree_cols[1] = s.n_wires;
    l.tree_cols[2] = s.n_challenges + s.n_partial + s.n_lookup_polys;
    l.tree_cols[3] = s.n_quotient;
    const uint32_t counts[N_OPENINGS] = {s.n_constants, s.n_sigmas, s.n_wires, s.n_challenges, s.n_challenges, s.n_lookup_polys,
                                         s.n_lookup_polys, s.n_partial, s.n_quotient};
    size_t b = 0, w = 0;
    auto words = [&](size_t n, size_t* at_b, size_t* at_w) {
        *at_b = b;
        *at_w = w;
        b += 8 * n;
        w += n;
    };
    words(3 * l.cap_words, &l.caps, &l.w_caps);
    for (uint32_t c = 0; c < N_OPENINGS; c++) {
        l.open_count[c] = counts[c];
        words(2 * (size_t)counts[c], &l.openings[c], &l.w_openings[c]);
    }
    words(l.n_layers * l.cap_words, &l.fri_caps, &l.w_fri_caps);
    {
        size_t qb = 0, qw = 0;
        for (uint32_t o = 0; o < N_TREES; o++) {
            l.row[o] = qb;
            l.w_row[o] = qw;
            qb += 8 * (size_t)l.tree_cols[o];
            qw += l.tree_cols[o];
            l.path_len[o] = qb++;
            l.path[o] = qb;
            l.w_path[o] = qw;
            qb += 32 * (size_t)l.tree_plen;
            qw += 4 * (size_t)l.tree_plen;
        }
        uint32_t lg = l.log_L;
        for (uint32_t k = 0; k < l.n_layers; k++) {
            lg -= s.arity_bits;
            l.layer_plen[k] = lg > s.cap_height ? lg - s.cap_height : 0;   // a tree no taller than its cap: no siblings
            l.layer_evals[k] = qb;
            l.w_layer_evals[k] = qw;
            qb += 16 * (size_t)l.arity;
            qw += 2 * (size_t)l.arity;
            l.layer_path_len[k] = qb++;
            l.layer_path[k] = qb;
            l.w_layer_path[k] = qw;
            qb += 32 * (size_t)l.layer_plen[k];
            qw += 4 * (size_t)l.layer_plen[k];
        }
        l.query_bytes = qb;
        l.w_query_words = qw;
    }
    l.queries = b;
    l.w_queries = w;
    b += l.query_bytes * s.n_queries;
    w += l.w_query_words * s.n_queries;
    words(2 * (size_t)l.final_len, &l.final_poly, &l.w_final_poly);
    words(1, &l.pow_witness, &l.w_pow_witness);
    words(1, &l.n_pis_word, &l.w_n_pis_word);
    words(s.n_pis, &l.public_inputs, &l.w_public_inputs);
    l.total = b;
    l.w_total = w;
    return true;
}

enum : uint32_t { SOUND = 0, BAD_LENGTH = 1, BAD_PUBLIC_INPUT_COUNT = 2, BAD_PATH_LENGTH = 3, BAD_WORD = 4 };

struct Finding {
    uint32_t what = SOUND;
    uint32_t query = 0, tree = 0, layer = 0;   // BAD_PATH_LENGTH: where (tree < N_TREES: an initial tree; else a FRI layer)
    size_t word = 0;                           // BAD_WORD: its index in the staging buffer
};

// Checks `proof` against the layout and fills `staging` (l.w_total words).  Reads proof[0 .. len) only, and nothing at all unless
// len == l.total; no offset depends on a byte of the proof.  The first finding wins, in the order of the enum.
inline uint32_t parse(const Layout& l, const uint8_t* proof, size_t len, uint64_t* staging, Finding* f) {
    *f = Finding();
    if (len != l.total) return f->what = BAD_LENGTH;
    uint64_t n_pis;
    memcpy(&n_pis, proof + l.n_pis_word, 8);
    if (n_pis != l.sh.n_pis) return f->what = BAD_PUBLIC_INPUT_COUNT;
    memcpy(staging, proof, l.queries);
    for (uint32_t q = 0; q < l.sh.n_queries; q++) {
        const uint8_t* qp = proof + l.queries + (size_t)q * l.query_bytes;
        uint64_t* qs = staging + l.w_queries + (size_t)q * l.w_query_words;
        for (uint32_t o = 0; o < N_TREES; o++) {
            if (qp[l.path_len[o]] != l.tree_plen && f->what == SOUND) {
                f->what = BAD_PATH_LENGTH;
                f->query = q;
                f->tree = o;
            }
            memcpy(qs + l.w_row[o], qp + l.row[o], 8 * (size_t)l.tree_cols[o]);
            memcpy(qs + l.w_path[o], qp + l.path[o], 32 * (size_t)l.tree_plen);
        }
        for (uint32_t k = 0; k < l.n_layers; k++) {
            if (qp[l.layer_path_len[k]] != l.layer_plen[k] && f->what == SOUND) {
                f->what = BAD_PATH_LENGTH;
                f->query = q;
                f->tree = N_TREES + k;
                f->layer = k;
            }
            memcpy(qs + l.w_layer_evals[k], qp + l.layer_evals[k], 16 * (size_t)l.arity);
            memcpy(qs + l.w_layer_path[k], qp + l.layer_path[k], 32 * (size_t)l.layer_plen[k]);
        }
    }
    memcpy(staging + l.w_final_poly, proof + l.final_poly, l.total - l.final_poly);
    if (f->what != SOUND) return f->what;
    for (size_t i = 0; i < l.w_total; i++)
        if (staging[i] >= FIELD_P) {   // the proof-of-work witness is a field element too; the count word was compared above
            f->what = BAD_WORD;
            f->word = i;
            return f->what;
        }
    return SOUND;
}

}  // namespace ppl
}  // namespace nlx
