// Where everything lies in a STARK proof (wire format: DESIGN.md section 8), computed from the descriptor alone, and the parser
// that checks a proof's structure against it.  Host only: no HIP include, so that a stand-alone program can run it under a
// sanitizer (tests/tools/stark_layout_check.cpp).
//
//   caps of the trace batches, then the quotient cap                (n_oracles x 4 << cap_height words)
//   openings: local, next (n_cols extension elements each), quotient (nq)
//   FRI commit caps                                                 (n_layers caps)
//   per query:  per commitment  row | path-length byte | siblings (4 words each)
//               per FRI layer   2 x arity words | path-length byte | siblings
//   final polynomial (2 x final_len words), proof-of-work witness
//   public-input count (one word), public inputs, round values
//
// The path-length bytes leave every later 64-bit word unaligned.  parse() checks those bytes and copies the words into an
// aligned staging buffer - the proof without its path-length bytes, so a word's place there follows from the descriptor too.
// The device reads only that buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace nlx {
namespace spl {

constexpr uint64_t FIELD_P = 0xFFFFFFFF00000001ULL;
constexpr uint32_t MAX_ORACLES = 32;   // NLX_STARK_MAX_ORACLES trace batches and the quotient
constexpr uint32_t MAX_LAYERS = 16;

// what the descriptor says
struct Shape {
    uint32_t degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits, n_queries;
    uint32_t n_cols, nq, n_pis, n_round_values;
    uint32_t n_oracles;                 // trace batches, then the quotient
    uint32_t oracle_cols[MAX_ORACLES];
};

struct Layout {
    Shape sh;
    uint32_t log_L, n_layers, arity, final_len, n_path_bytes_per_query;
    uint32_t oracle_plen, layer_plen[MAX_LAYERS];
    size_t cap_words;
    // byte offsets in the proof
    size_t caps, local, next, quotient, fri_caps, queries, query_bytes, final_poly, pow_witness, n_pis_word, public_inputs,
        round_values, total;
    // byte offsets within one query
    size_t row[MAX_ORACLES], path_len[MAX_ORACLES], path[MAX_ORACLES];
    size_t layer_evals[MAX_LAYERS], layer_path_len[MAX_LAYERS], layer_path[MAX_LAYERS];
    // word offsets in the staging buffer
    size_t w_caps, w_local, w_next, w_quotient, w_fri_caps, w_queries, w_query_words, w_final_poly, w_pow_witness, w_n_pis_word,
        w_public_inputs, w_round_values, w_total;
    // word offsets within one query of the staging buffer
    size_t w_row[MAX_ORACLES], w_path[MAX_ORACLES], w_layer_evals[MAX_LAYERS], w_layer_path[MAX_LAYERS];
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

// false: a shape no proof has (more commitments or layers than the format allows)
inline bool make_layout(const Shape& s, Layout* out) {
    Layout& l = *out;
    memset(&l, 0, sizeof l);
    l.sh = s;
    l.log_L = s.degree_bits + s.rate_bits;
    l.n_layers = num_layers(s);
    if (s.n_oracles == 0 || s.n_oracles > MAX_ORACLES || l.n_layers > MAX_LAYERS || s.cap_height > l.log_L || s.arity_bits > 6) return false;
    l.arity = 1u << s.arity_bits;
    l.final_len = 1u << (s.degree_bits - l.n_layers * s.arity_bits);
    l.cap_words = (size_t)4 << s.cap_height;
    l.oracle_plen = l.log_L - s.cap_height;
    size_t b = 0, w = 0;
    auto words = [&](size_t n, size_t* at_b, size_t* at_w) {
        *at_b = b;
        *at_w = w;
        b += 8 * n;
        w += n;
    };
    words(s.n_oracles * l.cap_words, &l.caps, &l.w_caps);
    words(2 * (size_t)s.n_cols, &l.local, &l.w_local);
    words(2 * (size_t)s.n_cols, &l.next, &l.w_next);
    words(2 * (size_t)s.nq, &l.quotient, &l.w_quotient);
    words(l.n_layers * l.cap_words, &l.fri_caps, &l.w_fri_caps);
    {
        size_t qb = 0, qw = 0;
        for (uint32_t o = 0; o < s.n_oracles; o++) {
            l.row[o] = qb;
            l.w_row[o] = qw;
            qb += 8 * (size_t)s.oracle_cols[o];
            qw += s.oracle_cols[o];
            l.path_len[o] = qb++;
            l.path[o] = qb;
            l.w_path[o] = qw;
            qb += 32 * (size_t)l.oracle_plen;
            qw += 4 * (size_t)l.oracle_plen;
        }
        uint32_t lg = l.log_L;
        for (uint32_t k = 0; k < l.n_layers; k++) {
            lg -= s.arity_bits;
            l.layer_plen[k] = lg > s.cap_height ? lg - s.cap_height : 0;
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
        l.n_path_bytes_per_query = s.n_oracles + l.n_layers;
    }
    l.queries = b;
    l.w_queries = w;
    b += l.query_bytes * s.n_queries;
    w += l.w_query_words * s.n_queries;
    words(2 * (size_t)l.final_len, &l.final_poly, &l.w_final_poly);
    words(1, &l.pow_witness, &l.w_pow_witness);
    words(1, &l.n_pis_word, &l.w_n_pis_word);
    words(s.n_pis, &l.public_inputs, &l.w_public_inputs);
    words(s.n_round_values, &l.round_values, &l.w_round_values);
    l.total = b;
    l.w_total = w;
    return true;
}

enum : uint32_t { SOUND = 0, BAD_LENGTH = 1, BAD_PUBLIC_INPUT_COUNT = 2, BAD_PATH_LENGTH = 3, BAD_WORD = 4 };

struct Finding {
    uint32_t what = SOUND;
    uint32_t query = 0, tree = 0, layer = 0;   // BAD_PATH_LENGTH: where (tree < n_oracles: a commitment; else a FRI layer)
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
        for (uint32_t o = 0; o < l.sh.n_oracles; o++) {
            if (qp[l.path_len[o]] != l.oracle_plen && f->what == SOUND) {
                f->what = BAD_PATH_LENGTH;
                f->query = q;
                f->tree = o;
            }
            memcpy(qs + l.w_row[o], qp + l.row[o], 8 * (size_t)l.sh.oracle_cols[o]);
            memcpy(qs + l.w_path[o], qp + l.path[o], 32 * (size_t)l.oracle_plen);
        }
        for (uint32_t k = 0; k < l.n_layers; k++) {
            if (qp[l.layer_path_len[k]] != l.layer_plen[k] && f->what == SOUND) {
                f->what = BAD_PATH_LENGTH;
                f->query = q;
                f->tree = l.sh.n_oracles + k;
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

}  // namespace spl
}  // namespace nlx
