// What the proof formats with a FRI proof in them have in common (stark_proof_layout.hpp, plonk_proof_layout.hpp): a head of the
// format's own - caps and openings -, then
//
//   FRI commit caps                                                 (n_layers caps)
//   per query:  per initial tree  row | path-length byte | siblings (4 words each)
//               per FRI layer     2 x arity words | path-length byte | siblings
//   final polynomial (2 x final_len words), proof-of-work witness
//   public-input count (one word), public inputs, then words of the format's own
//
// and the one parser that checks a proof's structure against that.  The path-length bytes leave every later 64-bit word
// unaligned.  parse() checks those bytes and copies the words into an aligned staging buffer - the proof without its path-length
// bytes, so a word's place there follows from the descriptor too.  The device reads only that buffer.
// A proof made under the PoseidonBN128 config (Layout::hasher = HASHER_BN128) has the same bytes, but a digest there is four
// little-endian words of ONE integer below BN254's r, and its words need not be below p: the layout knows which staging words are
// digests - the head's caps, the FRI caps, every path sibling - and parse() checks those four at a time against r.
// Host only: no HIP include, so that a stand-alone program can run it under a sanitizer (tests/tools/layout_check.cpp,
// tests/tools/digest_words_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "bn254_fp.hpp"

namespace nlx {
namespace fpl {

constexpr uint64_t FIELD_P = 0xFFFFFFFF00000001ULL;
constexpr uint32_t MAX_TREES = 32;    // initial trees of one proof
constexpr uint32_t MAX_LAYERS = 16;
enum : uint32_t { HASHER_GOLDILOCKS = 0, HASHER_BN128 = 1 };   // NLX_HASHER_* (include/nlx.h)

// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits)
inline uint32_t num_layers(uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t arity_bits, uint32_t final_poly_bits) {
    uint32_t r = 0;
    while (degree_bits > final_poly_bits && degree_bits + rate_bits >= cap_height + arity_bits) {
        if (degree_bits < arity_bits) break;
        degree_bits -= arity_bits;
        r++;
    }
    return r;
}

struct Layout {
    uint32_t hasher;                       // of the proof's Merkle trees; fill() leaves HASHER_GOLDILOCKS
    size_t w_head_caps, n_head_cap_words;  // the caps in the format's head (staging words); the format sets them after fill()
    uint32_t n_queries, n_pis, n_trees, tree_cols[MAX_TREES];
    uint32_t log_L, n_layers, arity, final_len;
    uint32_t tree_plen, layer_plen[MAX_LAYERS];
    size_t cap_words;
    // byte offsets in the proof
    size_t fri_caps, queries, query_bytes, final_poly, pow_witness, n_pis_word, public_inputs, total;
    // byte offsets within one query
    size_t row[MAX_TREES], path_len[MAX_TREES], path[MAX_TREES];
    size_t layer_evals[MAX_LAYERS], layer_path_len[MAX_LAYERS], layer_path[MAX_LAYERS];
    // word offsets in the staging buffer
    size_t w_fri_caps, w_queries, w_query_words, w_final_poly, w_pow_witness, w_n_pis_word, w_public_inputs, w_total;
    // word offsets within one query of the staging buffer
    size_t w_row[MAX_TREES], w_path[MAX_TREES], w_layer_evals[MAX_LAYERS], w_layer_path[MAX_LAYERS];
};

// Fills `l`: head_words words of the format's own before the FRI caps, tail_words after the public inputs.
// false: a shape no proof has (more trees or layers than the format allows)
inline bool fill(Layout& l, uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t arity_bits, uint32_t final_poly_bits,
                 uint32_t n_queries, uint32_t n_pis, uint32_t n_trees, const uint32_t* tree_cols, size_t head_words, size_t tail_words) {
    l.hasher = HASHER_GOLDILOCKS;
    l.w_head_caps = l.n_head_cap_words = 0;
    l.log_L = degree_bits + rate_bits;
    l.n_layers = num_layers(degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits);
    if (n_trees > MAX_TREES || l.n_layers > MAX_LAYERS || cap_height > l.log_L || arity_bits > 6) return false;
    l.n_queries = n_queries;
    l.n_pis = n_pis;
    l.n_trees = n_trees;
    l.arity = 1u << arity_bits;
    l.final_len = 1u << (degree_bits - l.n_layers * arity_bits);
    l.cap_words = (size_t)4 << cap_height;
    l.tree_plen = l.log_L - cap_height;
    size_t b = 8 * head_words, w = head_words;
    auto words = [&](size_t n, size_t* at_b, size_t* at_w) {
        *at_b = b;
        *at_w = w;
        b += 8 * n;
        w += n;
    };
    words(l.n_layers * l.cap_words, &l.fri_caps, &l.w_fri_caps);
    size_t qb = 0, qw = 0;
    for (uint32_t o = 0; o < n_trees; o++) {
        l.tree_cols[o] = tree_cols[o];
        l.row[o] = qb;
        l.w_row[o] = qw;
        qb += 8 * (size_t)tree_cols[o];
        qw += tree_cols[o];
        l.path_len[o] = qb++;
        l.path[o] = qb;
        l.w_path[o] = qw;
        qb += 32 * (size_t)l.tree_plen;
        qw += 4 * (size_t)l.tree_plen;
    }
    uint32_t lg = l.log_L;
    for (uint32_t k = 0; k < l.n_layers; k++) {
        lg -= arity_bits;
        l.layer_plen[k] = lg > cap_height ? lg - cap_height : 0;   // a tree no taller than its cap: no siblings
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
    l.queries = b;
    l.w_queries = w;
    b += l.query_bytes * n_queries;
    w += l.w_query_words * n_queries;
    words(2 * (size_t)l.final_len, &l.final_poly, &l.w_final_poly);
    words(1, &l.pow_witness, &l.w_pow_witness);
    words(1, &l.n_pis_word, &l.w_n_pis_word);
    words(n_pis, &l.public_inputs, &l.w_public_inputs);
    l.total = b + 8 * tail_words;
    l.w_total = w + tail_words;
    return true;
}

enum : uint32_t { SOUND = 0, BAD_LENGTH = 1, BAD_PUBLIC_INPUT_COUNT = 2, BAD_PATH_LENGTH = 3, BAD_WORD = 4 };

struct Finding {
    uint32_t what = SOUND;
    uint32_t query = 0, tree = 0, layer = 0;   // BAD_PATH_LENGTH: where (tree < n_trees: an initial tree; else a FRI layer)
    size_t word = 0;                           // BAD_WORD: its index in the staging buffer
};

// The first word in staging[a, b) that is not below p, or b
inline size_t first_word_not_below_p(const uint64_t* staging, size_t a, size_t b) {
    for (size_t i = a; i < b; i++)
        if (staging[i] >= FIELD_P) return i;
    return b;
}
// The first word of the first digest in staging[a, b) (whole digests of four words) that is not below r, or b
inline size_t first_digest_not_below_r(const uint64_t* staging, size_t a, size_t b) {
    for (size_t i = a; i + 4 <= b; i += 4)
        if (!bnf::below_mod<bnf::RP>(staging + i)) return i;
    return b;
}

// The word check under HASHER_BN128, in staging order: a digest (the head's caps, the FRI caps, every sibling) must be below r as
// one integer, every other word below p.  The index of the first offender (a digest's first word), or l.w_total.
inline size_t first_bad_word_bn128(const Layout& l, const uint64_t* staging) {
    size_t at = 0, bad;
    // [at, to): field words, then [to, to + n): digests
    auto span = [&](size_t to, size_t n) {
        if ((bad = first_word_not_below_p(staging, at, to)) != to) return false;
        if ((bad = first_digest_not_below_r(staging, to, to + n)) != to + n) return false;
        at = to + n;
        return true;
    };
    if (!span(l.w_head_caps, l.n_head_cap_words)) return bad;
    if (!span(l.w_fri_caps, l.n_layers * l.cap_words)) return bad;
    for (uint32_t q = 0; q < l.n_queries; q++) {
        const size_t q0 = l.w_queries + (size_t)q * l.w_query_words;
        for (uint32_t o = 0; o < l.n_trees; o++)
            if (!span(q0 + l.w_path[o], 4 * (size_t)l.tree_plen)) return bad;
        for (uint32_t k = 0; k < l.n_layers; k++)
            if (!span(q0 + l.w_layer_path[k], 4 * (size_t)l.layer_plen[k])) return bad;
    }
    if (!span(l.w_total, 0)) return bad;
    return l.w_total;
}

// Checks `proof` against the layout and fills `staging` (l.w_total words).  Reads proof[0 .. len) only, and nothing at all unless
// len == l.total; no offset depends on a byte of the proof.  The first finding wins, in the order of the enum.
inline uint32_t parse(const Layout& l, const uint8_t* proof, size_t len, uint64_t* staging, Finding* f) {
    *f = Finding();
    if (len != l.total) return f->what = BAD_LENGTH;
    uint64_t n_pis;
    memcpy(&n_pis, proof + l.n_pis_word, 8);
    if (n_pis != l.n_pis) return f->what = BAD_PUBLIC_INPUT_COUNT;
    memcpy(staging, proof, l.queries);
    for (uint32_t q = 0; q < l.n_queries; q++) {
        const uint8_t* qp = proof + l.queries + (size_t)q * l.query_bytes;
        uint64_t* qs = staging + l.w_queries + (size_t)q * l.w_query_words;
        // one tree of the query: its path-length byte against the layout's, its row (or coset) and its siblings
        auto tree = [&](uint32_t t, uint32_t layer, size_t at_len, uint32_t plen, size_t at_row, size_t w_row, size_t row_bytes, size_t at_path,
                        size_t w_path) {
            if (qp[at_len] != plen && f->what == SOUND) {
                f->what = BAD_PATH_LENGTH;
                f->query = q;
                f->tree = t;
                f->layer = layer;
            }
            memcpy(qs + w_row, qp + at_row, row_bytes);
            memcpy(qs + w_path, qp + at_path, 32 * (size_t)plen);
        };
        for (uint32_t o = 0; o < l.n_trees; o++)
            tree(o, 0, l.path_len[o], l.tree_plen, l.row[o], l.w_row[o], 8 * (size_t)l.tree_cols[o], l.path[o], l.w_path[o]);
        for (uint32_t k = 0; k < l.n_layers; k++)
            tree(l.n_trees + k, k, l.layer_path_len[k], l.layer_plen[k], l.layer_evals[k], l.w_layer_evals[k], 16 * (size_t)l.arity,
                 l.layer_path[k], l.w_layer_path[k]);
    }
    memcpy(staging + l.w_final_poly, proof + l.final_poly, l.total - l.final_poly);
    if (f->what != SOUND) return f->what;
    if (l.hasher == HASHER_BN128) {
        const size_t bad = first_bad_word_bn128(l, staging);
        if (bad != l.w_total) {
            f->what = BAD_WORD;
            f->word = bad;
            return f->what;
        }
        return SOUND;
    }
    for (size_t i = 0; i < l.w_total; i++)
        if (staging[i] >= FIELD_P) {   // the proof-of-work witness is a field element too; the count word was compared above
            f->what = BAD_WORD;
            f->word = i;
            return f->what;
        }
    return SOUND;
}

}  // namespace fpl
}  // namespace nlx
