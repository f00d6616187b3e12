// Stand-alone driver of the proof parser's digest-word rule (host only: csrc/plonk_proof_layout.hpp over csrc/fri_proof_layout.hpp),
// built with -fsanitize=address,undefined by tests/test_plonk_verify_bn128_cpu.py.  Under HASHER_BN128 the head's caps, the FRI
// caps and every path sibling are digests - four little-endian words of one integer that must be below BN254's r - and every other
// word a field element below p; under HASHER_GOLDILOCKS every word is a field element, as before the hasher existed.  The parser
// runs in BOTH modes on a proof file, on every truncation of it to a multiple of 8 bytes and to one byte either side, and on
// seeded mutations: one byte xor-ed, or a whole word set to all ones.  Every input is an exact-size heap copy and the staging
// buffer has exactly w_total words, so a read or a write past either end is reported.
//
//   digest_words_check PROOF SEED N_MUTATIONS degree_bits rate_bits cap_height arity_bits final_poly_bits n_queries n_pis
//                      n_constants n_sigmas n_wires n_challenges n_partial n_lookup_polys n_quotient
// Prints "total <bytes>", "file <goldilocks finding> <bn128 finding>", "truncations <tried> sound <goldilocks> <bn128>", then per
// mutation "mut <offset> <kind> <goldilocks finding> <its word> <bn128 finding> <its word>" (finding: 0 sound, 1 length,
// 2 public-input count, 3 path-length byte, 4 word; kind: the xor-ed byte value, or 256 for the word at <offset> set to all ones).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../near-light-client_amd/csrc/plonk_proof_layout.hpp"

using namespace nlx;

struct Found {
    uint32_t what;
    size_t word;
};

static Found run(const fpl::Layout& l, const uint8_t* src, size_t len) {
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    memcpy(copy, src, len);
    uint64_t* staging = (uint64_t*)malloc(8 * (l.w_total ? l.w_total : 1));
    fpl::Finding f;
    const uint32_t r = fpl::parse(l, copy, len, staging, &f);
    free(staging);
    free(copy);
    return Found{r, f.word};
}

int main(int argc, char** argv) {
    if (argc != 18) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<uint8_t> proof;
    for (int c; (c = fgetc(fh)) != EOF;) proof.push_back((uint8_t)c);
    fclose(fh);
    uint64_t seed = strtoull(argv[2], nullptr, 10);
    const unsigned n_mut = (unsigned)strtoul(argv[3], nullptr, 10);
    ppl::Shape s{};
    uint32_t* fields[] = {&s.degree_bits, &s.rate_bits, &s.cap_height, &s.arity_bits, &s.final_poly_bits, &s.n_queries, &s.n_pis,
                          &s.n_constants, &s.n_sigmas, &s.n_wires, &s.n_challenges, &s.n_partial, &s.n_lookup_polys, &s.n_quotient};
    for (int i = 0; i < 14; i++) *fields[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
    ppl::Layout gl, bn;
    if (!ppl::make_layout(s, &gl) || !ppl::make_layout(s, &bn, fpl::HASHER_BN128)) return 3;
    if (gl.hasher != fpl::HASHER_GOLDILOCKS || bn.hasher != fpl::HASHER_BN128 || gl.total != bn.total || gl.w_total != bn.w_total) return 4;
    printf("total %zu\n", gl.total);
    printf("file %u %u\n", run(gl, proof.data(), proof.size()).what, run(bn, proof.data(), proof.size()).what);
    size_t tried = 0, sound_gl = 0, sound_bn = 0;
    for (size_t t = 0; t < proof.size(); t++) {
        if (t % 8 != 0 && t % 8 != 1 && t % 8 != 7) continue;
        tried++;
        sound_gl += run(gl, proof.data(), t).what == fpl::SOUND;
        sound_bn += run(bn, proof.data(), t).what == fpl::SOUND;
    }
    printf("truncations %zu sound %zu %zu\n", tried, sound_gl, sound_bn);
    std::vector<uint8_t> m(proof);
    for (unsigned k = 0; k < n_mut && proof.size() >= 8; k++) {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;   // Knuth's MMIX generator: the test steps it too
        size_t off = (size_t)((seed >> 16) % proof.size());
        unsigned kind = 1 + (unsigned)((seed >> 56) % 255);
        uint8_t saved[8];
        if (k % 4 == 3) {   // a whole word of ones: the only way a flip of a few bits lifts a digest's top word past r's
            if (off + 8 > proof.size()) off = proof.size() - 8;
            kind = 256;
            memcpy(saved, &m[off], 8);
            memset(&m[off], 0xFF, 8);
        } else {
            saved[0] = m[off];
            m[off] ^= (uint8_t)kind;
        }
        const Found a = run(gl, m.data(), m.size()), b = run(bn, m.data(), m.size());
        printf("mut %zu %u %u %zu %u %zu\n", off, kind, a.what, a.word, b.what, b.word);
        memcpy(&m[off], saved, kind == 256 ? 8 : 1);
    }
    return 0;
}
