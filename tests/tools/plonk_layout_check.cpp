// Stand-alone driver of csrc/plonk_proof_layout.hpp (host only), built with -fsanitize=address,undefined by
// tests/test_plonk_verify_cpu.py: the proof parser on a proof file, on every truncation of it to a multiple of 8 bytes and to one
// byte either side, and on seeded single-byte mutations.  Every input is an exact-size heap copy and the staging buffer has
// exactly w_total words, so a read or a write past either end is reported.
//
//   plonk_layout_check PROOF SEED N_MUTATIONS degree_bits rate_bits cap_height arity_bits final_poly_bits n_queries n_pis
//                      n_constants n_sigmas n_wires n_challenges n_partial n_lookup_polys n_quotient
// Prints  "total <bytes>", "file <finding>", "truncations <tried> sound <how many were called sound>", then
// "mut <offset> <xor> <finding>" per mutation (finding: 0 sound, 1 length, 2 public-input count, 3 path-length byte, 4 word >= p).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../near-light-client_amd/csrc/plonk_proof_layout.hpp"

using namespace nlx::ppl;

static uint32_t run(const Layout& l, const uint8_t* src, size_t len) {
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    memcpy(copy, src, len);
    uint64_t* staging = (uint64_t*)malloc(8 * (l.w_total ? l.w_total : 1));
    Finding f;
    const uint32_t r = parse(l, copy, len, staging, &f);
    free(staging);
    free(copy);
    return r;
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
    Shape s{};
    uint32_t* fields[] = {&s.degree_bits, &s.rate_bits, &s.cap_height, &s.arity_bits, &s.final_poly_bits, &s.n_queries, &s.n_pis,
                          &s.n_constants, &s.n_sigmas, &s.n_wires, &s.n_challenges, &s.n_partial, &s.n_lookup_polys, &s.n_quotient};
    for (int i = 0; i < 14; i++) *fields[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
    Layout l;
    if (!make_layout(s, &l)) return 3;
    printf("total %zu\n", l.total);
    printf("file %u\n", run(l, proof.data(), proof.size()));
    size_t tried = 0, sound = 0;
    for (size_t t = 0; t < proof.size(); t++) {
        if (t % 8 != 0 && t % 8 != 1 && t % 8 != 7) continue;
        tried++;
        sound += run(l, proof.data(), t) == SOUND;
    }
    printf("truncations %zu sound %zu\n", tried, sound);
    std::vector<uint8_t> m(proof);
    for (unsigned k = 0; k < n_mut && !proof.empty(); k++) {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;   // Knuth's MMIX generator: the test steps it too
        const size_t off = (size_t)((seed >> 16) % proof.size());
        const uint8_t x = (uint8_t)(1 + (seed >> 56) % 255);
        m[off] ^= x;
        printf("mut %zu %u %u\n", off, (unsigned)x, run(l, m.data(), m.size()));
        m[off] ^= x;
    }
    return 0;
}
