// Stand-alone driver of the proof layout headers (host only: csrc/fri_proof_layout.hpp and the two formats on top of it), built
// with -fsanitize=address,undefined by tests/test_stark_verify_cpu.py and tests/test_plonk_verify_cpu.py: the one proof parser
// on a proof file, on every truncation of it to a multiple of 8 bytes and to one byte either side, and on seeded single-byte
// mutations.  Every input is an exact-size heap copy and the staging buffer has exactly w_total words, so a read or a write past
// either end is reported.
//
//   layout_check stark PROOF SEED N_MUTATIONS degree_bits rate_bits cap_height arity_bits final_poly_bits n_queries n_cols nq
//                      n_pis n_round_values oracle_cols...
//   layout_check plonk PROOF SEED N_MUTATIONS degree_bits rate_bits cap_height arity_bits final_poly_bits n_queries n_pis
//                      n_constants n_sigmas n_wires n_challenges n_partial n_lookup_polys n_quotient
// Prints  "total <bytes>", "file <finding>", "truncations <tried> sound <how many were called sound>", then
// "mut <offset> <xor> <finding>" per mutation (finding: 0 sound, 1 length, 2 public-input count, 3 path-length byte, 4 word >= p).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../near-light-client_amd/csrc/plonk_proof_layout.hpp"
#include "../../near-light-client_amd/csrc/stark_proof_layout.hpp"

using namespace nlx;

static uint32_t run(const fpl::Layout& l, const uint8_t* src, size_t len) {
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    memcpy(copy, src, len);
    uint64_t* staging = (uint64_t*)malloc(8 * (l.w_total ? l.w_total : 1));
    fpl::Finding f;
    const uint32_t r = fpl::parse(l, copy, len, staging, &f);
    free(staging);
    free(copy);
    return r;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const bool stark = !strcmp(argv[1], "stark");
    if (!stark && strcmp(argv[1], "plonk")) return 2;
    if (stark ? argc < 16 : argc != 19) return 2;
    FILE* fh = fopen(argv[2], "rb");
    if (!fh) return 2;
    std::vector<uint8_t> proof;
    for (int c; (c = fgetc(fh)) != EOF;) proof.push_back((uint8_t)c);
    fclose(fh);
    uint64_t seed = strtoull(argv[3], nullptr, 10);
    const unsigned n_mut = (unsigned)strtoul(argv[4], nullptr, 10);
    auto arg = [&](int i) { return (uint32_t)strtoul(argv[5 + i], nullptr, 10); };
    spl::Layout sl;
    ppl::Layout pl;
    const fpl::Layout* lay;
    if (stark) {
        spl::Shape s{};
        uint32_t* fields[] = {&s.degree_bits, &s.rate_bits, &s.cap_height, &s.arity_bits, &s.final_poly_bits, &s.n_queries,
                              &s.n_cols, &s.nq, &s.n_pis, &s.n_round_values};
        for (int i = 0; i < 10; i++) *fields[i] = arg(i);
        for (int i = 10; 5 + i < argc && s.n_oracles < spl::MAX_ORACLES; i++) s.oracle_cols[s.n_oracles++] = arg(i);
        if (!spl::make_layout(s, &sl)) return 3;
        lay = &sl;
    } else {
        ppl::Shape s{};
        uint32_t* fields[] = {&s.degree_bits, &s.rate_bits, &s.cap_height, &s.arity_bits, &s.final_poly_bits, &s.n_queries, &s.n_pis,
                              &s.n_constants, &s.n_sigmas, &s.n_wires, &s.n_challenges, &s.n_partial, &s.n_lookup_polys, &s.n_quotient};
        for (int i = 0; i < 14; i++) *fields[i] = arg(i);
        if (!ppl::make_layout(s, &pl)) return 3;
        lay = &pl;
    }
    const fpl::Layout& l = *lay;
    printf("total %zu\n", l.total);
    printf("file %u\n", run(l, proof.data(), proof.size()));
    size_t tried = 0, sound = 0;
    for (size_t t = 0; t < proof.size(); t++) {
        if (t % 8 != 0 && t % 8 != 1 && t % 8 != 7) continue;
        tried++;
        sound += run(l, proof.data(), t) == fpl::SOUND;
    }
    printf("truncations %zu sound %zu\n", tried, sound);
    std::vector<uint8_t> m(proof);
    for (unsigned k = 0; k < n_mut && !proof.empty(); k++) {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;   // Knuth's MMIX generator: the tests step it too
        const size_t off = (size_t)((seed >> 16) % proof.size());
        const uint8_t x = (uint8_t)(1 + (seed >> 56) % 255);
        m[off] ^= x;
        printf("mut %zu %u %u\n", off, (unsigned)x, run(l, m.data(), m.size()));
        m[off] ^= x;
    }
    return 0;
}
