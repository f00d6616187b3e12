// The host half of the PLONK verifier (csrc/bn254_plonk_verify_host.hpp) built with plain g++ and run against vectors the
// big-integer model writes (tests/test_bn254_plonk_verify_host_native_cpu.py): decoding and the verdict's index, the transcript's
// four challenges, the scalars of the two combinations, the algebraic relation, gamma' and lambda.
//   key   log_n n_public k k1 k2 [row]*k [point]*(9 + k)          compressed points: the 8 + k commitments, then G
//   proof HEX [public]*n_public = reason index [gamma beta alpha zeta zn2 sc_z sc_s3]     the scalars only when reason = 0
//   fold  FOLDED_H LIN = gamma' lambda v_f scalar_of_G scalar_of_H_z n_terms
// Scalars are canonical integers, 64 hex digits.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "bn254_plonk_verify_host.hpp"

using namespace nlx;
using pvh::Fr;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
static std::string hex_of(const Fr& canonical) {
    uint8_t b[32];
    ppr::fr_to_be(canonical, b);
    char buf[65];
    for (int i = 0; i < 32; i++) snprintf(buf + 2 * i, 3, "%02x", b[i]);
    return std::string(buf, 64);
}
static Fr fr_of(const std::string& s) {   // canonical hex -> Montgomery
    const std::vector<uint8_t> b = unhex(s);
    return ppr::fr_from_be32(b.data());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    pvh::Key key;
    pvh::Proof proof;
    size_t cases = 0, bad = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op, tok;
        ss >> op;
        std::vector<std::string> args, want;
        bool after = false;
        while (ss >> tok) {
            if (tok == "=") after = true;
            else (after ? want : args).push_back(tok);
        }
        std::vector<std::string> got;
        if (op == "key") {
            key = pvh::Key();
            key.log_n = (uint32_t)std::stoul(args[0]), key.n_public = (uint32_t)std::stoul(args[1]), key.k = (uint32_t)std::stoul(args[2]);
            key.k1 = fr_of(args[3]), key.k2 = fr_of(args[4]);
            for (uint32_t j = 0; j < key.k; j++) key.commit_rows[j] = (uint32_t)std::stoul(args[5 + j]);
            for (uint32_t i = 0; i < 9 + key.k; i++)
                if (!ppr::g1_decode(unhex(args[5 + key.k + i]).data(), key.points + 8 * i)) bad++;
        } else if (op == "proof") {
            const std::vector<uint8_t> bytes = unhex(args[0]);
            std::vector<Fr> publics;
            for (uint32_t i = 0; i < key.n_public; i++) publics.push_back(fr_of(args[1 + i]));
            proof = pvh::Proof();
            pvh::decode(key, bytes.data(), bytes.size(), proof);
            if (!proof.rejected()) pvh::relation(key, publics.data(), proof);
            got.push_back(std::to_string(proof.reason));
            got.push_back(std::to_string(proof.index));
            if (!proof.rejected()) {
                for (const Fr* x : {&proof.gamma, &proof.beta, &proof.alpha, &proof.zeta}) got.push_back(hex_of(bnf::from_mont(*x)));
                got.push_back(hex_of(proof.a0[1].scalar));
                got.push_back(hex_of(proof.a1[5].scalar));
                got.push_back(hex_of(proof.a1[6].scalar));
            }
        } else if (op == "fold") {
            uint64_t fh[8], lin[8];
            if (!ppr::g1_decode(unhex(args[0]).data(), fh) || !ppr::g1_decode(unhex(args[1]).data(), lin)) bad++;
            pvh::fold(key, fh, lin, proof);
            for (const Fr* x : {&proof.gp, &proof.lambda, &proof.vf}) got.push_back(hex_of(bnf::from_mont(*x)));
            got.push_back(hex_of(proof.b0[proof.b0.size() - 3].scalar));
            got.push_back(hex_of(proof.b0.back().scalar));
            got.push_back(std::to_string(proof.b0.size() + proof.b1.size()));
        } else {
            std::cout << "unknown op " << op << "\n";
            bad++;
        }
        cases++;
        if (got != want) {
            bad++;
            std::cout << "case " << cases << " (" << op << "): got";
            for (const std::string& g : got) std::cout << " " << g;
            std::cout << "\n want";
            for (const std::string& w : want) std::cout << " " << w;
            std::cout << "\n";
        }
    }
    std::cout << cases << " cases, " << bad << " bad\n";
    return bad ? 1 : 0;
}
