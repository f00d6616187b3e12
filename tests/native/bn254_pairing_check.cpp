// Host build of the BN254 pairing (csrc/bn254_pairing.hpp: the Fq12 tower, the Miller loop, the final exponentiation, the G2
// subgroup test) from the header alone.  Reads cases from the file named on the command line, one per line:
//     op  operand ... = expected ...
// every number a hexadecimal integer below 2^256.  Operands are Montgomery words (x 2^256 mod q, what the library's callers
// hand over); expected Fq12 values are the twelve canonical integers in E12 order.  tests/test_bn254_pairing_native_cpu.py
// writes the cases from tools/bn254_pairing_model.py.  Exit status 0: every case agrees; 1: one does not (named on stdout).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "bn254_pairing.hpp"

using namespace nlx::pairing;

typedef std::vector<uint64_t> Words;   // four per number

static bool parse_line(char* line, std::string& op, Words& in, Words& expect) {
    char* tok = strtok(line, " \t\r\n");
    if (!tok) return false;
    op = tok;
    Words* to = &in;
    while ((tok = strtok(nullptr, " \t\r\n"))) {
        if (!strcmp(tok, "=")) {
            to = &expect;
            continue;
        }
        uint64_t w[4] = {0, 0, 0, 0};
        const size_t len = strlen(tok);
        for (size_t i = 0; i < len && i < 64; i++) {
            const char ch = tok[len - 1 - i];
            const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
            w[i / 16] |= d << (4 * (i % 16));
        }
        to->insert(to->end(), w, w + 4);
    }
    return true;
}

static bool same(const Fe12& a, const Words& expect) {
    uint64_t w[48];
    f12_store(a, false, w);
    return expect.size() == 48 && !memcmp(w, expect.data(), sizeof w);
}
// the same value through the Montgomery writer and the reader: what nlx_bn254_pairing hands out is what it takes in
static bool round_trip(const Fe12& a) {
    uint64_t w[48];
    f12_store(a, true, w);
    return f12_eq(f12_load(w), a);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "r");
    if (!fp) return 2;
    std::vector<char> line(1 << 16);
    int n = 0, bad = 0;
    while (fgets(line.data(), (int)line.size(), fp)) {
        std::string op;
        Words in, ex;
        if (!parse_line(line.data(), op, in, ex)) continue;
        n++;
        bool ok = false;
        const uint64_t* a = in.data();
        if (op == "mul" && in.size() == 96) ok = same(f12_mul(f12_load(a), f12_load(a + 48)), ex);
        else if (op == "sqr" && in.size() == 48) ok = same(f12_sqr(f12_load(a)), ex) && round_trip(f12_sqr(f12_load(a)));
        else if (op == "inv" && in.size() == 48) ok = same(f12_inv(f12_load(a)), ex);
        else if (op == "conj" && in.size() == 48) ok = same(f12_conj(f12_load(a)), ex);
        else if (op == "frob1" && in.size() == 48) ok = same(f12_frobenius<1>(f12_load(a)), ex);
        else if (op == "frob2" && in.size() == 48) ok = same(f12_frobenius<2>(f12_load(a)), ex);
        else if (op == "frob3" && in.size() == 48) ok = same(f12_frobenius<3>(f12_load(a)), ex);
        else if (op == "cyc" && in.size() == 48) ok = same(f12_cyclotomic_sqr(f12_load(a)), ex);
        else if (op == "expx" && in.size() == 48) ok = same(f12_exp_by_x(f12_load(a)), ex);
        else if (op == "finalexp" && in.size() == 48) ok = same(final_exponentiation(f12_load(a)), ex);
        else if (op == "line" && in.size() == 48 + 24) {   // a, then l0 l1 l2 as six Fq
            uint32_t v[48];
            for (int i = 0; i < 24; i++) {
                v[2 * i] = (uint32_t)a[48 + i];
                v[2 * i + 1] = (uint32_t)(a[48 + i] >> 32);
            }
            ok = same(f12_mul_by_line(f12_load(a), F2::from_mont256(v), F2::from_mont256(v + 16), F2::from_mont256(v + 32)), ex);
        } else if (op == "pairing" && in.size() == 8 + 16) {
            ok = same(final_exponentiation(miller_loop(g1_load(a), g2_load(a + 8))), ex);
        } else if (op == "miller" && in.size() == 8 + 16 + 48) {
            // the lines are scaled by factors in Fq2, so the Miller value is the model's up to one: the quotient must lie in Fq2
            const Fe12 f = miller_loop(g1_load(a), g2_load(a + 8));
            uint64_t w[48];
            f12_store(f12_mul(f, f12_inv(f12_load(a + 24))), false, w);
            uint64_t rest = 0, head = 0;
            for (int i = 0; i < 8; i++) head |= w[i];
            for (int i = 8; i < 48; i++) rest |= w[i];
            ok = head != 0 && rest == 0;
        } else if (op == "miller_is_one" && in.size() == 8 + 16) {
            ok = f12_eq(miller_loop(g1_load(a), g2_load(a + 8)), f12_one());
        } else if (op == "check" && in.size() == 8 + 16 && ex.size() == 4) {
            ok = check_pair(a, a + 8) == (uint32_t)ex[0];
        } else {
            printf("case %d: unknown op or operand count: %s (%zu)\n", n, op.c_str(), in.size());
            bad++;
            continue;
        }
        if (!ok) {
            printf("case %d: %s disagrees\n", n, op.c_str());
            bad++;
        }
    }
    fclose(fp);
    printf("%d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
