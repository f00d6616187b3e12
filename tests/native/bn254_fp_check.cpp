// Host build of the eight-limb Montgomery arithmetic of BN254 (csrc/bn254_fp.hpp; base field q and scalar field r: the MSM's
// tail, the NTT's tables, the Groth16 rows, every range check of a caller's scalars): reads "modulus op A B" lines (hexadecimal
// integers below 2^256; B is the 64-bit exponent of "pow"), prints the result as a hexadecimal integer.
// tests/test_bn254_model.py checks every answer with Python integers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bn254_fp.hpp"

using namespace nlx::bnf;

static void parse(const char* hex, uint64_t w[4]) {
    for (int i = 0; i < 4; i++) w[i] = 0;
    const size_t len = strlen(hex);
    for (size_t i = 0; i < len && i < 64; i++) {
        const char ch = hex[len - 1 - i];
        const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        w[i / 16] |= d << (4 * (i % 16));
    }
}
template <class P>
static void print(const Fp<P>& a) {
    uint64_t w[4];
    store_words(a, w);
    printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]);
}

template <class P>
static int run(const char* op, const uint64_t* a, const uint64_t* b) {
    const Fp<P> x = load_words<P>(a), y = load_words<P>(b);
    if (!strcmp(op, "add")) print(add(x, y));
    else if (!strcmp(op, "sub")) print(sub(x, y));
    else if (!strcmp(op, "neg")) print(neg(x));
    else if (!strcmp(op, "mul")) print(mul(x, y));
    else if (!strcmp(op, "tomont")) print(to_mont(x));
    else if (!strcmp(op, "frommont")) print(from_mont(x));
    else if (!strcmp(op, "inv")) print(inv_host(x));
    else if (!strcmp(op, "pow")) print(pow_host(x, b[0]));
    else if (!strcmp(op, "below")) {
        if (below_mod<P>(a) == geq_mod(x)) return 3;   // the comparison on words and the one on limbs are one predicate
        printf("%d\n", below_mod<P>(a) ? 1 : 0);
    }
    else return 2;
    return 0;
}

int main() {   // lines: modulus ("q" | "r") op A B
    char mod[8], op[32], a[128], b[128];
    while (scanf("%7s %31s %127s %127s", mod, op, a, b) == 4) {
        uint64_t x[4], y[4];
        parse(a, x);
        parse(b, y);
        const int rc = mod[0] == 'q' ? run<QP>(op, x, y) : run<RP>(op, x, y);
        if (rc) return rc;
    }
    return 0;
}
