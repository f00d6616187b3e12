// Host build of csrc/fe25519_fast.hpp (the arithmetic of the Ed25519 trace generator's scan) at given operands.  Reads one
// operation per line and prints its result on one line; tests/test_ed25519_aims_cpu.py compares with Python integers.
//   F l0 .. l9                freeze: the canonical value, 64 hex digits
//   M a0 .. a9 b0 .. b9       mul: the product's ten carried limbs (decimal), then its canonical value
//   L <64 hex digits>         from_limbs16 of the 256-bit number: ten limbs
//   S a[10] b[10] c[10] d[10] the four-term sums of the scan: limbs and canonical value of a + b + c + d, a - b - c - d,
//                             2 (a + b) and -(a + b) - (c + d), through add, sub, dbl and neg
// Limbs are signed decimals (ten per value, 26 bits apart).  Exit code 2 on a malformed line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fe25519_fast.hpp"

using namespace nlx;

static bool read_fe(char*& p, fe::Fe& v) {
    for (int i = 0; i < 10; i++) {
        char* end;
        v.l[i] = strtoll(p, &end, 10);
        if (end == p) return false;
        p = end;
    }
    return true;
}
static void print_limbs(const fe::Fe& v) {
    for (int i = 0; i < 10; i++) printf("%lld ", (long long)v.l[i]);
}
static void print_frozen(const fe::Fe& v) {
    uint32_t w[16];
    fe::freeze(v, w);
    for (int i = 15; i >= 0; i--) {
        if (w[i] > 0xFFFF) exit(4);   // a limb of the canonical form left its 16 bits
        printf("%04x", w[i]);
    }
}

int main() {
    static char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char* p = line + 1;
        fe::Fe a, b, c, d;
        switch (line[0]) {
            case 'F':
                if (!read_fe(p, a)) return 2;
                print_frozen(a);
                break;
            case 'M': {
                if (!read_fe(p, a) || !read_fe(p, b)) return 2;
                const fe::Fe m = fe::mul(a, b);
                print_limbs(m);
                print_frozen(m);
                break;
            }
            case 'L': {
                char hex[80];
                if (sscanf(p, "%64s", hex) != 1 || strlen(hex) != 64) return 2;
                uint32_t w[16];
                for (int i = 0; i < 16; i++) {
                    unsigned x = 0;
                    if (sscanf(hex + 4 * (15 - i), "%4x", &x) != 1) return 2;
                    w[i] = x;
                }
                print_limbs(fe::from_limbs16(w));
                break;
            }
            case 'S': {
                if (!read_fe(p, a) || !read_fe(p, b) || !read_fe(p, c) || !read_fe(p, d)) return 2;
                const fe::Fe r[4] = {fe::add(fe::add(a, b), fe::add(c, d)), fe::sub(fe::sub(fe::sub(a, b), c), d), fe::dbl(fe::add(a, b)),
                                     fe::sub(fe::neg(fe::add(a, b)), fe::add(c, d))};
                for (int k = 0; k < 4; k++) {
                    print_limbs(r[k]);
                    print_frozen(r[k]);
                    printf(" ");
                }
                break;
            }
            default: return 2;
        }
        printf("\n");
    }
    return 0;
}
