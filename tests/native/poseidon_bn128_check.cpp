// Host build of the PoseidonBN128 permutation (csrc/poseidon_bn128.hpp, the arithmetic of csrc/poseidon_bn128.hip).
// Reads lines from stdin, one operation each; tests/test_poseidon_bn128_cpu.py checks every answer with Python integers:
//   perm A0 A1 A2 A3     four integers below 2^256 (hexadecimal) -> the permutation of their residues, four canonical integers
//   dot4 I S0 S1 S2 S3   row I of the MDS product on raw limb values below 2^258 -> the raw result and whether it is < 2^255
//   sbox X               x^5 (Montgomery) on a raw value below 2^257.5 -> the raw result and whether it is < 2^255
//   conv A               integer below 2^256 -> Montgomery form -> canonical integer (A mod r)
//   trace A0 A1 A2 A3    as perm, then the largest raw value over all 64 rounds at each point of a round (the state on entry,
//                        after the constants, the S-box outputs, after the MDS rows: pbn::permute's observer stages) and
//                        whether every limb 0..7 stayed below 2^29, so the header's bounds can be asserted mid-permutation
#include <cstdio>
#include <cstring>
#include <string>
#include "poseidon_bn128.hpp"

using namespace nlx;
using f29::Fe;

static Fe parse(const char* hex) {   // integer -> limbs by bit slicing (limbs 0..7 < 2^29, limb 8 the rest)
    unsigned char bits[272] = {0};
    const size_t len = strlen(hex);
    for (size_t i = 0; i < len; i++) {
        const char ch = hex[len - 1 - i];
        const int d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        for (int b = 0; b < 4; b++)
            if (4 * i + b < 272) bits[4 * i + b] = (d >> b) & 1;
    }
    Fe r = f29::zero();
    for (int i = 0; i < f29::NL; i++)
        for (int b = 0; b < (i == f29::NL - 1 ? 32 : f29::LB); b++)
            if (f29::LB * i + b < 272 && bits[f29::LB * i + b]) r.v[i] |= 1u << b;
    return r;
}
static void words_of(const char* hex, uint64_t* w) {   // integer < 2^256 -> four little-endian words
    uint32_t x[8];
    f29::to_words256(parse(hex), x);
    for (int k = 0; k < 4; k++) w[k] = (uint64_t)x[2 * k] | ((uint64_t)x[2 * k + 1] << 32);
}
static void print_raw(const Fe& a, bool bound_ok) {   // sum v[i] 2^(29 i) as hex
    unsigned char bits[300] = {0};
    for (int i = 0; i < f29::NL; i++)
        for (int b = 0; b < 32; b++) {
            if (!((a.v[i] >> b) & 1)) continue;
            int pos = f29::LB * i + b;
            while (bits[pos]) bits[pos++] = 0;
            bits[pos] = 1;
        }
    bool limbs_ok = true;
    for (int i = 0; i < f29::NL - 1; i++) limbs_ok = limbs_ok && a.v[i] <= f29::MASK;
    std::string s;
    for (int nib = 74; nib >= 0; nib--) {
        int d = 0;
        for (int b = 0; b < 4; b++) d |= bits[4 * nib + b] << b;
        s += "0123456789abcdef"[d];
    }
    printf("%s %d\n", s.c_str(), (int)(bound_ok && limbs_ok));
}
static bool below_2_255(const Fe& a) { return a.v[f29::NL - 1] < (1u << (255 - 29 * 8)); }   // limbs 0..7 < 2^29
// the raw integer sum v[i] 2^(29 i) as five little-endian words, and a < b on that integer
static void raw_words(const Fe& a, uint64_t (&w)[5]) {
    for (int k = 0; k < 5; k++) w[k] = 0;
    for (int i = 0; i < f29::NL; i++) {
        const int pos = f29::LB * i, k = pos / 64, sh = pos % 64;
        const uint64_t lo = (uint64_t)a.v[i] << sh, hi = sh ? (uint64_t)a.v[i] >> (64 - sh) : 0;
        w[k] += lo;
        uint64_t c = (w[k] < lo) + hi;
        for (int j = k + 1; j < 5 && c; j++) {
            w[j] += c;
            c = w[j] < c;
        }
    }
}
static void keep_max(const Fe& a, uint64_t (&best)[5], bool& limbs_ok) {
    uint64_t w[5];
    raw_words(a, w);
    for (int k = 4; k >= 0; k--)
        if (w[k] != best[k]) {
            if (w[k] > best[k])
                for (int j = 0; j < 5; j++) best[j] = w[j];
            break;
        }
    for (int i = 0; i < f29::NL - 1; i++) limbs_ok = limbs_ok && a.v[i] <= f29::MASK;
}
static void print_words(const uint64_t* w) {
    for (int k = 3; k >= 0; k--) printf("%016llx", (unsigned long long)w[k]);
}

int main() {
    char op[16], a[4][128];
    while (scanf("%15s", op) == 1) {
        if (!strcmp(op, "perm")) {
            if (scanf("%127s %127s %127s %127s", a[0], a[1], a[2], a[3]) != 4) return 2;
            Fe s[pbn::T];
            for (int i = 0; i < pbn::T; i++) {
                uint64_t w[4];
                words_of(a[i], w);
                s[i] = pbn::from_words(w[0], w[1], w[2], w[3]);
            }
            pbn::permute(s);
            for (int i = 0; i < pbn::T; i++) {
                uint64_t w[4];
                pbn::to_words(s[i], w);
                print_words(w);
                printf(i + 1 < pbn::T ? " " : "\n");
            }
        } else if (!strcmp(op, "trace")) {
            if (scanf("%127s %127s %127s %127s", a[0], a[1], a[2], a[3]) != 4) return 2;
            Fe s[pbn::T];
            for (int i = 0; i < pbn::T; i++) {
                uint64_t w[4];
                words_of(a[i], w);
                s[i] = pbn::from_words(w[0], w[1], w[2], w[3]);
            }
            uint64_t mx[4][5] = {};
            bool limbs_ok = true;
            pbn::permute(s, [&](int stage, const Fe& v) { keep_max(v, mx[stage], limbs_ok); });
            for (int i = 0; i < pbn::T; i++) {
                uint64_t w[4];
                pbn::to_words(s[i], w);
                print_words(w);
                printf(" ");
            }
            for (int p = 0; p < 4; p++) {
                for (int k = 4; k >= 0; k--) printf("%016llx", (unsigned long long)mx[p][k]);
                printf(" ");
            }
            printf("%d\n", (int)limbs_ok);
        } else if (!strcmp(op, "dot4")) {
            int row;
            if (scanf("%d %127s %127s %127s %127s", &row, a[0], a[1], a[2], a[3]) != 5) return 2;
            Fe s[pbn::T];
            for (int i = 0; i < pbn::T; i++) s[i] = parse(a[i]);
            const Fe r = pbn::dot4(row, s);
            print_raw(r, below_2_255(r));
        } else if (!strcmp(op, "sbox")) {
            if (scanf("%127s", a[0]) != 1) return 2;
            const Fe r = pbn::sbox(parse(a[0]));
            print_raw(r, below_2_255(r));
        } else if (!strcmp(op, "conv")) {
            if (scanf("%127s", a[0]) != 1) return 2;
            uint64_t w[4], o[4];
            words_of(a[0], w);
            const Fe m = pbn::from_words(w[0], w[1], w[2], w[3]);
            pbn::to_words(m, o);
            print_words(o);
            printf(" %d\n", (int)below_2_255(m));
        } else {
            return 2;
        }
    }
    return 0;
}
