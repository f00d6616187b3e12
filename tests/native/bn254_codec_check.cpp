// Host build of the BN254 point codec (csrc/bn254_codec.hpp: the square roots in Fq and Fq2, the "largest" rule, gnark-crypto's
// point bytes both ways) from the header alone.  Reads cases from the file named on the command line, one per line:
//     op  operand ... = expected ...
// every number a hexadecimal integer below 2^256.  Field operands are Montgomery words (x 2^256 mod q); a point's bytes are given
// 32 at a time, each chunk as the big-endian integer it spells.  tests/test_bn254_codec_native_cpu.py writes the cases from
// tools/gnark_bytes_model.py.  Exit status 0: every case agrees; 1: one does not (named on stdout).
//   sqrt a = exists y            y: the canonical root that is not "largest" (0 where there is none)
//   sqrt2 a0 a1 = exists y0 y1   the same over Fq2
//   largest y = 0|1              largest2 y0 y1 = 0|1
//   g1dec raw chunk.. = status X Y             g2dec raw subgroup chunk.. = status X.A0 X.A1 Y.A0 Y.A1   (words as integers)
//   g1enc raw X Y = status chunk..             g2enc raw X.A0 X.A1 Y.A0 Y.A1 = status chunk..
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "bn254_codec.hpp"

using namespace nlx;
using namespace nlx::codec;

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

static f29::Fe load_fq(const uint64_t* w) {
    uint32_t v[8];
    for (int i = 0; i < 4; i++) {
        v[2 * i] = (uint32_t)w[i];
        v[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return f29::tighten<QM>(f29::from_mont256<QM>(v));
}
static bool canonical_is(const f29::Fe& a, const uint64_t* expect) {
    uint64_t w[4];
    pairing::fq_store(a, false, w);
    return !memcmp(w, expect, 32);
}
// number k of a case -> 32 big-endian bytes as eight native words of memory
static void chunk_to_memory(const uint64_t* number, uint32_t* m) {
    uint8_t b[32];
    for (int i = 0; i < 32; i++) b[31 - i] = (uint8_t)(number[i / 8] >> (8 * (i % 8)));
    memcpy(m, b, 32);
}
static bool memory_is(const uint32_t* m, const uint64_t* number) {
    uint32_t want[8];
    chunk_to_memory(number, want);
    return !memcmp(m, want, 32);
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
        const size_t ni = in.size() / 4, ne = ex.size() / 4;
        if (op == "sqrt" && ni == 1 && ne == 2) {
            f29::Fe y;
            const bool exists = fq_sqrt(load_fq(a), y);
            uint32_t yc[8];
            f29::to_canonical256<QM>(y, yc);
            if (limbs_largest(yc)) y = fq_neg(y);
            ok = exists == (ex[0] != 0) && (!exists || canonical_is(y, &ex[4]));
        } else if (op == "sqrt2" && ni == 2 && ne == 3) {
            f29::Fe2 y;
            const bool exists = f2_sqrt(f29::Fe2{load_fq(a), load_fq(a + 4)}, y);
            if (exists && f2_largest(y)) y = f2_neg_tight(y);
            ok = exists == (ex[0] != 0) && (!exists || (canonical_is(y.c0, &ex[4]) && canonical_is(y.c1, &ex[8])));
        } else if (op == "largest" && ni == 1 && ne == 1) {
            uint32_t yc[8];
            f29::to_canonical256<QM>(load_fq(a), yc);
            ok = limbs_largest(yc) == (ex[0] != 0);
        } else if (op == "largest2" && ni == 2 && ne == 1) {
            ok = f2_largest(f29::Fe2{load_fq(a), load_fq(a + 4)}) == (ex[0] != 0);
        } else if ((op == "g1dec" || op == "g2dec") && ni >= 2) {
            const bool g2 = op == "g2dec", raw = a[0] != 0;
            const size_t head = g2 ? 2 : 1, chunks = (g2 ? 2 : 1) * (raw ? 2 : 1), words = g2 ? 16 : 8;
            if (ni != head + chunks || ne != 1 + words / 4) {
                printf("case %d: %s: operand count\n", n, op.c_str());
                bad++;
                continue;
            }
            uint32_t m[32];
            uint64_t out[16];
            for (size_t k = 0; k < chunks; k++) chunk_to_memory(a + 4 * (head + k), m + 8 * k);
            const uint32_t st = g2 ? g2_decode(m, raw, a[4] != 0, out) : g1_decode(m, raw, out);
            ok = st == (uint32_t)ex[0] && !memcmp(out, &ex[4], words * 8);
        } else if ((op == "g1enc" || op == "g2enc") && ni >= 3) {
            const bool g2 = op == "g2enc", raw = a[0] != 0;
            const size_t chunks = (g2 ? 2 : 1) * (raw ? 2 : 1), words = g2 ? 16 : 8;
            if (ni != 1 + words / 4 || ne != 1 + chunks) {
                printf("case %d: %s: operand count\n", n, op.c_str());
                bad++;
                continue;
            }
            uint32_t m[32];
            const uint32_t st = g2 ? g2_encode(a + 4, raw, m) : g1_encode(a + 4, raw, m);
            ok = st == (uint32_t)ex[0];
            for (size_t k = 0; k < chunks; k++) ok = ok && memory_is(m + 8 * k, &ex[4 * (1 + k)]);
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
