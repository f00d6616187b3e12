// gnark-crypto's bytes on the host, written once: field elements and G1 points to and from big-endian bytes (Marshal, Bytes,
// SetBytes with its square root), fr.Hash and the fiatshamir transcript over SHA-256.  Shared by the PLONK prover
// (bn254_plonk_prove.hip), the Groth16 verifier (bn254_pairing.hip) and the PLONK verifier (bn254_plonk_verify_host.hpp).  Eight-limb
// arithmetic (bn254_fp.hpp) only: builds with plain g++ as well as hipcc.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "bn254_fp.hpp"
#include "sha256_host.hpp"

namespace nlx {
namespace ppr {

using namespace bnf;
typedef Fp<RP> Fr;
typedef Fp<QP> Fq;

// ---- host: field helpers, bytes, transcript ----
inline Fr fr_words(const uint64_t* w) { return load_words<RP>(w); }
inline Fr fr_small(uint64_t x) {
    Fr a = zero<RP>();
    a.v[0] = (uint32_t)x, a.v[1] = (uint32_t)(x >> 32);
    return to_mont(a);
}
// 32 big-endian bytes, any value below 2^256 -> the residue, Montgomery
inline Fr fr_from_be32(const uint8_t* b) {
    Fr a;
    for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)b[31 - 4 * i] | (uint32_t)b[30 - 4 * i] << 8 | (uint32_t)b[29 - 4 * i] << 16 | (uint32_t)b[28 - 4 * i] << 24;
    return to_mont(a);   // the Montgomery product reduces: a < 2^256, R^2 mod r < r
}
template <class P>
inline void be32(const Fp<P>& mont, uint8_t* out) {   // the canonical integer, big-endian
    const Fp<P> c = from_mont(mont);
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[31 - 4 * i - b] = (uint8_t)(c.v[i] >> (8 * b));
}
// G1Affine.Marshal(): x || y big-endian; infinity: 0x40 and zeros
inline void g1_marshal(const uint64_t w[8], uint8_t out[64]) {
    const Fp<QP> x = load_words<QP>(w), y = load_words<QP>(w + 4);
    if (is_zero(x) && is_zero(y)) {
        memset(out, 0, 64);
        out[0] = 0x40;
        return;
    }
    be32(x, out);
    be32(y, out + 32);
}
// G1Affine.Bytes(): x with 0b10 / 0b11 in the top two bits for the smaller / larger y, 0b01 for infinity
inline void g1_compress(const uint64_t w[8], uint8_t out[32]) {
    const Fp<QP> x = load_words<QP>(w), y = load_words<QP>(w + 4);
    if (is_zero(x) && is_zero(y)) {
        memset(out, 0, 32);
        out[0] = 0x40;
        return;
    }
    be32(x, out);
    // y > (q - 1) / 2  <=>  2 y > q - 1  <=>  2 y >= q (q odd, y < q): the doubling of the canonical integer carries past q
    const Fp<QP> c = from_mont(y);
    uint32_t d[9];
    uint32_t carry = 0;
    for (int i = 0; i < 8; i++) {
        d[i] = (c.v[i] << 1) | carry;
        carry = c.v[i] >> 31;
    }
    d[8] = carry;
    bool larger = d[8] != 0;
    if (!larger) {
        larger = true;   // equal cannot happen (q odd)
        for (int i = 7; i >= 0; i--)
            if (d[i] != QP::mod(i)) {
                larger = d[i] > QP::mod(i);
                break;
            }
    }
    out[0] |= larger ? 0xC0 : 0x80;
}

// gnark-crypto fr.Hash(msg, dst, 1)[0]: expand_message_xmd (RFC 9380) over SHA-256 to 48 bytes, big-endian, mod r
inline Fr hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
    uint8_t b0[32], b1[32], b2[32], x[32];
    const uint8_t zpad[64] = {0}, lib[3] = {0, 48, 0}, dl = (uint8_t)dst_len, i1 = 1, i2 = 2;
    Sha256 h;
    h.update(zpad, 64);
    h.update(msg, len);
    h.update(lib, 3);
    h.update(dst, dst_len);
    h.update(&dl, 1);
    h.final(b0);
    h.reset();
    h.update(b0, 32);
    h.update(&i1, 1);
    h.update(dst, dst_len);
    h.update(&dl, 1);
    h.final(b1);
    for (int i = 0; i < 32; i++) x[i] = b0[i] ^ b1[i];
    h.reset();
    h.update(x, 32);
    h.update(&i2, 1);
    h.update(dst, dst_len);
    h.update(&dl, 1);
    h.final(b2);
    // the 48 bytes b1 || b2[:16] = hi 2^256 + lo with hi = b1[:16], lo = b1[16:] || b2[:16]
    uint8_t hi[32] = {0}, lo[32];
    memcpy(hi + 16, b1, 16);
    memcpy(lo, b1 + 16, 16);
    memcpy(lo + 16, b2, 16);
    Fr r2;
    for (int i = 0; i < 8; i++) r2.v[i] = RP::r2(i);   // as an element: 2^256 mod r
    return add(fr_from_be32(lo), mul(fr_from_be32(hi), r2));
}

// gnark-crypto fiatshamir.Transcript over SHA-256: challenge i hashes its name, the raw bytes of challenge i - 1 and whatever was
// bound to it; the prover derives them in order, so one running hash per challenge is all the state there is
struct Challenge {
    Sha256 h;
    uint8_t raw[32];
    Challenge(const char* name, const Challenge* prev) {
        h.update(name, strlen(name));
        if (prev) h.update(prev->raw, 32);
    }
    void bind_point(const uint64_t w[8]) {
        uint8_t b[64];
        g1_marshal(w, b);
        h.update(b, 64);
    }
    void bind_fr(const Fr& x) {
        uint8_t b[32];
        be32(x, b);
        h.update(b, 32);
    }
    Fr value() {
        h.final(raw);
        return fr_from_be32(raw);
    }
};

// ---- decoding gnark-crypto's compressed points ----
template <class P>
inline Fp<P> pow_limbs(const Fp<P>& a, const uint32_t e[8]) {
    Fp<P> r = one<P>();
    for (int bit = 255; bit >= 0; bit--) {
        r = sqr(r);
        if ((e[bit >> 5] >> (bit & 31)) & 1) r = mul(r, a);
    }
    return r;
}
// a square root in Fq (q = 3 mod 4: a^((q + 1) / 4)), false if there is none
inline bool fq_sqrt(const Fq& a, Fq& out) {
    uint32_t e[8];
    uint64_t c = 1;
    for (int i = 0; i < 8; i++) {   // q + 1
        c += QP::mod(i);
        e[i] = (uint32_t)c;
        c >>= 32;
    }
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> 2) | (i < 7 ? e[i + 1] << 30 : 0);
    out = pow_limbs<QP>(a, e);
    return equal(sqr(out), a);
}
// 32 big-endian bytes (the top two bits dropped with `mask`) -> an element; false if the integer is not below q
inline bool fq_from_be(const uint8_t* b, bool mask, Fq& out) {
    Fq x;
    for (int i = 0; i < 8; i++) {
        const uint8_t* p = b + 28 - 4 * i;
        uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
        if (i == 7 && mask) w &= 0x3FFFFFFFu;
        x.v[i] = w;
    }
    if (geq_mod(x)) return false;
    out = to_mont(x);
    return true;
}
// gnark-crypto's "lexicographically largest": y > (q - 1) / 2, i.e. y > -y as integers
inline bool lex_largest(const Fq& y) {
    const Fq a = from_mont(y), b = from_mont(neg(y));
    for (int i = 7; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
    return false;
}
inline bool rest_zero(const uint8_t* b, size_t n) {
    uint8_t o = 0;
    for (size_t i = 1; i < n; i++) o |= b[i];
    return o == 0;
}
// G1Affine.SetBytes on 32 bytes: words (all zero for the point at infinity); false: malformed
inline bool g1_decode(const uint8_t* b, uint64_t w[8]) {
    memset(w, 0, 64);
    const unsigned flag = b[0] >> 6;
    if (flag == 1) return b[0] == 0x40 && rest_zero(b, 32);
    if (flag == 0) return false;
    Fq x, y;
    if (!fq_from_be(b, true, x)) return false;
    const Fq one_ = one<QP>(), three = add(one_, add(one_, one_));
    if (!fq_sqrt(add(mul(sqr(x), x), three), y)) return false;
    if (lex_largest(y) != (flag == 3)) y = neg(y);
    store_words(x, w);
    store_words(y, w + 4);
    return true;
}
// a canonical integer below r as 32 big-endian bytes
inline void fr_to_be(const Fr& canonical, uint8_t* b) {
    for (int i = 0; i < 8; i++) {
        uint8_t* p = b + 28 - 4 * i;
        p[0] = (uint8_t)(canonical.v[i] >> 24); p[1] = (uint8_t)(canonical.v[i] >> 16); p[2] = (uint8_t)(canonical.v[i] >> 8); p[3] = (uint8_t)canonical.v[i];
    }
}

}  // namespace ppr
}  // namespace nlx
