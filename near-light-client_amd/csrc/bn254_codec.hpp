// gnark-crypto's point bytes on the kernels' field: G1Affine / G2Affine Bytes() (compressed, 32 / 64 bytes), RawBytes() (64 / 128)
// and SetBytes with its square roots, one point per call - host and device source in the manner of bn254_pairing.hpp (SURVEY.md
// §8 row f.4).  Builds with plain g++ (tests/native/bn254_codec_check.cpp) and is compared there with the
// big-integer model tools/gnark_bytes_model.py, the place of record for every rule named below.
//
// All arithmetic is bn254_f29.hpp's nine 29-bit limbs (f29::mul, F2 of the curve code, the pairing's cst / g2_in_subgroup /
// fq_store): there is no second field here, only 2^522 mod q, which takes a canonical integer into the form in one product.
//
//   square root in Fq    q = 3 mod 4: w = a^((q - 3) / 4) over the bits of that constant (wave-uniform), y = w a, and y^2 = a
//                        is tested.  w is kept because it is also 1 / y up to the sign chi(a) = y w
//   square root in Fq2   the norm's root s (one chain), t = (a0 + s) / 2 - or (a0 - s) / 2 where that is zero, which only a1 = 0
//                        makes it - and c = t^((q + 1) / 4) (a second chain).  c^2 = t: the root is c + a1 / (2 c) u.  c^2 = -t:
//                        it is a1 / (2 c) + c u.  1 / c is +-w of the second chain, so there is no inversion.  y^2 = a is tested
//                        at the end, which is also what answers "no root".  The model takes another route (a^((q - 3) / 4) in Fq2)
//   bytes                a coordinate's 32 big-endian bytes arrive as eight native 32-bit words of memory (two 16-byte loads on
//                        the device); be_to_limbs reverses them in registers
#pragma once
#include <cstdint>
#include "bn254_pairing.hpp"

namespace nlx {
namespace codec {

using f29::Fe;
using f29::Fe2;
typedef f29::F2 F2;
typedef f29::QMod QM;
typedef bnf::QP QP;

// the status of one point; include/nlx.h's NLX_BN254_POINT_* (held together in bn254_codec.hip)
enum Status : uint32_t { ST_OK = 0, ST_BAD_FLAG = 1, ST_RANGE = 2, ST_BAD_INFINITY = 3, ST_OFF_CURVE = 4, ST_NOT_IN_SUBGROUP = 5 };

// ---- integers as eight 32-bit limbs, little-endian ----
F29_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }
F29_HD void be_to_limbs(const uint32_t* m, uint32_t* w) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[7 - i] = bswap32(m[i]);
}
F29_HD void limbs_to_be(const uint32_t* w, uint32_t* m) {
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = bswap32(w[7 - i]);
}
F29_HD bool limbs_below_q(const uint32_t* w) {
    bool lt = false, eq = true;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt |= eq & (w[i] < QP::mod(i));
        eq &= w[i] == QP::mod(i);
    }
    return lt;
}
// gnark-crypto's "lexicographically largest" on a canonical integer: y > (q - 1) / 2 = q >> 1
F29_HD bool limbs_largest(const uint32_t* w) {
    bool gt = false, eq = true;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const uint32_t h = (QP::mod(i) >> 1) | (i < 7 ? QP::mod(i < 7 ? i + 1 : 7) << 31 : 0u);
        gt |= eq & (w[i] > h);
        eq &= w[i] == h;
    }
    return gt;
}
F29_HD bool limbs_zero(const uint32_t* w) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}

// ---- in and out of the kernels' form ----
// a canonical integer below q -> x 2^261: one product with 2^522 mod q
F29_HD Fe from_canonical(const uint32_t* w) {
    constexpr uint32_t C522[f29::NL] = {0x059bac10u, 0x0d1503a3u, 0x018016b8u, 0x10ab0ca8u, 0x02632639u, 0x02c0169fu, 0x169bfd53u, 0x11869d4cu, 0x002a11a6u};
    Fe c;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) c.v[i] = C522[i];
    return f29::mul<QM>(f29::from_words256(w), c);
}
F29_HD Fe fq_neg(const Fe& a) { return f29::tighten<QM>(f29::sub<4, QM>(f29::zero(), a)); }   // a < 2^255
// a / 2 for a normalised value: a + q where a is odd, then one shift through the limbs
F29_HD Fe fq_half(const Fe& a) {
    Fe qm;
    const uint32_t odd = 0u - (a.v[0] & 1u);
#pragma unroll
    for (int i = 0; i < f29::NL; i++) qm.v[i] = QM::p(i) & odd;
    const Fe s = f29::add(a, qm);
    Fe r;
#pragma unroll
    for (int i = 0; i < f29::NL - 1; i++) r.v[i] = (s.v[i] >> 1) | ((s.v[i + 1] & 1u) << (f29::LB - 1));
    r.v[f29::NL - 1] = s.v[f29::NL - 1] >> 1;
    return r;
}
F29_HD bool fq_eq(const Fe& a, const Fe& b) { return f29::is_zero_mod<QM>(f29::sub<4, QM>(a, b)); }   // b < 2^255

// a^((q - 3) / 4): bit b of the exponent is bit b + 2 of q - 3, and q ends in ...47, so q - 3 is q's words but for the lowest,
// without a borrow.  q has 254 bits: the exponent 252.  a < 2^257.5; the result is tight
BNP_FN Fe fq_pow_q34(const Fe& a) {
    Fe r = f29::one<QM>();
    for (int bit = 253; bit >= 2; bit--) {
        r = f29::mul<QM>(r, r);
        const uint32_t word = QP::mod(bit >> 5) - ((bit >> 5) == 0 ? 3u : 0u);
        if ((word >> (bit & 31)) & 1) r = f29::mul<QM>(r, a);
    }
    return r;
}
// a square root of a (tight) in Fq; false: there is none, and y is then a root of -a
BNP_FN bool fq_sqrt(const Fe& a, Fe& y) {
    y = f29::mul<QM>(fq_pow_q34(a), a);
    return fq_eq(f29::mul<QM>(y, y), a);
}
// a square root of a (components tight) in Fq2; false: there is none
BNP_FN bool f2_sqrt(const Fe2& a, Fe2& y) {
    const Fe n = f29::add(f29::mul<QM>(a.c0, a.c0), f29::mul<QM>(a.c1, a.c1));   // the norm, < 2^256
    const Fe s = f29::mul<QM>(fq_pow_q34(n), n);                                  // its root, if it has one
    const Fe tp = fq_half(f29::tighten<QM>(f29::add(a.c0, s))), tm = fq_half(f29::tighten<QM>(f29::sub<4, QM>(a.c0, s)));
    const bool use_tm = f29::is_zero_mod<QM>(tp);
    Fe t;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) t.v[i] = use_tm ? tm.v[i] : tp.v[i];
    const Fe w = fq_pow_q34(t), c = f29::tighten<QM>(f29::mul<QM>(w, t));
    const bool real = fq_eq(f29::mul<QM>(c, c), t);                               // c^2 = t; otherwise c^2 = -t
    const Fe o = fq_half(f29::tighten<QM>(f29::mul<QM>(a.c1, w)));                // a1 w / 2 = +- a1 / (2 c)
    const Fe on = fq_neg(o);
#pragma unroll
    for (int i = 0; i < f29::NL; i++) {
        y.c0.v[i] = real ? c.v[i] : on.v[i];
        y.c1.v[i] = real ? o.v[i] : c.v[i];
    }
    return pairing::f2_eq(F2::sqr(y), a);
}
F29_HD Fe2 f2_neg_tight(const Fe2& a) { return Fe2{fq_neg(a.c0), fq_neg(a.c1)}; }
// rule 5 over Fq2: decided on A1, on A0 when A1 is zero
BNP_FN bool f2_largest(const Fe2& y) {
    uint32_t w0[8], w1[8];
    f29::to_canonical256<QM>(y.c0, w0);
    f29::to_canonical256<QM>(y.c1, w1);
    return limbs_zero(w1) ? limbs_largest(w0) : limbs_largest(w1);
}
F29_HD Fe fq_three() { return f29::add(f29::one<QM>(), f29::add(f29::one<QM>(), f29::one<QM>())); }

// ---- decode: m = the point's bytes as native 32-bit words of memory (8 per coordinate); out: the words, all zero for the point
// at infinity and for every bad point.  The order of the checks is rule 6 of the model ----
// rules 1 and 2 on the first coordinate's limbs (flag bits still in place) and the OR of every other limb of the point
F29_HD bool head_status(uint32_t top_limb, uint32_t rest_or, bool raw, uint32_t& st) {
    const uint32_t flag = top_limb >> 30;
    if (flag == 1) {
        st = ((top_limb & 0x3fffffffu) | rest_or) ? ST_BAD_INFINITY : ST_OK;
        return true;
    }
    if (raw ? flag != 0 : flag == 0) {
        st = ST_BAD_FLAG;
        return true;
    }
    return false;
}
BNP_FN uint32_t g1_decode(const uint32_t* m /* 8, raw: 16 */, bool raw, uint64_t* out /* 8 */) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    uint32_t x[8], y[8];
    be_to_limbs(m, x);
    if (raw) be_to_limbs(m + 8, y);
    else for (int i = 0; i < 8; i++) y[i] = 0;
    uint32_t rest = 0, st;
    for (int i = 0; i < 7; i++) rest |= x[i];
    for (int i = 0; i < 8; i++) rest |= y[i];
    if (head_status(x[7], rest, raw, st)) return st;
    const bool flag_largest = (x[7] >> 30) == 3;
    x[7] &= 0x3fffffffu;
    if (!limbs_below_q(x) || (raw && !limbs_below_q(y))) return ST_RANGE;
    const Fe xf = from_canonical(x);
    const Fe rhs = f29::tighten<QM>(f29::add(f29::mul<QM>(f29::mul<QM>(xf, xf), xf), fq_three()));
    Fe yf;
    if (raw) {
        yf = from_canonical(y);
        if (!fq_eq(f29::mul<QM>(yf, yf), rhs)) return ST_OFF_CURVE;
    } else {
        if (!fq_sqrt(rhs, yf)) return ST_OFF_CURVE;
        uint32_t yc[8];
        f29::to_canonical256<QM>(yf, yc);
        if (limbs_largest(yc) != flag_largest) yf = fq_neg(yf);
    }
    pairing::fq_store(xf, true, out);
    pairing::fq_store(yf, true, out + 4);
    return ST_OK;
}
// m: X.A1 X.A0 (Y.A1 Y.A0); out: X.A0 X.A1 Y.A0 Y.A1
BNP_FN uint32_t g2_decode(const uint32_t* m /* 16, raw: 32 */, bool raw, bool subgroup, uint64_t* out /* 16 */) {
    for (int i = 0; i < 16; i++) out[i] = 0;
    uint32_t x1[8], x0[8], y1[8], y0[8];
    be_to_limbs(m, x1);
    be_to_limbs(m + 8, x0);
    if (raw) {
        be_to_limbs(m + 16, y1);
        be_to_limbs(m + 24, y0);
    } else {
        for (int i = 0; i < 8; i++) y1[i] = y0[i] = 0;
    }
    uint32_t rest = 0, st;
    for (int i = 0; i < 7; i++) rest |= x1[i];
    for (int i = 0; i < 8; i++) rest |= x0[i] | y1[i] | y0[i];
    if (head_status(x1[7], rest, raw, st)) return st;
    const bool flag_largest = (x1[7] >> 30) == 3;
    x1[7] &= 0x3fffffffu;
    if (!limbs_below_q(x1) || !limbs_below_q(x0) || (raw && (!limbs_below_q(y1) || !limbs_below_q(y0)))) return ST_RANGE;
    const Fe2 xf = F2::tighten(Fe2{from_canonical(x0), from_canonical(x1)});
    const Fe2 rhs = F2::add(pairing::f2_mul(pairing::f2_sqr(xf), xf), pairing::cst(pairing::BNP_TWIST_B));
    Fe2 yf;
    if (raw) {
        yf = F2::tighten(Fe2{from_canonical(y0), from_canonical(y1)});
        if (!pairing::f2_eq(pairing::f2_sqr(yf), rhs)) return ST_OFF_CURVE;
    } else {
        if (!f2_sqrt(rhs, yf)) return ST_OFF_CURVE;
        if (f2_largest(yf) != flag_largest) yf = f2_neg_tight(yf);
    }
    if (subgroup && !pairing::g2_in_subgroup(pairing::G2Point{xf, yf, false})) return ST_NOT_IN_SUBGROUP;
    pairing::fq_store(xf.c0, true, out);
    pairing::fq_store(xf.c1, true, out + 4);
    pairing::fq_store(yf.c0, true, out + 8);
    pairing::fq_store(yf.c1, true, out + 12);
    return ST_OK;
}

// ---- encode: the words -> bytes as native 32-bit words of memory.  The curve is not tested (gnark does not); a coordinate
// that is not below q is refused (ST_RANGE, zero bytes) ----
F29_HD void write_infinity(uint32_t* m, int n) {
    m[0] = 0x40u;   // the first byte in memory: both sides are little-endian machines
    for (int i = 1; i < n; i++) m[i] = 0;
}
BNP_FN uint32_t g1_encode(const uint64_t* w /* 8 */, bool raw, uint32_t* m /* 8, raw: 16 */) {
    const int n = raw ? 16 : 8;
    if (!pairing::coords_below_q(w, 2)) {
        for (int i = 0; i < n; i++) m[i] = 0;
        return ST_RANGE;
    }
    if (pairing::words_zero(w, 8)) {
        write_infinity(m, n);
        return ST_OK;
    }
    const pairing::G1Point p = pairing::g1_load(w);
    uint32_t x[8], y[8];
    f29::to_canonical256<QM>(p.x, x);
    f29::to_canonical256<QM>(p.y, y);
    if (!raw) x[7] |= limbs_largest(y) ? 0xC0000000u : 0x80000000u;
    limbs_to_be(x, m);
    if (raw) limbs_to_be(y, m + 8);
    return ST_OK;
}
BNP_FN uint32_t g2_encode(const uint64_t* w /* 16 */, bool raw, uint32_t* m /* 16, raw: 32 */) {
    const int n = raw ? 32 : 16;
    if (!pairing::coords_below_q(w, 4)) {
        for (int i = 0; i < n; i++) m[i] = 0;
        return ST_RANGE;
    }
    if (pairing::words_zero(w, 16)) {
        write_infinity(m, n);
        return ST_OK;
    }
    const pairing::G2Point p = pairing::g2_load(w);
    uint32_t x0[8], x1[8], y0[8], y1[8];
    f29::to_canonical256<QM>(p.x.c0, x0);
    f29::to_canonical256<QM>(p.x.c1, x1);
    f29::to_canonical256<QM>(p.y.c0, y0);
    f29::to_canonical256<QM>(p.y.c1, y1);
    if (!raw) x1[7] |= (limbs_zero(y1) ? limbs_largest(y0) : limbs_largest(y1)) ? 0xC0000000u : 0x80000000u;
    limbs_to_be(x1, m);
    limbs_to_be(x0, m + 8);
    if (raw) {
        limbs_to_be(y1, m + 16);
        limbs_to_be(y0, m + 24);
    }
    return ST_OK;
}

}  // namespace codec
}  // namespace nlx
