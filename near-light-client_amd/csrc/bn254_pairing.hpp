// The optimal ate pairing on BN254: the tower Fq2 - Fq6 - Fq12 over f29::F2 (bn254_f29.hpp), the Miller loop, the final
// exponentiation and the G2 subgroup test - host and device source.  Builds with
// plain g++ (tests/native/bn254_pairing_check.cpp) and is compared there with the big-integer model tools/bn254_pairing_model.py,
// which shares no formula with it.
//
//   Fq6  = Fq2[v] / (v^3 - xi), xi = 9 + u          Fe6 {b0, b1, b2}
//   Fq12 = Fq6[w] / (w^2 - v)                        Fe12 {c0, c1}; c_c.b_b is the Fq2 coefficient of w^(2 b + c) - gnark-crypto's
//                                                    E12, and the order of the twelve Fq elements in memory
//   twist  y^2 = x^3 + b', b' = 3 / xi (D type): (x', y') -> (x' w^2, y' w^3) lands on y^2 = x^3 + 3 over Fq12
//
// Every Fq2 value is tightened (f29::F2: both components below 1.1 q), so no bound is tracked through the formulas.  Nothing
// here branches on or indexes by a value that came from the caller: the loops run over the bits of the compile-time constants
// 6 x + 2, x, q - 2 and r - 1, and a point at infinity is carried through as whatever its zero coordinates give and replaced by 1
// at the end.
//
// The big functions are not inlined on the device: a lane's Fq12 values are 108 registers each, and one Fq12 product inlined is
// 54 base-field products of ~250 instructions.  As calls, the code is a few dozen kilobytes and the values between calls rest
// in scratch (profiles/bn254_pairing_resource_usage.txt).
#pragma once
#include <cstdint>
#include "bn254_f29.hpp"
#if defined(__HIPCC__)
#define BNP_FN static __host__ __device__ __noinline__
#else
#define BNP_FN static inline
#endif

namespace nlx {
namespace pairing {

using f29::Fe;
using f29::Fe2;
typedef f29::F2 F2;
typedef f29::QMod QM;

#include "bn254_pairing_consts.inc"

F29_HD Fe2 cst(int k) {
    constexpr uint32_t T[BNP_N_CONSTS][2][f29::NL] = {BNP_CONST_TABLE};
    Fe2 r;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) {
        r.c0.v[i] = T[k][0][i];
        r.c1.v[i] = T[k][1][i];
    }
    return r;
}

constexpr uint64_t BN_X = 4965661367192848881ull;          // the curve's parameter x
constexpr uint64_t ATE_LOOP_LOW = 0x9d797039be763ba8ull;   // 6 x + 2 = 2^64 + this (65 bits); checked below
static_assert(6 * (unsigned __int128)BN_X + 2 == (((unsigned __int128)1 << 64) | ATE_LOOP_LOW), "6 x + 2");

struct Fe6 {
    Fe2 b0, b1, b2;
};
struct Fe12 {
    Fe6 c0, c1;
};
struct G1Point {   // affine over Fq; inf: the point at infinity (both words strings zero)
    Fe x, y;
    bool inf;
};
struct G2Point {   // affine over Fq2 on the twist
    Fe2 x, y;
    bool inf;
};

// ---- Fq2 beyond f29::F2 ----
F29_HD Fe2 f2_neg(const Fe2& a) { return F2::sub<4>(F2::zero(), a); }
F29_HD Fe2 f2_conj(const Fe2& a) { return Fe2{a.c0, F2::tt(f29::sub<4, QM>(f29::zero(), a.c1))}; }
F29_HD Fe2 f2_mul_fq(const Fe2& a, const Fe& s) { return Fe2{F2::tt(f29::mul<QM>(a.c0, s)), F2::tt(f29::mul<QM>(a.c1, s))}; }
F29_HD Fe2 f2_mul_xi(const Fe2& a) {   // (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u
    const Fe2 t = F2::add(F2::dbl(F2::dbl(F2::dbl(a))), a);
    return Fe2{F2::tt(f29::sub<4, QM>(t.c0, a.c1)), F2::tt(f29::add(t.c1, a.c0))};
}
F29_HD Fe2 f2_triple(const Fe2& a) { return F2::add(F2::dbl(a), a); }
F29_HD bool f2_eq(const Fe2& a, const Fe2& b) { return F2::is_zero_mod(F2::sub<4>(a, b)); }
// a^(q - 2) over the bits of the constant q - 2 (Fermat): the one base-field inversion of a check
BNP_FN Fe fq_inv(const Fe& a) {
    Fe r = f29::one<QM>();
    for (int bit = 253; bit >= 0; bit--) {
        r = f29::mul<QM>(r, r);
        // q - 2 as eight 32-bit words: q's own but for the lowest (q ends in ...47)
        const uint32_t word = bnf::QP::mod(bit >> 5) - ((bit >> 5) == 0 ? 2u : 0u);
        if ((word >> (bit & 31)) & 1) r = f29::mul<QM>(r, a);
    }
    return f29::tighten<QM>(r);
}
BNP_FN Fe2 f2_inv(const Fe2& a) {   // conj(a) / (a0^2 + a1^2)
    const Fe d = fq_inv(f29::add(f29::mul<QM>(a.c0, a.c0), f29::mul<QM>(a.c1, a.c1)));
    return f2_conj(f2_mul_fq(a, d));
}
BNP_FN Fe2 f2_mul(const Fe2& a, const Fe2& b) { return F2::mul(a, b); }   // the out-of-line product the big functions call
BNP_FN Fe2 f2_sqr(const Fe2& a) { return F2::sqr(a); }

// ---- Fq6 ----
F29_HD Fe6 f6_zero() { return Fe6{F2::zero(), F2::zero(), F2::zero()}; }
F29_HD Fe6 f6_one() { return Fe6{F2::one(), F2::zero(), F2::zero()}; }
F29_HD Fe6 f6_add(const Fe6& a, const Fe6& b) { return Fe6{F2::add(a.b0, b.b0), F2::add(a.b1, b.b1), F2::add(a.b2, b.b2)}; }
F29_HD Fe6 f6_sub(const Fe6& a, const Fe6& b) { return Fe6{F2::sub<4>(a.b0, b.b0), F2::sub<4>(a.b1, b.b1), F2::sub<4>(a.b2, b.b2)}; }
F29_HD Fe6 f6_neg(const Fe6& a) { return Fe6{f2_neg(a.b0), f2_neg(a.b1), f2_neg(a.b2)}; }
F29_HD Fe6 f6_mul_v(const Fe6& a) { return Fe6{f2_mul_xi(a.b2), a.b0, a.b1}; }
// Karatsuba over Fq2: six products
BNP_FN Fe6 f6_mul(const Fe6& a, const Fe6& b) {
    const Fe2 t0 = f2_mul(a.b0, b.b0), t1 = f2_mul(a.b1, b.b1), t2 = f2_mul(a.b2, b.b2);
    Fe6 r;
    r.b0 = F2::add(f2_mul_xi(F2::sub<4>(F2::sub<4>(f2_mul(F2::add(a.b1, a.b2), F2::add(b.b1, b.b2)), t1), t2)), t0);
    r.b1 = F2::add(F2::sub<4>(F2::sub<4>(f2_mul(F2::add(a.b0, a.b1), F2::add(b.b0, b.b1)), t0), t1), f2_mul_xi(t2));
    r.b2 = F2::add(F2::sub<4>(F2::sub<4>(f2_mul(F2::add(a.b0, a.b2), F2::add(b.b0, b.b2)), t0), t2), t1);
    return r;
}
// a (c0 + c1 v): five products (the sparse half of a line)
BNP_FN Fe6 f6_mul_by_01(const Fe6& a, const Fe2& c0, const Fe2& c1) {
    const Fe2 t0 = f2_mul(a.b0, c0), t1 = f2_mul(a.b1, c1);
    Fe6 r;
    r.b0 = F2::add(f2_mul_xi(F2::sub<4>(f2_mul(F2::add(a.b1, a.b2), c1), t1)), t0);
    r.b1 = F2::sub<4>(F2::sub<4>(f2_mul(F2::add(a.b0, a.b1), F2::add(c0, c1)), t0), t1);
    r.b2 = F2::add(F2::sub<4>(f2_mul(F2::add(a.b0, a.b2), c0), t0), t1);
    return r;
}
BNP_FN Fe6 f6_mul_f2(const Fe6& a, const Fe2& c) { return Fe6{f2_mul(a.b0, c), f2_mul(a.b1, c), f2_mul(a.b2, c)}; }
// (A, B, C) / (a0 A + xi (a2 B + a1 C)), A = a0^2 - xi a1 a2, B = xi a2^2 - a0 a1, C = a1^2 - a0 a2
BNP_FN Fe6 f6_inv(const Fe6& a) {
    const Fe2 A = F2::sub<4>(f2_sqr(a.b0), f2_mul_xi(f2_mul(a.b1, a.b2)));
    const Fe2 B = F2::sub<4>(f2_mul_xi(f2_sqr(a.b2)), f2_mul(a.b0, a.b1));
    const Fe2 C = F2::sub<4>(f2_sqr(a.b1), f2_mul(a.b0, a.b2));
    const Fe2 F = F2::add(f2_mul(a.b0, A), f2_mul_xi(F2::add(f2_mul(a.b2, B), f2_mul(a.b1, C))));
    const Fe2 fi = f2_inv(F);
    return Fe6{f2_mul(A, fi), f2_mul(B, fi), f2_mul(C, fi)};
}

// ---- Fq12 ----
F29_HD Fe12 f12_one() { return Fe12{f6_one(), f6_zero()}; }
F29_HD Fe12 f12_conj(const Fe12& a) { return Fe12{a.c0, f6_neg(a.c1)}; }   // the q^6 power; the inverse on the cyclotomic subgroup
BNP_FN Fe12 f12_mul(const Fe12& a, const Fe12& b) {   // Karatsuba over Fq6: three products
    const Fe6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    Fe12 r;
    r.c1 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1);
    r.c0 = f6_add(t0, f6_mul_v(t1));
    return r;
}
BNP_FN Fe12 f12_sqr(const Fe12& a) {   // (a0 + a1)(a0 + v a1) - t - v t + 2 t w, t = a0 a1: two products
    const Fe6 t = f6_mul(a.c0, a.c1);
    Fe12 r;
    r.c0 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1))), t), f6_mul_v(t));
    r.c1 = f6_add(t, t);
    return r;
}
// a times the line l0 + l1 w + l2 w^3 (coefficients at c0.b0, c1.b0, c1.b1): thirteen Fq2 products
BNP_FN Fe12 f12_mul_by_line(const Fe12& a, const Fe2& l0, const Fe2& l1, const Fe2& l2) {
    const Fe6 t0 = f6_mul_f2(a.c0, l0), t1 = f6_mul_by_01(a.c1, l1, l2);
    Fe12 r;
    r.c1 = f6_sub(f6_sub(f6_mul_by_01(f6_add(a.c0, a.c1), F2::add(l0, l1), l2), t0), t1);
    r.c0 = f6_add(t0, f6_mul_v(t1));
    return r;
}
BNP_FN Fe12 f12_inv(const Fe12& a) {   // (a0 - a1 w) / (a0^2 - v a1^2)
    const Fe6 t = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return Fe12{f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t))};
}
// the q^k power, k = 1, 2, 3: coefficient i of w^i is conjugated (odd k) and multiplied by xi^(i (q^k - 1) / 6)
template <int K>
BNP_FN Fe12 f12_frobenius(const Fe12& a) {
    static_assert(K >= 1 && K <= 3, "q, q^2, q^3");
    constexpr int base = BNP_FROB + 5 * (K - 1);
    constexpr bool cj = (K & 1) != 0;
    Fe12 r;
    r.c0.b0 = cj ? f2_conj(a.c0.b0) : a.c0.b0;                                         // w^0
    r.c1.b0 = f2_mul(cj ? f2_conj(a.c1.b0) : a.c1.b0, cst(base + 0));                  // w^1
    r.c0.b1 = f2_mul(cj ? f2_conj(a.c0.b1) : a.c0.b1, cst(base + 1));                  // w^2
    r.c1.b1 = f2_mul(cj ? f2_conj(a.c1.b1) : a.c1.b1, cst(base + 2));                  // w^3
    r.c0.b2 = f2_mul(cj ? f2_conj(a.c0.b2) : a.c0.b2, cst(base + 3));                  // w^4
    r.c1.b2 = f2_mul(cj ? f2_conj(a.c1.b2) : a.c1.b2, cst(base + 4));                  // w^5
    return r;
}
// Granger and Scott's square for an element of the cyclotomic subgroup (a^(q^4 - q^2 + 1) = 1), through its three Fq4 pairs
// (c0.b0, c1.b1), (c1.b0, c0.b2), (c0.b1, c1.b2): nine Fq2 squares
BNP_FN Fe12 f12_cyclotomic_sqr(const Fe12& a) {
    Fe2 t0 = f2_sqr(a.c1.b1), t1 = f2_sqr(a.c0.b0);
    const Fe2 t6 = F2::sub<4>(F2::sub<4>(f2_sqr(F2::add(a.c1.b1, a.c0.b0)), t0), t1);   // 2 c1.b1 c0.b0
    Fe2 t2 = f2_sqr(a.c0.b2), t3 = f2_sqr(a.c1.b0);
    const Fe2 t7 = F2::sub<4>(F2::sub<4>(f2_sqr(F2::add(a.c0.b2, a.c1.b0)), t2), t3);   // 2 c0.b2 c1.b0
    Fe2 t4 = f2_sqr(a.c1.b2), t5 = f2_sqr(a.c0.b1);
    const Fe2 t8 = f2_mul_xi(F2::sub<4>(F2::sub<4>(f2_sqr(F2::add(a.c1.b2, a.c0.b1)), t4), t5));   // 2 c1.b2 c0.b1 xi
    t0 = F2::add(f2_mul_xi(t0), t1);
    t2 = F2::add(f2_mul_xi(t2), t3);
    t4 = F2::add(f2_mul_xi(t4), t5);
    Fe12 r;
    r.c0.b0 = F2::add(F2::dbl(F2::sub<4>(t0, a.c0.b0)), t0);
    r.c0.b1 = F2::add(F2::dbl(F2::sub<4>(t2, a.c0.b1)), t2);
    r.c0.b2 = F2::add(F2::dbl(F2::sub<4>(t4, a.c0.b2)), t4);
    r.c1.b0 = F2::add(F2::dbl(F2::add(t8, a.c1.b0)), t8);
    r.c1.b1 = F2::add(F2::dbl(F2::add(t6, a.c1.b1)), t6);
    r.c1.b2 = F2::add(F2::dbl(F2::add(t7, a.c1.b2)), t7);
    return r;
}
F29_HD bool f6_eq(const Fe6& a, const Fe6& b) { return f2_eq(a.b0, b.b0) && f2_eq(a.b1, b.b1) && f2_eq(a.b2, b.b2); }
BNP_FN bool f12_eq(const Fe12& a, const Fe12& b) { return f6_eq(a.c0, b.c0) && f6_eq(a.c1, b.c1); }   // equality mod q
// branch-free choice (a point at infinity's Miller value is replaced by 1)
F29_HD Fe12 f12_select(bool take_b, const Fe12& a, const Fe12& b) {
    Fe12 r;
    const uint32_t m = take_b ? 0xffffffffu : 0u;
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(&a);
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(&b);
    uint32_t* pr = reinterpret_cast<uint32_t*>(&r);
    for (unsigned i = 0; i < sizeof(Fe12) / 4; i++) pr[i] = (pa[i] & ~m) | (pb[i] & m);
    return r;
}

// ---- Miller loop: T in homogeneous coordinates (X : Y : Z) on the twist, the lines scaled by a factor in Fq2 (the final
// exponentiation kills it).  A line at P = (xP, yP) is l0 + l1 w + l2 w^3. ----
struct G2Proj {
    Fe2 x, y, z;
};
struct Line {
    Fe2 l0, l1, l2;
};
// T <- 2 T; the tangent at T: 2 Y Z yP - 3 X^2 xP w + (Y^2 - 3 b' Z^2) w^3
BNP_FN Line double_step(G2Proj& t, const Fe& xp, const Fe& yp) {
    const Fe2 a = f2_mul(t.x, t.y), b = f2_sqr(t.y), c = f2_sqr(t.z);
    const Fe2 e = f2_mul(c, cst(BNP_TWIST_3B)), f = f2_triple(e);
    const Fe2 h = F2::dbl(f2_mul(t.y, t.z)), xx = f2_sqr(t.x);
    Line l;
    l.l0 = f2_mul_fq(h, yp);
    l.l1 = f2_neg(f2_mul_fq(f2_triple(xx), xp));
    l.l2 = F2::sub<4>(b, e);
    const Fe2 e2 = f2_sqr(e);
    t.x = f2_mul(F2::dbl(a), F2::sub<4>(b, f));
    t.y = F2::sub<4>(f2_sqr(F2::add(b, f)), F2::dbl(F2::dbl(f2_triple(e2))));
    t.z = F2::dbl(F2::dbl(f2_mul(b, h)));
    return l;
}
// T <- T + Q; the chord: mu yP - theta xP w + (theta x2 - mu y2) w^3, theta = Y - y2 Z, mu = X - x2 Z
BNP_FN Line add_step(G2Proj& t, const Fe2& x2, const Fe2& y2, const Fe& xp, const Fe& yp) {
    const Fe2 theta = F2::sub<4>(t.y, f2_mul(y2, t.z)), mu = F2::sub<4>(t.x, f2_mul(x2, t.z));
    Line l;
    l.l0 = f2_mul_fq(mu, yp);
    l.l1 = f2_neg(f2_mul_fq(theta, xp));
    l.l2 = F2::sub<4>(f2_mul(theta, x2), f2_mul(mu, y2));
    const Fe2 c = f2_sqr(theta), d = f2_sqr(mu), e = f2_mul(mu, d), f = f2_mul(t.z, c), g = f2_mul(t.x, d);
    const Fe2 h = F2::sub<4>(F2::add(e, f), F2::dbl(g));
    const Fe2 y3 = F2::sub<4>(f2_mul(theta, F2::sub<4>(g, h)), f2_mul(e, t.y));
    t.x = f2_mul(mu, h);
    t.y = y3;
    t.z = f2_mul(t.z, e);
    return l;
}
// f_(6x+2, Q)(P) l_(T, pi Q)(P) l_(T + pi Q, -pi^2 Q)(P); 1 if either point is the point at infinity
BNP_FN Fe12 miller_loop(const G1Point& p, const G2Point& q) {
    G2Proj t{q.x, q.y, F2::one()};
    Fe12 f = f12_one();
    for (int bit = 63; bit >= 0; bit--) {
        Line l = double_step(t, p.x, p.y);
        f = f12_mul_by_line(f12_sqr(f), l.l0, l.l1, l.l2);
        if ((ATE_LOOP_LOW >> bit) & 1) {
            l = add_step(t, q.x, q.y, p.x, p.y);
            f = f12_mul_by_line(f, l.l0, l.l1, l.l2);
        }
    }
    // pi(x', y') = (conj(x') xi^((q-1)/3), conj(y') xi^((q-1)/2)); pi^2(x', y') = (x' xi^((q^2-1)/3), y' xi^((q^2-1)/2))
    const Fe2 x1 = f2_mul(f2_conj(q.x), cst(BNP_FROB + 1)), y1 = f2_mul(f2_conj(q.y), cst(BNP_FROB + 2));
    const Fe2 x2 = f2_mul(q.x, cst(BNP_FROB + 5 + 1)), y2 = f2_neg(f2_mul(q.y, cst(BNP_FROB + 5 + 2)));
    Line l = add_step(t, x1, y1, p.x, p.y);
    f = f12_mul_by_line(f, l.l0, l.l1, l.l2);
    l = add_step(t, x2, y2, p.x, p.y);
    f = f12_mul_by_line(f, l.l0, l.l1, l.l2);
    return f12_select(p.inf | q.inf, f, f12_one());
}

// ---- final exponentiation ----
BNP_FN Fe12 f12_exp_by_x(const Fe12& a) {   // a^x for a in the cyclotomic subgroup: x has 63 bits
    Fe12 r = a;
    for (int bit = 61; bit >= 0; bit--) {
        r = f12_cyclotomic_sqr(r);
        if ((BN_X >> bit) & 1) r = f12_mul(r, a);
    }
    return r;
}
// f^((q^12 - 1) / r) exactly: the easy part (q^6 - 1)(q^2 + 1), then (q^4 - q^2 + 1) / r by the chain of Scott, Benger,
// Charlemagne, Dominguez Perez and Kachisa (y0 .. y6; tools/bn254_pairing_model.py recomputes the exponent from the chain)
BNP_FN Fe12 final_exponentiation(const Fe12& in) {
    Fe12 f = f12_mul(f12_conj(in), f12_inv(in));
    f = f12_mul(f12_frobenius<2>(f), f);
    const Fe12 fp = f12_frobenius<1>(f), fp2 = f12_frobenius<2>(f), fp3 = f12_frobenius<3>(f);
    const Fe12 fu = f12_exp_by_x(f), fu2 = f12_exp_by_x(fu), fu3 = f12_exp_by_x(fu2);
    const Fe12 y0 = f12_mul(f12_mul(fp, fp2), fp3);
    const Fe12 y1 = f12_conj(f);
    const Fe12 y2 = f12_frobenius<2>(fu2);
    const Fe12 y3 = f12_conj(f12_frobenius<1>(fu));
    const Fe12 y4 = f12_conj(f12_mul(fu, f12_frobenius<1>(fu2)));
    const Fe12 y5 = f12_conj(fu2);
    const Fe12 y6 = f12_conj(f12_mul(fu3, f12_frobenius<1>(fu3)));
    Fe12 t0 = f12_mul(f12_mul(f12_cyclotomic_sqr(y6), y4), y5);
    Fe12 t1 = f12_mul(f12_mul(y3, y5), t0);
    t0 = f12_mul(t0, y2);
    t1 = f12_cyclotomic_sqr(f12_mul(f12_cyclotomic_sqr(t1), t0));
    t0 = f12_mul(t1, y1);
    t1 = f12_mul(t1, y0);
    return f12_mul(f12_cyclotomic_sqr(t0), t1);
}

// ---- points from gnark-crypto's words (Montgomery, R = 2^256; all zero = the point at infinity), and their checks ----
F29_HD bool words_zero(const uint64_t* w, int n) {
    uint64_t o = 0;
    for (int i = 0; i < n; i++) o |= w[i];
    return o == 0;
}
BNP_FN G1Point g1_load(const uint64_t* w /* 8 */) {
    uint32_t v[16];
    for (int i = 0; i < 8; i++) {
        v[2 * i] = (uint32_t)w[i];
        v[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return G1Point{f29::tighten<QM>(f29::from_mont256<QM>(v)), f29::tighten<QM>(f29::from_mont256<QM>(v + 8)), words_zero(w, 8)};
}
BNP_FN G2Point g2_load(const uint64_t* w /* 16: X.A0 X.A1 Y.A0 Y.A1 */) {
    uint32_t v[32];
    for (int i = 0; i < 16; i++) {
        v[2 * i] = (uint32_t)w[i];
        v[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return G2Point{F2::from_mont256(v), F2::from_mont256(v + 16), words_zero(w, 16)};
}
enum PointStatus : uint32_t {   // what the entry checks answer, in the order they are made
    POINT_OK = 0, G1_RANGE = 1, G1_OFF_CURVE = 2, G2_RANGE = 3, G2_OFF_CURVE = 4, G2_NOT_IN_SUBGROUP = 5
};
F29_HD bool coords_below_q(const uint64_t* w, int n_coords) {
    bool ok = true;
    for (int i = 0; i < n_coords; i++) ok &= bnf::below_mod<bnf::QP>(w + 4 * i);
    return ok;
}
BNP_FN bool g1_on_curve(const G1Point& p) {   // y^2 = x^3 + 3, or the point at infinity
    Fe three = f29::add(f29::one<QM>(), f29::add(f29::one<QM>(), f29::one<QM>()));
    const Fe rhs = f29::tighten<QM>(f29::add(f29::mul<QM>(f29::mul<QM>(p.x, p.x), p.x), three));   // < 2^255 + 3 q, then < 1.1 q
    return p.inf | f29::is_zero_mod<QM>(f29::sub<4, QM>(f29::mul<QM>(p.y, p.y), rhs));
}
BNP_FN bool g2_on_curve(const G2Point& q) {   // y^2 = x^3 + b'
    return q.inf | f2_eq(f2_sqr(q.y), F2::add(f2_mul(f2_sqr(q.x), q.x), cst(BNP_TWIST_B)));
}
// [r] Q = O the plain way: T = [r - 1] Q by double-and-add over the bits of the constant r - 1 with the Miller loop's own point
// steps (their lines dropped), then T = -Q.  A step that meets T = +-Q or the point at infinity on the way (only a point
// outside the subgroup can) leaves Z = 0, and Z = 0 stays: the answer is then "no", as it must be.
BNP_FN bool g2_in_subgroup(const G2Point& q) {
    G2Proj t{q.x, q.y, F2::one()};
    const Fe dummy = f29::zero();
    for (int bit = 252; bit >= 0; bit--) {   // r - 1 has 254 bits; the top one is T = Q
        (void)double_step(t, dummy, dummy);
        const uint32_t word = bnf::RP::mod(bit >> 5) - ((bit >> 5) == 0 ? 1u : 0u);   // r ends in ...1: no borrow
        if ((word >> (bit & 31)) & 1) (void)add_step(t, q.x, q.y, dummy, dummy);
    }
    const bool same_x = f2_eq(t.x, f2_mul(q.x, t.z)), opposite_y = F2::is_zero_mod(F2::add(t.y, f2_mul(q.y, t.z)));
    return q.inf | (same_x & opposite_y & !F2::is_zero_mod(t.z));
}
// every check of one pair on its words, first failure wins
BNP_FN uint32_t check_g1(const uint64_t* g1w) {
    if (!coords_below_q(g1w, 2)) return G1_RANGE;
    return g1_on_curve(g1_load(g1w)) ? POINT_OK : G1_OFF_CURVE;
}
BNP_FN uint32_t check_g2(const uint64_t* g2w) {
    if (!coords_below_q(g2w, 4)) return G2_RANGE;
    const G2Point q = g2_load(g2w);
    if (!g2_on_curve(q)) return G2_OFF_CURVE;
    return g2_in_subgroup(q) ? POINT_OK : G2_NOT_IN_SUBGROUP;
}
BNP_FN uint32_t check_pair(const uint64_t* g1w, const uint64_t* g2w) {
    const uint32_t st = check_g1(g1w);
    return st != POINT_OK ? st : check_g2(g2w);
}

// ---- a GT element in memory: twelve Fq elements in E12 order, four 64-bit words each; canonical integers, or Montgomery
// (x 2^256, gnark-crypto's fp.Element) ----
BNP_FN void fq_store(const Fe& a, bool montgomery, uint64_t* w) {
    uint32_t v[8];
    if (montgomery) {   // x 2^261 -> x 2^256: one product with the integer 2^256 (limb 8 holds bit 232 upward)
        Fe k = f29::zero();
        k.v[8] = 1u << 24;
        f29::to_words256(f29::canonical<QM>(f29::mul<QM>(a, k)), v);
    } else {
        f29::to_canonical256<QM>(a, v);
    }
    for (int i = 0; i < 4; i++) w[i] = (uint64_t)v[2 * i] | ((uint64_t)v[2 * i + 1] << 32);
}
BNP_FN void f12_store(const Fe12& a, bool montgomery, uint64_t* w /* 48 */) {
    const Fe2* c[6] = {&a.c0.b0, &a.c0.b1, &a.c0.b2, &a.c1.b0, &a.c1.b1, &a.c1.b2};
    for (int i = 0; i < 6; i++) {
        fq_store(c[i]->c0, montgomery, w + 8 * i);
        fq_store(c[i]->c1, montgomery, w + 8 * i + 4);
    }
}
BNP_FN Fe12 f12_load(const uint64_t* w /* 48, Montgomery */) {
    Fe12 a;
    Fe2* c[6] = {&a.c0.b0, &a.c0.b1, &a.c0.b2, &a.c1.b0, &a.c1.b1, &a.c1.b2};
    for (int i = 0; i < 6; i++) {
        uint32_t v[16];
        for (int k = 0; k < 8; k++) {
            v[2 * k] = (uint32_t)w[8 * i + k];
            v[2 * k + 1] = (uint32_t)(w[8 * i + k] >> 32);
        }
        *c[i] = F2::from_mont256(v);
    }
    return a;
}

}  // namespace pairing
}  // namespace nlx
