// The host half of the BN254 MSM (bn254_msm.hip) and the MSM's phases as calls of their own - what the Groth16 prover
// (bn254_groth16.hip) schedules: one digit decomposition and one set of sorted indices serve every query over the same
// scalars.  The group law is written over a field policy H (H1 = Fq, H2 = Fq2) on bn254_fp.hpp's 32-bit limbs.
#pragma once
#include <cstddef>
#include <cstdint>
#include "bn254_fp.hpp"
#include "ctx.hpp"

namespace nlx {
namespace msm {

using namespace bnf;
typedef Fp<QP> Fq;
typedef Fp<RP> Fr;

// ---- host side (the short tail of an MSM, nlx_bn254_g1_sum): eight 32-bit limbs, bn254_fp.hpp ----
struct H1 {   // Fq
    typedef Fq T;
    static constexpr int WORDS64 = 4;
    static T zero() { return bnf::zero<QP>(); }
    static T one() { return bnf::one<QP>(); }
    static bool is_zero(const T& a) { return bnf::is_zero(a); }
    static T add(const T& a, const T& b) { return bnf::add(a, b); }
    static T sub(const T& a, const T& b) { return bnf::sub(a, b); }
    static T mul(const T& a, const T& b) { return bnf::mul(a, b); }
    static T sqr(const T& a) { return bnf::mul(a, a); }
    static T neg(const T& a) { return bnf::neg(a); }
    static T inv(const T& a) { return bnf::inv_host(a); }
    static T load(const uint64_t* w) { return load_words<QP>(w); }
    static void store(const T& a, uint64_t* w) { store_words(a, w); }
    static T from_canonical(const uint32_t* w) {   // plain integer limbs -> Montgomery form
        Fq x;
        for (int l = 0; l < 8; l++) x.v[l] = w[l];
        return to_mont(x);
    }
};
struct H2 {   // Fq2 = Fq[u] / (u^2 + 1); gnark-crypto's E2{A0, A1}
    struct T { Fq c0, c1; };
    static constexpr int WORDS64 = 8;
    static T zero() { return T{bnf::zero<QP>(), bnf::zero<QP>()}; }
    static T one() { return T{bnf::one<QP>(), bnf::zero<QP>()}; }
    static bool is_zero(const T& a) { return bnf::is_zero(a.c0) && bnf::is_zero(a.c1); }
    static T add(const T& a, const T& b) { return T{bnf::add(a.c0, b.c0), bnf::add(a.c1, b.c1)}; }
    static T sub(const T& a, const T& b) { return T{bnf::sub(a.c0, b.c0), bnf::sub(a.c1, b.c1)}; }
    static T mul(const T& a, const T& b) {
        const Fq t0 = bnf::mul(a.c0, b.c0), t1 = bnf::mul(a.c1, b.c1);
        const Fq s = bnf::mul(bnf::add(a.c0, a.c1), bnf::add(b.c0, b.c1));
        return T{bnf::sub(t0, t1), bnf::sub(bnf::sub(s, t0), t1)};
    }
    static T sqr(const T& a) { return mul(a, a); }
    static T neg(const T& a) { return T{bnf::neg(a.c0), bnf::neg(a.c1)}; }
    static T inv(const T& a) {   // conj(a) / (a0^2 + a1^2)
        const Fq d = bnf::inv_host(bnf::add(bnf::mul(a.c0, a.c0), bnf::mul(a.c1, a.c1)));
        return T{bnf::mul(a.c0, d), bnf::neg(bnf::mul(a.c1, d))};
    }
    static T load(const uint64_t* w) { return T{load_words<QP>(w), load_words<QP>(w + 4)}; }
    static void store(const T& a, uint64_t* w) { store_words(a.c0, w); store_words(a.c1, w + 4); }
    static T from_canonical(const uint32_t* w) { return T{H1::from_canonical(w), H1::from_canonical(w + 8)}; }
};
template <class H> struct AffineH { typename H::T x, y; };   // (0, 0) = the point at infinity (gnark-crypto's convention)
template <class H> struct JacH { typename H::T x, y, z; };   // z = 0: the point at infinity
template <class H> inline typename H::T hdbl(const typename H::T& a) { return H::add(a, a); }
template <class H> inline JacH<H> hinf() { return JacH<H>{H::one(), H::one(), H::zero()}; }
// dbl-2009-l (a = 0): 2M + 5S
template <class H> inline JacH<H> hjdbl(const JacH<H>& p) {
    typedef typename H::T T;
    if (H::is_zero(p.z)) return p;
    const T a = H::sqr(p.x), b = H::sqr(p.y), c = H::sqr(b);
    const T d = hdbl<H>(H::sub(H::sub(H::sqr(H::add(p.x, b)), a), c));
    const T e = H::add(hdbl<H>(a), a), f = H::sqr(e);
    JacH<H> r;
    r.x = H::sub(f, hdbl<H>(d));
    r.y = H::sub(H::mul(e, H::sub(d, r.x)), hdbl<H>(hdbl<H>(hdbl<H>(c))));
    r.z = hdbl<H>(H::mul(p.y, p.z));
    return r;
}
// add-2007-bl: 11M + 5S; equal and opposite points are real cases
template <class H> inline JacH<H> hjadd(const JacH<H>& p, const JacH<H>& q) {
    typedef typename H::T T;
    if (H::is_zero(p.z)) return q;
    if (H::is_zero(q.z)) return p;
    const T z1z1 = H::sqr(p.z), z2z2 = H::sqr(q.z);
    const T u1 = H::mul(p.x, z2z2), u2 = H::mul(q.x, z1z1);
    const T s1 = H::mul(H::mul(p.y, q.z), z2z2), s2 = H::mul(H::mul(q.y, p.z), z1z1);
    const T h = H::sub(u2, u1);
    T r = H::sub(s2, s1);
    if (H::is_zero(h)) return H::is_zero(r) ? hjdbl<H>(p) : hinf<H>();
    r = hdbl<H>(r);
    const T i = H::sqr(hdbl<H>(h)), j = H::mul(h, i), v = H::mul(u1, i);
    JacH<H> o;
    o.x = H::sub(H::sub(H::sqr(r), j), hdbl<H>(v));
    o.y = H::sub(H::mul(r, H::sub(v, o.x)), hdbl<H>(H::mul(s1, j)));
    o.z = H::mul(H::sub(H::sub(H::sqr(H::add(p.z, q.z)), z1z1), z2z2), h);
    return o;
}
template <class H> inline JacH<H> hfrom_affine(const AffineH<H>& p) {
    return (H::is_zero(p.x) && H::is_zero(p.y)) ? hinf<H>() : JacH<H>{p.x, p.y, H::one()};
}
// Jacobian -> affine words (all zero for the point at infinity)
template <class H> inline void hstore_affine(const JacH<H>& p, uint64_t* out) {
    for (int i = 0; i < 2 * H::WORDS64; i++) out[i] = 0;
    if (H::is_zero(p.z)) return;
    const typename H::T zi = H::inv(p.z), zi2 = H::sqr(zi);
    H::store(H::mul(p.x, zi2), out);
    H::store(H::mul(p.y, H::mul(zi2, zi)), out + H::WORDS64);
}

// k p by double-and-add; k: the canonical integer (eight 32-bit limbs, below r)
template <class H> inline JacH<H> hjmul(const JacH<H>& p, const Fr& k) {
    JacH<H> acc = hinf<H>();
    for (int bit = 255; bit >= 0; bit--) {
        acc = hjdbl<H>(acc);
        if ((k.v[bit >> 5] >> (bit & 31)) & 1) acc = hjadd<H>(acc, p);
    }
    return acc;
}
template <class H> inline JacH<H> hjneg(const JacH<H>& p) { return JacH<H>{p.x, H::neg(p.y), p.z}; }
template <class H> inline JacH<H> hload_affine(const uint64_t* w) {
    return hfrom_affine<H>(AffineH<H>{H::load(w), H::load(w + H::WORDS64)});
}

// ---- the phases of one MSM (bn254_msm.hip).  g2 = 0: G1 (64-byte converted points), 1: G2 (128 bytes). ----
// phase 1: the scalars' sixteen digits, every window's (digit, index) pairs sorted by digit, every bucket's range
struct SortedDigits {
    size_t n = 0;
    uint32_t* sorted = nullptr;   // [window][n] point indices
    uint32_t* lo = nullptr;       // [window][65536] | hi: [window][65536]
    uint32_t* hi = nullptr;
    void* tmp[4] = {nullptr, nullptr, nullptr, nullptr};   // the sort's temporaries (released with the rest)
};
int32_t sort_digits(nlx_ctx* ctx, const uint64_t* d_scalars, size_t n, int montgomery, SortedDigits* out);   // enqueues; n >= 1
void release_digits(nlx_ctx* ctx, SortedDigits* s);   // after the stream has been synchronised
// gnark-crypto affine words -> the kernels' form (enqueues).  index (may be NULL): out[i] = points[index[i]], the point at
// infinity where index[i] = 0xFFFFFFFF - a query filtered of its points at infinity, expanded to the wires' index space
size_t converted_point_bytes(int g2);
void convert_points(nlx_ctx* ctx, const uint64_t* d_points, const uint32_t* d_index, size_t n, int g2, void* d_out);
// phases 2 and 3: bucket sums through the sorted indices, then the windows' partial sums (enqueues)
size_t bucket_bytes(int g2);
size_t window_sum_bytes(int g2);
void bucket_reduce(nlx_ctx* ctx, const SortedDigits& s, const void* d_converted, int g2, void* d_buckets, void* d_window_sums);
// phase 4, host: the fetched partial sums -> sum_w 2^(16 w) W_w
JacH<H1> window_tail_g1(const void* window_sums);
JacH<H2> window_tail_g2(const void* window_sums);

}  // namespace msm
}  // namespace nlx
