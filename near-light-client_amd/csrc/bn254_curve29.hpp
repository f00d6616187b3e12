// The BN254 group law on the device's field representation (bn254_f29.hpp), written once over a field policy F: what the MSM's
// kernels (bn254_msm.hip) and the Groth16 verifier's public sum (bn254_pairing.hip) add points with.  F1 = Fq: loose values; the
// bound of every intermediate is noted where it is not a product - products are < 2^255 whenever the two operands multiply to
// less than 2^515.  F2 = Fq2: every result tightened, nothing to track.  Coordinates of stored points are "tight" (< 2^255).
#pragma once
#include <cstdint>
#include "bn254_f29.hpp"

namespace nlx {
namespace msm {

using f29::F1;
using f29::F2;
using f29::Fe;
template <class F> struct AffT { typename F::T x, y; };        // both exactly zero: the point at infinity
template <class F> struct JacT { typename F::T x, y, z; };     // z exactly zero: the point at infinity
template <class F> struct JacWordsT { uint32_t x[F::WORDS], y[F::WORDS], z[F::WORDS]; };   // canonical integers, for the host's tail
// How the converted points rest in memory: the coordinates (tight, below 2^255) re-sliced into eight 32-bit words per base
// field element - 64 bytes per G1 point, one aligned access per gathered point (as 72 bytes of limbs a point straddled two
// 128-byte lines: the bucket kernel fetched 67 GB for 2^28 gathered points, PMC FETCH_SIZE); 128 bytes per G2 point.
template <class F> struct __attribute__((aligned(64))) PackedT { uint32_t x[F::WORDS], y[F::WORDS]; };
template <class F> __device__ __forceinline__ AffT<F> unpack(const PackedT<F>& p) { return AffT<F>{F::from_words(p.x), F::from_words(p.y)}; }
typedef AffT<F1> Aff29;
typedef JacT<F1> Jac29;
typedef PackedT<F1> AffPacked;

template <class F> __device__ __forceinline__ bool is_inf(const AffT<F>& p) { return F::is_zero_exact(p.x) && F::is_zero_exact(p.y); }
template <class F> __device__ __forceinline__ JacT<F> inf29() { return JacT<F>{F::one(), F::one(), F::zero()}; }

template <class F>
__device__ __noinline__ JacT<F> jdbl29(const JacT<F>& p) {   // rare in the bucket kernel (a bucket receiving its own sum): kept out of line
    typedef typename F::T T;
    if (F::is_zero_exact(p.z)) return p;
    const T a = F::sqr(p.x), b = F::sqr(p.y), c = F::sqr(b);
    const T d = F::dbl(F::tighten(F::template sub<8>(F::sqr(F::add(p.x, b)), F::add(a, c))));   // (x + b)^2 - a - c: the subtrahend < 2^256; d < 2.2 q
    const T e = F::add(F::dbl(a), a);                                      // 3 a < 3 * 2^255
    JacT<F> r;
    r.x = F::tighten(F::template sub<8>(F::sqr(e), F::dbl(d)));            // 2 d < 2^256
    const T t = F::mul(e, F::template sub<4>(d, r.x));                     // d - x3 + 4 q < 2^256.3, times e < 2^256.6
    const T c4 = F::dbl(F::dbl(F::tighten(c)));                            // 4 c < 4.4 q: subtracted twice (8 c would pass 8 q)
    r.y = F::tighten(F::template sub<8>(F::tighten(F::template sub<8>(t, c4)), c4));
    r.z = F::tighten(F::dbl(F::mul(p.y, p.z)));
    return r;
}
// The mixed addition in place, common case only: returns 0 and leaves acc + q in acc, or - touching nothing - 1 if q is
// acc's own point (the sum is a doubling) or 2 if it is its negative (the sum is the point at infinity).  The rare cases
// are the caller's, OUTSIDE this function: with the doubling called from in here the result struct of the whole addition
// lived in scratch memory - 112 bytes written and read back per addition, 30 GB per 2^24-point MSM (PMC WRITE_SIZE).
template <class F>
__device__ __forceinline__ int jmadd29_common(JacT<F>& acc, const AffT<F>& q) {
    typedef typename F::T T;
    const T z1z1 = F::sqr(acc.z), u2 = F::mul(q.x, z1z1), s2 = F::mul(F::mul(q.y, acc.z), z1z1);
    const T h = F::template sub<4>(u2, acc.x), r0 = F::template sub<4>(s2, acc.y);   // < 2^255 + 4 q = 2^256.3
    if (F::is_zero_mod(h)) return F::is_zero_mod(r0) ? 1 : 2;
    const T r = F::dbl(r0);                                                           // < 2^257.3
    const T hh = F::sqr(h), i = F::dbl(F::dbl(hh)), j = F::mul(h, i), v = F::mul(acc.x, i);   // i < 2^257
    const T x3 = F::tighten(F::template sub<8>(F::sqr(r), F::add(j, F::dbl(v))));     // j + 2 v < 3 * 2^255 <= 8 q
    const T y3 = F::tighten(F::template sub<8>(F::mul(r, F::template sub<4>(v, x3)), F::dbl(F::mul(acc.y, j))));
    acc.z = F::tighten(F::template sub<8>(F::sqr(F::add(acc.z, h)), F::add(z1z1, hh)));   // z + h < 2^256.8
    acc.x = x3;
    acc.y = y3;
    return 0;
}
template <class F>
__device__ __forceinline__ JacT<F> jmadd29(const JacT<F>& p, const AffT<F>& q) {
    if (is_inf(q)) return p;
    if (F::is_zero_exact(p.z)) return JacT<F>{q.x, q.y, F::one()};
    JacT<F> o = p;
    const int st = jmadd29_common(o, q);
    if (st == 1) return jdbl29(JacT<F>{q.x, q.y, F::one()});
    if (st == 2) return inf29<F>();
    return o;
}
template <class F>
__device__ __forceinline__ JacT<F> jadd29(const JacT<F>& p, const JacT<F>& q) {
    typedef typename F::T T;
    if (F::is_zero_exact(p.z)) return q;
    if (F::is_zero_exact(q.z)) return p;
    const T z1z1 = F::sqr(p.z), z2z2 = F::sqr(q.z);
    const T u1 = F::mul(p.x, z2z2), u2 = F::mul(q.x, z1z1);
    const T s1 = F::mul(F::mul(p.y, q.z), z2z2), s2 = F::mul(F::mul(q.y, p.z), z1z1);
    const T h = F::template sub<4>(u2, u1), r0 = F::template sub<4>(s2, s1);
    if (F::is_zero_mod(h)) {
        if (F::is_zero_mod(r0)) return jdbl29(p);
        return inf29<F>();
    }
    const T r = F::dbl(r0);
    const T i = F::sqr(F::dbl(h)), j = F::mul(h, i), v = F::mul(u1, i);          // 2 h < 2^257.3
    JacT<F> o;
    o.x = F::tighten(F::template sub<8>(F::sqr(r), F::add(j, F::dbl(v))));
    o.y = F::tighten(F::template sub<8>(F::mul(r, F::template sub<4>(v, o.x)), F::dbl(F::mul(s1, j))));
    o.z = F::mul(F::template sub<8>(F::sqr(F::add(p.z, q.z)), F::add(z1z1, z2z2)), h);        // (< 2^257.1) (< 2^256.3)
    return o;
}
template <class F>
__device__ __forceinline__ JacT<F> jneg29(const JacT<F>& p) { return JacT<F>{p.x, F::tighten(F::template sub<4>(F::zero(), p.y)), p.z}; }

}  // namespace msm
}  // namespace nlx
