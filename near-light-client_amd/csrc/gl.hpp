// Goldilocks field F_p, p = 2^64 - 2^32 + 1, and its quadratic extension F_p[X]/(X^2 - 7),
// for gfx950 device code and for the C++ host orchestration (same source, both sides).
//
// Replaces plonky2_field::goldilocks_field::GoldilocksField and extension::quadratic
// (crate pinned at /root/reference/Cargo.lock:4912-4914; reached from every prover call
// behind nearx/src/test_utils.rs:62).  Written for CDNA4: there is no 64-bit integer MFMA, so
// a field multiply is four v_mad_u64_u32 plus a shift/add reduction that never divides.
//
// Representation: values in memory are canonical (< p).  Inside kernels a value may be any
// u64 congruent to the element ("loose"); functions say which they accept and return.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "nlx_field.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GL_HD __host__ __device__ __forceinline__
#define GL_H __host__ inline   // host half of a function that has a hand-written __device__ overload
#else
#define GL_HD inline
#define GL_H inline
#endif

namespace gl {

constexpr uint64_t P = 0xFFFFFFFF00000001ULL;
constexpr uint64_t EPS = 0xFFFFFFFFULL;  // 2^64 mod p
// the generator pair comes from include/nlx_field.h (one definition for product, oracle and golden model)
constexpr uint64_t GEN = NLX_GL_MULTIPLICATIVE_GROUP_GENERATOR;  // multiplicative generator = coset shift
constexpr uint64_t POW2_GEN = NLX_GL_POWER_OF_TWO_GENERATOR;     // order 2^32
constexpr unsigned TWO_ADICITY = 32;
constexpr uint64_t W = 7;  // X^2 = W in the quadratic extension

GL_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

#if defined(__HIP__)
// Device forms with hand-placed carries (overloads of the host forms below: clang resolves __host__ / __device__ per side).  Every vector instruction of this code issues at the same ~2 ns whatever it is
// (gl32.hpp), so the forms below are chosen by COUNT: hipcc's u64 code for the three functions needs 4 / 6 / 6.
// x + EPS carries out of 2^64 exactly when x >= P = 2^64 - EPS, and the sum is then x - P: one multiply-add (-1 * 1 + x,
// carry into an SGPR pair) and two selects.
__device__ __forceinline__ uint64_t canon(uint64_t a) {
    uint64_t t, c;
    asm("v_mad_u64_u32 %[t], %[c], -1, 1, %[a]" : [t] "=&v"(t), [c] "=s"(c) : [a] "v"(a));
    uint32_t r0, r1;
    asm("v_cndmask_b32_e64 %[r0], %[a0], %[t0], %[c]\n\t"
        "v_cndmask_b32_e64 %[r1], %[a1], %[t1], %[c]"
        : [r0] "=&v"(r0), [r1] "=v"(r1)
        : [a0] "v"((uint32_t)a), [a1] "v"((uint32_t)(a >> 32)), [t0] "v"((uint32_t)t), [t1] "v"((uint32_t)(t >> 32)), [c] "s"(c));
    return ((uint64_t)r1 << 32) | r0;
}
// canonical + canonical -> canonical: s = a + b, reduced when the addition carried or s >= P (5 vector instructions)
__device__ __forceinline__ uint64_t add(uint64_t a, uint64_t b) {
    uint32_t s0, s1;
    uint64_t c1, c2, t;
    asm("v_add_co_u32 %[s0], vcc, %[a0], %[b0]\n\t"
        "v_addc_co_u32 %[s1], %[c1], %[a1], %[b1], vcc"
        : [s0] "=&v"(s0), [s1] "=&v"(s1), [c1] "=s"(c1)
        : [a0] "v"((uint32_t)a), [a1] "v"((uint32_t)(a >> 32)), [b0] "v"((uint32_t)b), [b1] "v"((uint32_t)(b >> 32))
        : "vcc");
    const uint64_t s = ((uint64_t)s1 << 32) | s0;
    asm("v_mad_u64_u32 %[t], %[c], -1, 1, %[s]" : [t] "=&v"(t), [c] "=s"(c2) : [s] "v"(s));
    const uint64_t c = c1 | c2;
    uint32_t r0, r1;
    asm("v_cndmask_b32_e64 %[r0], %[s0], %[t0], %[c]\n\t"
        "v_cndmask_b32_e64 %[r1], %[s1], %[t1], %[c]"
        : [r0] "=&v"(r0), [r1] "=v"(r1)
        : [s0] "v"(s0), [s1] "v"(s1), [t0] "v"((uint32_t)t), [t1] "v"((uint32_t)(t >> 32)), [c] "s"(c));
    return ((uint64_t)r1 << 32) | r0;
}
// (any u64) - canonical -> a value congruent to the difference, canonical when a is: a borrow is worth -EPS, and
// a - b + 2^64 >= 2^64 - (P - 1) > EPS, so the correction cannot borrow again (5 vector instructions)
__device__ __forceinline__ uint64_t sub(uint64_t a, uint64_t b) {
    uint32_t d0, d1, m;
    asm("v_sub_co_u32 %[d0], vcc, %[a0], %[b0]\n\t"
        "v_subb_co_u32 %[d1], vcc, %[a1], %[b1], vcc\n\t"
        "v_cndmask_b32_e64 %[m], 0, -1, vcc\n\t"
        "v_sub_co_u32 %[d0], vcc, %[d0], %[m]\n\t"
        "v_subbrev_co_u32 %[d1], vcc, 0, %[d1], vcc"
        : [d0] "=&v"(d0), [d1] "=&v"(d1), [m] "=&v"(m)
        : [a0] "v"((uint32_t)a), [a1] "v"((uint32_t)(a >> 32)), [b0] "v"((uint32_t)b), [b1] "v"((uint32_t)(b >> 32))
        : "vcc");
    return ((uint64_t)d1 << 32) | d0;
}
#endif
GL_H uint64_t canon(uint64_t a) { return a >= P ? a - P : a; }

// canonical + canonical -> canonical
GL_H uint64_t add(uint64_t a, uint64_t b) {
    uint64_t s = a + b;
    return (s < a || s >= P) ? s - P : s;
}
// canonical - canonical -> canonical
GL_H uint64_t sub(uint64_t a, uint64_t b) {
    uint64_t d = a - b;
    return a < b ? d + P : d;
}
GL_HD uint64_t neg(uint64_t a) { return a ? P - a : 0; }

// loose + canonical -> loose (single conditional fix-up; see plonky2 GoldilocksField::add)
#if defined(__HIP__)
// four vector instructions: the carry becomes a mask, and mask * 1 + s adds EPS where it is set
__device__ __forceinline__ uint64_t add_loose(uint64_t a, uint64_t c) {
    uint32_t s0, s1, m;
    asm("v_add_co_u32 %[s0], vcc, %[a0], %[c0]\n\t"
        "v_addc_co_u32 %[s1], vcc, %[a1], %[c1], vcc\n\t"
        "v_cndmask_b32_e64 %[m], 0, -1, vcc"
        : [s0] "=&v"(s0), [s1] "=&v"(s1), [m] "=v"(m)
        : [a0] "v"((uint32_t)a), [a1] "v"((uint32_t)(a >> 32)), [c0] "v"((uint32_t)c), [c1] "v"((uint32_t)(c >> 32))
        : "vcc");
    uint64_t r;
    asm("v_mad_u64_u32 %[r], vcc, %[m], 1, %[s]" : [r] "=&v"(r) : [m] "v"(m), [s] "v"(((uint64_t)s1 << 32) | s0) : "vcc");
    return r;
}
#endif
GL_H uint64_t add_loose(uint64_t a, uint64_t c) {
    uint64_t s = a + c;
    return s < a ? s + EPS : s;
}

// (hi:lo) mod p, any 128-bit input -> loose u64
GL_HD uint64_t reduce128_loose(uint64_t lo, uint64_t hi) {
    uint64_t hi_hi = hi >> 32, hi_lo = hi & EPS;
    uint64_t t0 = lo - hi_hi;
    if (lo < hi_hi) t0 -= EPS;
    uint64_t t1 = (hi_lo << 32) - hi_lo;  // hi_lo * (2^32 - 1)
    uint64_t r = t0 + t1;
    if (r < t1) r += EPS;
    return r;
}
GL_HD uint64_t reduce128(uint64_t lo, uint64_t hi) { return canon(reduce128_loose(lo, hi)); }

#if defined(__HIP__)
// ---- the ONE product chain and the ONE reduction of the device code ----------------------------------------------------------
// 64x64 -> 128 product and Goldilocks reduction in 14 vector instructions (16 up to round 4; hipcc's u64 code needs 29; see
// gl32.hpp for the measurements behind counting instructions and DESIGN §38 for this form).  The product is a chain of four
// multiply-adds, the third of which is ALLOWED to overflow:
//   p0 = a0 b0;  p1 = a0 b1 + hi(p0);  p2 = a1 b0 + p1 [carry k -> an SGPR pair];  p3 = a1 b1 + hi(p2)
//   a b = w0 + 2^32 w1 + 2^64 (w3:w2) + 2^96 k     (w0 = lo(p0), w1 = lo(p2), (w3:w2) = p3; w3 + k <= 2^32 - 1)
// p1 is a whole 64-bit addend, so only the two zero-extended high words cost a v_mov.  2^96 = -1 (mod p): k is the borrow-in of
// the reduction's first subtraction and costs no instruction.  -DNLX_FIELD_MUL_PARENT builds the form of round 4 for A/B runs:
// five multiply-adds none of which can overflow (p2 = a1 b0 + lo(p1), p3 = a1 b1 + hi(p1) + hi(p2)), three moves, no k.
#if defined(NLX_FIELD_MUL_PARENT)
constexpr bool MUL_HAS_K = false;
#else
constexpr bool MUL_HAS_K = true;
#endif
struct Wide128 {
    uint32_t w0, w1;
    uint64_t w32;  // limbs 2 and 3
    uint64_t k;    // lane mask of the carry of weight 2^96 that is NOT in w32 (meaningful when MUL_HAS_K)
};
__device__ __forceinline__ Wide128 mul_chain(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    // plain C++ where it can be: hipcc selects exactly v_mad_u64_u32 with a (value : 0) register pair for each addend and spaces
    // nothing (between asm statements it puts an s_nop)
    const uint64_t p0 = (uint64_t)a0 * b0;
    const uint64_t p1 = (uint64_t)a0 * b1 + (p0 >> 32);
#if defined(NLX_FIELD_MUL_PARENT)
    const uint64_t p2 = (uint64_t)a1 * b0 + (uint32_t)p1;
    uint64_t p3 = (uint64_t)a1 * b1 + (p1 >> 32), sink;
    asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(p3), "=s"(sink) : "v"((uint32_t)(p2 >> 32)), "v"(p3));   // x * 1 + c saves the pair
    return Wide128{(uint32_t)p0, (uint32_t)p2, p3, 0};
#else
    uint64_t p2, k;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(p2), "=&s"(k) : "v"(a1), "v"(b0), "v"(p1));
    const uint64_t p3 = (uint64_t)a1 * b1 + (p2 >> 32);   // cannot overflow: (2^32 - 1)^2 + 2^32 - 1 < 2^64
    return Wide128{(uint32_t)p0, (uint32_t)p2, p3, k};
#endif
}
// the product with k folded into limb 3 (one add-with-carry), for callers that add products as integers
__device__ __forceinline__ Wide128 fold_k(Wide128 x) {
#if !defined(NLX_FIELD_MUL_PARENT)
    uint32_t w3;
    uint64_t sink;
    asm("v_addc_co_u32_e64 %0, %1, 0, %2, %3" : "=v"(w3), "=&s"(sink) : "v"((uint32_t)(x.w32 >> 32)), "s"(x.k));
    x.w32 = ((uint64_t)w3 << 32) | (uint32_t)x.w32;
#endif
    return x;
}

// (w3 : w2 : w1 : w0) - 2^96 k mod p, any four 32-bit limbs (k: a lane mask with w3 + k <= 2^32 - 1, read only when HAS_K) -> loose
//   r = (w1:w0) - w3 - k [borrow b -> -EPS] + w2 EPS [carry -> +EPS]        2^64 = EPS, 2^96 = -1 (mod p)
// Eight instructions: three for the subtraction's borrow repair; w2 EPS is ONE multiply-add (carry-out in VCC), carry -> mask,
// mask * 1 + r (on gfx950 every VCC-chained add issues as slowly as a multiply, profiles/r02_valu_ubench.txt).
// -DNLX_FIELD_REDUCE7: seven.  The repair is worth b P = b (2^64 - EPS), so (w2 - b) EPS + r is the same value - except when
// w2 = 0 with a borrow (e.g. 2^63 * 2^33): m = w2 - b wraps to 2^32 - 1 and the sum is short by exactly 1.  That borrow-out
// (`bad`, an SGPR pair) is the carry-in of the final + EPS, which is then two add-with-carry instead of a multiply-add.
// No carry crosses an asm statement in VCC: k and bad are SGPR-pair operands.
#define NLX_GL_SUB_W3_K "v_subb_co_u32_e64 %[r0], vcc, %[w0], %[w3], %[k]\n\t"
#define NLX_GL_SUB_W3 "v_sub_co_u32 %[r0], vcc, %[w0], %[w3]\n\t"
template <bool HAS_K>
__device__ __forceinline__ uint64_t reduce128_core(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint64_t k) {
#if !defined(NLX_FIELD_REDUCE7)
#define NLX_GL_REPAIR                                \
    "v_subbrev_co_u32 %[r1], vcc, 0, %[w1], vcc\n\t" \
    "v_cndmask_b32_e64 %[t0], 0, -1, vcc\n\t"        \
    "v_sub_co_u32 %[r0], vcc, %[r0], %[t0]\n\t"      \
    "v_subbrev_co_u32 %[r1], vcc, 0, %[r1], vcc"
    uint32_t r0, r1, t0;
    if constexpr (HAS_K)
        asm(NLX_GL_SUB_W3_K NLX_GL_REPAIR
            : [r0] "=&v"(r0), [r1] "=&v"(r1), [t0] "=&v"(t0)
            : [w0] "v"(w0), [w1] "v"(w1), [w3] "v"(w3), [k] "s"(k)
            : "vcc");
    else
        asm(NLX_GL_SUB_W3 NLX_GL_REPAIR
            : [r0] "=&v"(r0), [r1] "=&v"(r1), [t0] "=&v"(t0)
            : [w0] "v"(w0), [w1] "v"(w1), [w3] "v"(w3)
            : "vcc");
#undef NLX_GL_REPAIR
    const uint64_t base = ((uint64_t)r1 << 32) | r0;
    uint64_t r;
    uint32_t tm;
    asm("v_mad_u64_u32 %[r], vcc, %[w2], -1, %[base]\n\t"
        "v_cndmask_b32_e64 %[t], 0, -1, vcc\n\t"
        "v_mad_u64_u32 %[r], vcc, %[t], 1, %[r]"
        : [r] "=&v"(r), [t] "=&v"(tm)
        : [w2] "v"(w2), [base] "v"(base)
        : "vcc");
    return r;
#else
#define NLX_GL_REPAIR                                \
    "v_subbrev_co_u32 %[r1], vcc, 0, %[w1], vcc\n\t" \
    "v_subbrev_co_u32_e64 %[m], %[bad], 0, %[w2], vcc"
    uint32_t r0, r1, m;
    uint64_t bad;
    if constexpr (HAS_K)
        asm(NLX_GL_SUB_W3_K NLX_GL_REPAIR
            : [r0] "=&v"(r0), [r1] "=&v"(r1), [m] "=&v"(m), [bad] "=&s"(bad)
            : [w0] "v"(w0), [w1] "v"(w1), [w2] "v"(w2), [w3] "v"(w3), [k] "s"(k)
            : "vcc");
    else
        asm(NLX_GL_SUB_W3 NLX_GL_REPAIR
            : [r0] "=&v"(r0), [r1] "=&v"(r1), [m] "=&v"(m), [bad] "=&s"(bad)
            : [w0] "v"(w0), [w1] "v"(w1), [w2] "v"(w2), [w3] "v"(w3)
            : "vcc");
#undef NLX_GL_REPAIR
    const uint64_t base = ((uint64_t)r1 << 32) | r0;
    uint64_t u;
    uint32_t t, lo, hi;
    asm("v_mad_u64_u32 %[u], vcc, %[m], -1, %[base]\n\t"
        "v_cndmask_b32_e64 %[t], 0, -1, vcc"
        : [u] "=&v"(u), [t] "=&v"(t)
        : [m] "v"(m), [base] "v"(base)
        : "vcc");
    asm("v_addc_co_u32_e64 %[lo], vcc, %[u0], %[t], %[bad]\n\t"
        "v_addc_co_u32 %[hi], vcc, 0, %[u1], vcc"
        : [lo] "=&v"(lo), [hi] "=v"(hi)
        : [u0] "v"((uint32_t)u), [u1] "v"((uint32_t)(u >> 32)), [t] "v"(t), [bad] "s"(bad)
        : "vcc");
    return ((uint64_t)hi << 32) | lo;
#endif
}
#undef NLX_GL_SUB_W3_K
#undef NLX_GL_SUB_W3

// loose * loose -> loose
__device__ __forceinline__ uint64_t mul_loose_asm(uint64_t a, uint64_t b) {
    const Wide128 x = mul_chain((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    return reduce128_core<MUL_HAS_K>(x.w0, x.w1, (uint32_t)x.w32, (uint32_t)(x.w32 >> 32), x.k);
}

// (w4 : w3 : w2 : w1 : w0) - 2^96 k mod p, any five 32-bit limbs -> canonical.  2^128 = -2^32:
//   the four low limbs by reduce128_core, made canonical, minus w4 2^32 (canonical for every w4: at most P - 1).
// One reduction for a whole sum of products: GateAcc's columns (prover_kernels.hip) and the extension product below.
// reduce160_loose skips the canonical step: sub takes any u64 on its left, and the result is any u64 congruent to the value.
template <bool CANON, bool HAS_K = false>
__device__ __forceinline__ uint64_t reduce160_impl(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint64_t k = 0) {
    const uint64_t r = reduce128_core<HAS_K>(w0, w1, w2, w3, k);
    return sub(CANON ? canon(r) : r, (uint64_t)w4 << 32);
}
__device__ __forceinline__ uint64_t reduce160(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4) {
    return reduce160_impl<true>(w0, w1, w2, w3, w4);
}
__device__ __forceinline__ uint64_t reduce160_loose(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4) {
    return reduce160_impl<false>(w0, w1, w2, w3, w4);
}
// the full 128-bit product (w32 : w1 : w0) + 2^96 k; a caller that reduces the product (or a sum it is part of) right away hands
// k to the reduction, which takes one k for nothing; any further product's k goes into its limb 3 by fold_k (7 instructions, 8 before)
__device__ __forceinline__ Wide128 mul_wide(uint64_t a, uint64_t b) {
    return mul_chain((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}
#endif

// loose * loose -> loose
GL_HD uint64_t mul_loose(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return mul_loose_asm(a, b);
#else
    return reduce128_loose(a * b, mulhi64(a, b));
#endif
}
// any * any -> canonical
GL_HD uint64_t mul(uint64_t a, uint64_t b) { return canon(mul_loose(a, b)); }
GL_HD uint64_t sqr(uint64_t a) { return mul(a, a); }

GL_HD uint64_t pow(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    while (e) {
        if (e & 1) r = mul(r, b);
        b = sqr(b);
        e >>= 1;
    }
    return r;
}
GL_HD uint64_t exp_pow2(uint64_t a, unsigned k) {
    while (k--) a = sqr(a);
    return a;
}
// a^(p-2); addition chain: p-2 = 2^64 - 2^32 - 1  (72 multiplications)
GL_HD uint64_t inv(uint64_t a) {
    // t_k = a^(2^k - 1)
    uint64_t t2 = mul(sqr(a), a);
    uint64_t t3 = mul(sqr(t2), a);
    uint64_t t6 = mul(exp_pow2(t3, 3), t3);
    uint64_t t12 = mul(exp_pow2(t6, 6), t6);
    uint64_t t24 = mul(exp_pow2(t12, 12), t12);
    uint64_t t30 = mul(exp_pow2(t24, 6), t6);
    uint64_t t31 = mul(sqr(t30), a);
    // p - 2 = (2^31 - 1) * 2^33 + (2^32 - 1)   [= 2^64 - 2^33 + 2^32 - 1]
    uint64_t t32 = mul(sqr(t31), a);
    return mul(exp_pow2(t31, 33), t32);
}
GL_HD uint64_t root_of_unity(unsigned n_log) { return exp_pow2(POW2_GEN, TWO_ADICITY - n_log); }

// ---- quadratic extension ----
struct Ext {
    uint64_t a, b;  // a + b X, canonical
};
GL_HD Ext ext(uint64_t a, uint64_t b = 0) { return Ext{a, b}; }
GL_HD Ext add(Ext x, Ext y) { return Ext{add(x.a, y.a), add(x.b, y.b)}; }
GL_HD Ext sub(Ext x, Ext y) { return Ext{sub(x.a, y.a), sub(x.b, y.b)}; }
#if defined(__HIP__)
// Device form, any u64 in, canonical out: the four 128-bit products are ADDED AS INTEGERS and each component is reduced once
//   c1 = a0 b1 + a1 b0 < 2^129;   c0 = a0 b0 + 7 a1 b1 < 2^131   (fifth limb < 2 and < 8)
// instead of four canonical multiplies, a generic 7 * bb and two canonical adds (98 vector instructions measured; this is 82).  The
// product by 7 rides on the addition: limb_i * 7 + q_i + carry <= 8 (2^32 - 1) + 7 fits 64 bits, so the chain never overflows.
template <bool CANON>
__device__ __forceinline__ Ext mul_impl(Ext x, Ext y) {
    const Wide128 ab = mul_wide(x.a, y.b), ba = fold_k(mul_wide(x.b, y.a));   // ab's k: the reduction's borrow-in
    uint32_t s0, s1, s2, s3, s4;
    asm("v_add_co_u32 %[s0], vcc, %[x0], %[y0]\n\t"
        "v_addc_co_u32 %[s1], vcc, %[x1], %[y1], vcc\n\t"
        "v_addc_co_u32 %[s2], vcc, %[x2], %[y2], vcc\n\t"
        "v_addc_co_u32 %[s3], vcc, %[x3], %[y3], vcc\n\t"
        "v_addc_co_u32 %[s4], vcc, 0, 0, vcc"
        : [s0] "=&v"(s0), [s1] "=&v"(s1), [s2] "=&v"(s2), [s3] "=&v"(s3), [s4] "=&v"(s4)
        : [x0] "v"(ab.w0), [x1] "v"(ab.w1), [x2] "v"((uint32_t)ab.w32), [x3] "v"((uint32_t)(ab.w32 >> 32)), [y0] "v"(ba.w0),
          [y1] "v"(ba.w1), [y2] "v"((uint32_t)ba.w32), [y3] "v"((uint32_t)(ba.w32 >> 32))
        : "vcc");
    const uint64_t c1 = reduce160_impl<CANON, MUL_HAS_K>(s0, s1, s2, s3, s4, ab.k);
    // one component at a time: with all four products in flight a caller holds 16 more registers (k_fri_fold lost a wave)
    __builtin_amdgcn_sched_barrier(0);
    const Wide128 aa = mul_wide(x.a, y.a), bb = fold_k(mul_wide(x.b, y.b));   // bb's k would weigh 7 * 2^96: into its limb 3
    const uint64_t t0 = (uint64_t)bb.w0 * (uint32_t)W + aa.w0;
    const uint64_t t1 = (uint64_t)bb.w1 * (uint32_t)W + (((uint64_t)aa.w1) + (t0 >> 32));
    const uint64_t t2 = (uint64_t)(uint32_t)bb.w32 * (uint32_t)W + ((aa.w32 & EPS) + (t1 >> 32));
    const uint64_t t3 = (uint64_t)(uint32_t)(bb.w32 >> 32) * (uint32_t)W + ((aa.w32 >> 32) + (t2 >> 32));
    const uint64_t c0 = reduce160_impl<CANON, MUL_HAS_K>((uint32_t)t0, (uint32_t)t1, (uint32_t)t2, (uint32_t)t3, (uint32_t)(t3 >> 32), aa.k);
    return Ext{c0, c1};
}
__device__ __forceinline__ Ext mul(Ext x, Ext y) { return mul_impl<true>(x, y); }
// any u64 in, LOOSE out (three instructions fewer per component): for products that only feed another multiply, the left of a
// sub or the first operand of add_loose
__device__ __forceinline__ Ext mul_loose(Ext x, Ext y) { return mul_impl<false>(x, y); }
#endif
GL_H Ext mul(Ext x, Ext y) {
    uint64_t bb = mul(x.b, y.b);
    // 7*bb without a full multiply: 8*bb - bb, done in 128 bits
    uint64_t c0 = add(mul(x.a, y.a), reduce128(bb * W, mulhi64(bb, W)));
    uint64_t c1 = add(mul(x.a, y.b), mul(x.b, y.a));
    return Ext{c0, c1};
}
GL_HD Ext mul(Ext x, uint64_t s) { return Ext{mul(x.a, s), mul(x.b, s)}; }
GL_HD Ext inv(Ext x) {
    uint64_t n = sub(sqr(x.a), mul(W, sqr(x.b)));
    uint64_t ni = inv(n);
    return Ext{mul(x.a, ni), mul(neg(x.b), ni)};
}
GL_HD Ext pow(Ext b, uint64_t e) {
    Ext r{1, 0};
    while (e) {
        if (e & 1) r = mul(r, b);
        b = mul(b, b);
        e >>= 1;
    }
    return r;
}
GL_HD bool eq(Ext x, Ext y) { return x.a == y.a && x.b == y.b; }

GL_HD uint32_t bitrev32(uint32_t x, unsigned bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
    uint32_t r = 0;
    for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
#endif
}

}  // namespace gl
