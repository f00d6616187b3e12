// Row f.4, third piece: the PLONK prover's quotient chain and one KZG opening over BN254's scalar field, on the pieces that
// exist (nlx_bn254_ntt_batch_coset: FFTInverse(DIF) / FFT(DIT, OnCoset); nlx_bn254_msm_g1).
//
// What the recursive wrap's prover (gnark backend/plonk/bn254 `Prove`, reached through succinct.json:7-8's entry point; Go,
// not in /root/reference) does between its commitments, restated from the published protocol (Gabizon-Williamson-Ciobotaru,
// "PLONK", the three-wire arithmetisation gnark implements), NOT from gnark's source - no blinding, no gnark byte format:
//   1. the thirteen polynomials it knows by their values on H (selectors ql qr qm qo qk, permutation s1 s2 s3, wires l r o,
//      grand product z, public-input polynomial) go to coefficients:           FFTInverse(DIF), no reordering
//   2. and from there to the coset shift * <w_4n> of four times the size:       FFT(DIT, OnCoset)
//   3. one pointwise pass builds the quotient's values there
//        t = [ ql l + qr r + qm l r + qo o + qk + pi
//              + alpha ( (l + beta x + gamma)(r + beta k1 x + gamma)(o + beta k2 x + gamma) z
//                        - (l + beta s1 + gamma)(r + beta s2 + gamma)(o + beta s3 + gamma) z(w x) )
//              + alpha^2 L1(x) (z - 1) ] / Z_H(x)
//   4. FFTInverse(OnCoset) gives t's coefficients: three chunks of n (the fourth is zero exactly when the witness satisfies
//      the circuit - reported, not assumed)
//   5. KZG: commitments are nlx_bn254_msm_g1 over the SRS; an opening at zeta is the evaluation, the synthetic division
//      (p(X) - p(zeta)) / (X - zeta) and one more MSM.
// gnark's additions to that chain are opt-in flags of nlx_bn254_plonk_quotient: NLX_BN254_PLONK_BLINDED (l r o z blinded by
// multiples of X^n - 1) and NLX_BN254_PLONK_COMMIT (Bsb22 commitments: the gate also carries sum_j qcp_j pi2_j, the 2 k extra
// polynomials taking steps 1 and 2 like the thirteen).
//
// Arithmetic: bn254_f29.hpp's nine 29-bit limbs (the NTT's and the MSM's element), every sum / difference tightened.  Elements
// rest in memory as gnark-crypto's fr.Element (Montgomery, R = 2^256: "D-form", x 2^256); the kernels' products divide by
// R' = 2^261, so uniform constants and the domain tables are kept in "I-form" (x 2^261): D x I -> D, I x I -> I, and only a
// product of two data values needs the factor 2^5 put back (x32).
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>
#include "ctx.hpp"
#include "bn254_f29.hpp"
#include "bn254_plonk.hpp"

namespace nlx {
namespace bnp {

using f29::Fe;
typedef f29::RMod RM;

__device__ __forceinline__ Fe ld(const uint64_t* p, size_t i) { return f29::load(p, i); }
__device__ __forceinline__ void st(uint64_t* p, size_t i, const Fe& v) { f29::store(p, i, f29::canonical<RM>(v)); }   // canonical: what gnark keeps in memory
__device__ __forceinline__ Fe mul(const Fe& a, const Fe& b) { return f29::mul<RM>(a, b); }
__device__ __forceinline__ Fe add(const Fe& a, const Fe& b) { return f29::tighten<RM>(f29::add(a, b)); }
__device__ __forceinline__ Fe sub(const Fe& a, const Fe& b) { return f29::tighten<RM>(f29::sub<4, RM>(a, b)); }
// x 2^5: D x D products come out as x y 2^251 (f29::x32: times 4, tightened, times 8, tightened)
__device__ __forceinline__ Fe x32(const Fe& a) { return f29::x32<RM>(a); }
__device__ __forceinline__ Fe mul_dd(const Fe& a, const Fe& b) { return x32(mul(a, b)); }   // D x D -> D
__device__ __forceinline__ Fe one_i() { return f29::one<RM>(); }
__device__ __forceinline__ Fe one_d() {   // 2^256 mod r
    constexpr uint32_t C[f29::NL] = {0x0ffffffbu, 0x04b1a0e2u, 0x18334a6bu, 0x18ed2b3eu, 0x1462e36fu, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
    Fe r;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) r.v[i] = C[i];
    return r;
}
__device__ __forceinline__ Fe root28_i() {   // gnark-crypto's 2^28-th root of unity 5^((r-1)/2^28), I-form
    constexpr uint32_t C[f29::NL] = {0x1a27b370u, 0x1d788b88u, 0x0a3c6e0bu, 0x1fd3f9dau, 0x0f541c23u, 0x1e4ddf15u, 0x093d0e83u, 0x0ae32ca7u, 0x0005d90bu};
    Fe r;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) r.v[i] = C[i];
    return r;
}
__device__ Fe pow_i(Fe b, uint64_t e) {   // I-form power
    Fe r = one_i();
    while (e) {
        if (e & 1) r = mul(r, b);
        b = mul(b, b);
        e >>= 1;
    }
    return r;
}
__device__ Fe inv_i(const Fe& a) {   // a^(r - 2), I-form in and out
    const uint64_t E[4] = {0x43e1f593efffffffull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    Fe r = one_i(), b = a;
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        uint64_t e = E[w];
#pragma unroll 1
        for (int i = 0; i < 64; i++) {
            if (e & 1) r = mul(r, b);
            b = mul(b, b);
            e >>= 1;
        }
    }
    return r;
}

// the uniform values of one quotient call, made once on the device
struct Consts {
    Fe w4n, shift, alpha, alpha2, beta_d, beta_k1_d, beta_k2_d, gamma_d, n_i;   // _d: D-form, the rest I-form
    Fe zh_inv[4];    // 1 / (x^n - 1) on the coset: x^n = shift^n i^(k mod 4)
};
struct QuotientParams {
    // evaluations on the coset, natural order, [4n] each, in two groups (a resident key keeps the first one across proofs):
    const uint64_t* ev_fixed;   // [8 + n_commit]: ql qr qm qo qk s1 s2 s3 (qcp_0 ..)
    const uint64_t* ev_proof;   // [4 + has_pi + n_commit]: l r o z (pi) (pi2_0 ..)
    const uint64_t* x;    // [4n] the points, I-form
    const uint64_t* linv; // [4n] 1 / (n (x - 1)), I-form
    const Consts* k;
    uint64_t* t;          // [4n]
    uint32_t log_n, has_pi;
    uint32_t n_commit;    // Bsb22 commitments (NLX_BN254_PLONK_COMMIT): read by k_plonk_quotient<true> only
};

// bad: set to 1 when Z_H vanishes on the coset (the shift lies in the size-4n subgroup): inv_i(0) = 0 would otherwise give a
// silently wrong quotient
__global__ void k_plonk_consts(Consts* out, uint32_t log_n, const uint64_t* in /* shift k1 k2 alpha beta gamma, D-form words */, uint32_t* bad) {
    if (threadIdx.x || blockIdx.x) return;
    Consts k;
    Fe w = root28_i();
    for (uint32_t i = log_n + 2; i < 28; i++) w = mul(w, w);
    k.w4n = w;
    k.shift = x32(ld(in, 0));
    const Fe k1 = x32(ld(in, 1)), k2 = x32(ld(in, 2));
    k.alpha = x32(ld(in, 3));
    k.alpha2 = mul(k.alpha, k.alpha);
    k.beta_d = ld(in, 4);
    k.beta_k1_d = mul(k.beta_d, k1);
    k.beta_k2_d = mul(k.beta_d, k2);
    k.gamma_d = ld(in, 5);
    Fe n = one_i();
    for (uint32_t i = 0; i < log_n; i++) n = add(n, n);
    k.n_i = n;
    const Fe sn = pow_i(k.shift, (uint64_t)1 << log_n), j = pow_i(w, (uint64_t)1 << log_n);   // j: a primitive 4th root of unity
    Fe jk = one_i();
    for (int q = 0; q < 4; q++) {
        const Fe den = sub(mul(sn, jk), one_i());
        if (f29::is_zero_mod<RM>(den)) *bad = 1;
        k.zh_inv[q] = inv_i(den);
        jk = mul(jk, j);
    }
    *out = k;
}

// One lane per run of DOMAIN_RUN points: x_i = shift w^i (one power, then a product per point) and 1 / (n (x_i - 1)) by
// Montgomery's batch inversion over the run (prefix products parked in the output, one inversion per run).
constexpr uint32_t DOMAIN_RUN = 64;
__global__ __launch_bounds__(64) void k_plonk_domain(const Consts* __restrict__ kp, uint32_t log_n, uint64_t* __restrict__ x_out,
                                                     uint64_t* __restrict__ linv_out) {
    const size_t N4 = (size_t)4 << log_n;
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * DOMAIN_RUN;
    if (i0 >= N4) return;
    const size_t i1 = i0 + DOMAIN_RUN < N4 ? i0 + DOMAIN_RUN : N4;
    const Fe w = kp->w4n, n = kp->n_i, one = one_i();
    Fe x = mul(kp->shift, pow_i(w, i0)), acc = one;
#pragma unroll 1
    for (size_t i = i0; i < i1; i++) {
        st(x_out, i, x);
        acc = mul(acc, mul(n, sub(x, one)));
        st(linv_out, i, acc);
        x = mul(x, w);
    }
    Fe inv = inv_i(acc);
#pragma unroll 1
    for (size_t i = i1; i-- > i0;) {
        const Fe v = mul(n, sub(ld(x_out, i), one));
        const Fe prev = i > i0 ? ld(linv_out, i - 1) : one;
        st(linv_out, i, mul(inv, prev));
        inv = mul(inv, v);
    }
}

// Coefficients in natural order (len of them, len <= 4n) -> their places in the zero-filled 4n-array the coset FFT (DIT) reads
__global__ __launch_bounds__(256) void k_plonk_place_coeffs(const uint64_t* __restrict__ coeffs, size_t len, uint32_t log_n, uint64_t* __restrict__ col) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const uint32_t pos = __brev((uint32_t)i) >> (32 - (log_n + 2));
    const uint4* q = reinterpret_cast<const uint4*>(coeffs + 4 * i);
    uint4* d = reinterpret_cast<uint4*>(col + 4 * (size_t)pos);
    d[0] = q[0];
    d[1] = q[1];
}

// Blinding in coefficient form: p(X) += (b_0 + b_1 X + ...)(X^n - 1), i.e. coefficient i loses b_i and coefficient n + i gains it.
// The coefficients lie in the 4n-array in bit-reversed order (what the coset FFT (DIT) reads): one lane per touched coefficient.
// ev: the per-proof group [l r o z ..][4n] elements; job t = (poly, i, sign) for the nine blinding scalars b (D-form words, in
// order l l r r o o z z z).
__global__ void k_plonk_blind(uint64_t* __restrict__ ev, const uint64_t* __restrict__ b, uint32_t log_n) {
    const uint32_t t = threadIdx.x;
    if (t >= 18) return;
    const uint32_t j = t >> 1, add_side = t & 1;                   // scalar j, the - b_i (0) or the + b_i (1) side
    const uint32_t poly = j < 6 ? (j >> 1) : 3, i = j < 6 ? (j & 1) : j - 6;
    const size_t N4 = (size_t)4 << log_n;
    const uint32_t idx = (add_side ? ((uint32_t)1 << log_n) : 0u) + i;
    const uint32_t pos = __brev(idx) >> (32 - (log_n + 2));
    uint64_t* col = ev + (size_t)poly * N4 * 4;
    const Fe cur = ld(col, pos), bj = ld(b, j);
    st(col, pos, add_side ? add(cur, bj) : sub(cur, bj));
}

// COMMIT: the gate also carries sum_j qcp_j pi2_j (gnark's Bsb22 commitments).  A template, so that the instantiation without
// commitments stays the kernel it was; with them the trip count comes from the params (wave-uniform, no per-lane branching).
template <bool COMMIT>
__global__ __launch_bounds__(256) void k_plonk_quotient(QuotientParams p) {
    const size_t N4 = (size_t)4 << p.log_n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N4) return;
    const Consts& k = *p.k;
    auto E = [&](int poly, size_t at) { return ld(p.ev_fixed + (size_t)poly * 4 * N4, at); };   // canonical words: already tight
    auto W = [&](int poly, size_t at) { return ld(p.ev_proof + (size_t)poly * 4 * N4, at); };
    const Fe l = W(0, i), r = W(1, i), o = W(2, i);
    // gate: ql l + qr r + qm l r + qo o + qk (+ pi); every product of two data values is put back into D-form
    Fe gate = mul_dd(E(0, i), l);
    gate = add(gate, mul_dd(E(1, i), r));
    gate = add(gate, mul_dd(E(2, i), mul_dd(l, r)));
    gate = add(gate, mul_dd(E(3, i), o));
    gate = add(gate, E(4, i));
    if (p.has_pi) gate = add(gate, W(4, i));
    if constexpr (COMMIT) {
        const int base = 4 + (int)p.has_pi, nc = (int)p.n_commit;
#pragma unroll 1
        for (int j = 0; j < nc; j++) gate = add(gate, mul_dd(E(8 + j, i), W(base + j, i)));
    }
    // permutation: the identity side on x, k1 x, k2 x and the sigma side on s1, s2, s3; z at the next point of the size-n
    // subgroup = four positions further on the size-4n coset
    const Fe x = ld(p.x, i), g = k.gamma_d;
    const Fe z = W(3, i), zn = W(3, (i + 4) & (N4 - 1));
    Fe f = mul_dd(add(add(l, mul(k.beta_d, x)), g), add(add(r, mul(k.beta_k1_d, x)), g));
    f = mul_dd(f, add(add(o, mul(k.beta_k2_d, x)), g));
    f = mul_dd(f, z);
    const Fe bi = x32(k.beta_d);   // beta, I-form: times a data value stays data
    Fe h = mul_dd(add(add(l, mul(E(5, i), bi)), g), add(add(r, mul(E(6, i), bi)), g));
    h = mul_dd(h, add(add(o, mul(E(7, i), bi)), g));
    h = mul_dd(h, zn);
    Fe t = add(gate, mul(sub(f, h), k.alpha));
    t = mul(t, k.zh_inv[i & 3]);
    // alpha^2 L1(x) (z - 1) / Z_H(x) = alpha^2 (z - 1) / (n (x - 1))
    t = add(t, mul(mul(sub(z, one_d()), ld(p.linv, i)), k.alpha2));
    st(p.t, i, t);
}

__global__ __launch_bounds__(256) void k_any_nonzero(const uint64_t* __restrict__ v, size_t words, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool nz = i < words && v[i] != 0;
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);   // one atomic per wave that saw anything
}

// ---- Horner scan: H_j = e_j + z H_{j-1} over a sequence in place (the synthetic division of a KZG opening) ----
// Three phases per level, runs of SCAN_RUN elements per lane: the runs' own Horner values, the same scan over those with
// z^SCAN_RUN, then every run again from its incoming value.  `rev`: the sequence is the array read backwards.
constexpr uint32_t SCAN_RUN = 64;
__global__ __launch_bounds__(64) void k_horner_local(const uint64_t* __restrict__ seq, size_t len, int rev, const uint64_t* __restrict__ zi,
                                                     uint64_t* __restrict__ runs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j0 = t * SCAN_RUN;
    if (j0 >= len) return;
    const size_t j1 = j0 + SCAN_RUN < len ? j0 + SCAN_RUN : len;
    const Fe z = ld(zi, 0);
    Fe h = f29::zero();
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) h = add(ld(seq, rev ? len - 1 - j : j), mul(h, z));
    st(runs, t, h);
}
// the incoming value of run t is the finished value of run t - 1 one level up; a short last run of the level above has
// already been multiplied by the right power there, because every run but the last is full
__global__ __launch_bounds__(64) void k_horner_final(uint64_t* __restrict__ seq, size_t len, int rev, const uint64_t* __restrict__ zi,
                                                     const uint64_t* __restrict__ runs_done) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j0 = t * SCAN_RUN;
    if (j0 >= len) return;
    const size_t j1 = j0 + SCAN_RUN < len ? j0 + SCAN_RUN : len;
    const Fe z = ld(zi, 0);
    Fe h = (t && runs_done) ? ld(runs_done, t - 1) : f29::zero();
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) {
        const size_t at = rev ? len - 1 - j : j;
        h = add(ld(seq, at), mul(h, z));
        st(seq, at, h);
    }
}
// z (D-form words) -> zpow[k] = z^(SCAN_RUN^k) in I-form, k < levels
__global__ void k_horner_powers(const uint64_t* __restrict__ z_d, uint64_t* __restrict__ zpow, uint32_t levels) {
    if (threadIdx.x || blockIdx.x) return;
    Fe z = x32(ld(z_d, 0));
    for (uint32_t k = 0; k < levels; k++) {
        st(zpow, k, z);
        for (uint32_t s = 1; s < SCAN_RUN; s <<= 1) z = mul(z, z);
    }
}

// ---- the permutation's grand product: z_0 = 1, z_{i+1} = z_i prod_j (w_j + beta id_j + gamma) / (w_j + beta sigma_j + gamma) ----
// k_gp_ratios: one lane per run of GP_RUN rows - the rows' ratios with ONE inversion per run (Montgomery's trick: the
// denominators' prefix products parked in the output), in I-form, written one place on (slot i + 1 = ratio_i, slot 0 = 1), so
// that an inclusive product scan leaves z in place; the last row's ratio goes to `last` (z_{n-1} ratio_{n-1} must be 1).
constexpr uint32_t GP_RUN = 64;
struct GrandProductParams {
    const uint64_t *l, *r, *o, *s1, *s2, *s3;
    const uint64_t* sc;   // device: beta, gamma, k1, k2 (D-form words)
    uint64_t* z;          // n elements
    uint64_t* last;       // 1 element: ratio_{n-1}, I-form
    uint32_t log_n;
};
__global__ __launch_bounds__(64) void k_gp_ratios(GrandProductParams p) {
    const size_t n = (size_t)1 << p.log_n;
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * GP_RUN;
    if (i0 >= n) return;
    const size_t i1 = i0 + GP_RUN < n ? i0 + GP_RUN : n;
    const Fe beta = ld(p.sc, 0), gamma = ld(p.sc, 1), beta_i = x32(beta);
    const Fe bk1 = mul(beta, x32(ld(p.sc, 2))), bk2 = mul(beta, x32(ld(p.sc, 3)));   // D x I -> D
    Fe w = root28_i();
    for (uint32_t k = p.log_n; k < 28; k++) w = mul(w, w);
    auto den_of = [&](size_t i) {   // I-form
        Fe d = mul_dd(add(add(ld(p.l, i), mul(ld(p.s1, i), beta_i)), gamma), add(add(ld(p.r, i), mul(ld(p.s2, i), beta_i)), gamma));
        return x32(mul_dd(d, add(add(ld(p.o, i), mul(ld(p.s3, i), beta_i)), gamma)));
    };
    // 1 / 0 := 0 (gnark's BatchInvert): a zero denominator stands as 1 in the run's product, so that the other rows' inverses
    // stay exact, and its own ratio is 0
    Fe acc = one_i();
#pragma unroll 1
    for (size_t i = i0; i < i1; i++) {
        const Fe d = den_of(i);
        acc = mul(acc, f29::is_zero_mod<RM>(d) ? one_i() : d);
        if (i + 1 < i1) st(p.z, i + 1, acc);   // prefix product up to row i, parked where row i's ratio will go
    }
    Fe inv = inv_i(acc);
    Fe x = pow_i(w, i1 - 1);                   // the run's last point, then downwards by w^-1 = w^(n-1)
    const Fe winv = pow_i(w, n - 1);
#pragma unroll 1
    for (size_t i = i1; i-- > i0;) {
        const Fe prev = i > i0 ? ld(p.z, i) : one_i();   // prefix product up to row i - 1
        const Fe d = den_of(i);
        const bool zero = f29::is_zero_mod<RM>(d);
        const Fe dinv = zero ? f29::zero() : mul(inv, prev);
        inv = mul(inv, zero ? one_i() : d);
        Fe num = mul_dd(add(add(ld(p.l, i), mul(beta, x)), gamma), add(add(ld(p.r, i), mul(bk1, x)), gamma));
        num = mul_dd(num, add(add(ld(p.o, i), mul(bk2, x)), gamma));
        const Fe ratio = mul(num, dinv);       // D x I -> D; the scan wants I-form
        if (i + 1 < n) st(p.z, i + 1, x32(ratio));
        else st(p.last, 0, x32(ratio));
        x = mul(x, winv);
    }
    if (i0 == 0) st(p.z, 0, one_i());
}
// inclusive product scan in place (I-form), runs of SCAN_RUN per lane; to_d: the finished values leave in D-form
__global__ __launch_bounds__(64) void k_mulscan_local(const uint64_t* __restrict__ seq, size_t len, uint64_t* __restrict__ runs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j0 = t * SCAN_RUN;
    if (j0 >= len) return;
    const size_t j1 = j0 + SCAN_RUN < len ? j0 + SCAN_RUN : len;
    Fe h = one_i();
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) h = mul(h, ld(seq, j));
    st(runs, t, h);
}
__global__ __launch_bounds__(64) void k_mulscan_final(uint64_t* __restrict__ seq, size_t len, const uint64_t* __restrict__ runs_done, int to_d) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j0 = t * SCAN_RUN;
    if (j0 >= len) return;
    const size_t j1 = j0 + SCAN_RUN < len ? j0 + SCAN_RUN : len;
    Fe h = (t && runs_done) ? ld(runs_done, t - 1) : one_i();
    const Fe c = one_d();   // the integer 2^256 mod r: I x plain -> D
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) {
        h = mul(h, ld(seq, j));
        st(seq, j, to_d ? mul(h, c) : h);
    }
}
// closes = (z_{n-1} ratio_{n-1} == 1): what a consistent permutation gives
__global__ void k_gp_closes(const uint64_t* __restrict__ z_d, size_t n, const uint64_t* __restrict__ last_i, uint32_t* __restrict__ flag) {
    if (threadIdx.x || blockIdx.x) return;
    const Fe v = f29::canonical<RM>(mul(ld(z_d, n - 1), ld(last_i, 0)));   // D x I -> D
    const Fe o = f29::canonical<RM>(one_d());
    uint32_t diff = 0;
    for (int i = 0; i < f29::NL; i++) diff |= v.v[i] ^ o.v[i];
    *flag = diff ? 1u : 0u;
}

// Groth16's quotient on the coset of the SAME size: h = (a b - c) / (x^n - 1), the divisor one constant there
__global__ __launch_bounds__(256) void k_g16_pointwise(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                                                       const uint64_t* __restrict__ zhinv_i, uint64_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st(out, i, mul(sub(mul_dd(ld(a, i), ld(b, i)), ld(c, i)), ld(zhinv_i, 0)));
}
__global__ void k_g16_const(const uint64_t* __restrict__ shift_d, uint32_t log_n, uint64_t* __restrict__ zhinv_i, uint32_t* bad) {
    if (threadIdx.x || blockIdx.x) return;
    const Fe den = sub(pow_i(x32(ld(shift_d, 0)), (uint64_t)1 << log_n), one_i());
    *bad = f29::is_zero_mod<RM>(den) ? 1u : 0u;   // the shift lies in H: x^n - 1 vanishes on the whole coset
    st(zhinv_i, 0, inv_i(den));
}

// out[i] = sum_t scalars[t] polys[t][i]: linearisation and batching polynomials of the last round
__global__ void k_to_iform(uint64_t* __restrict__ sc, uint32_t count) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) st(sc, t, x32(ld(sc, t)));
}
constexpr uint32_t LINCOMB_MAX_TERMS = 16;
struct LincombParams {
    const uint64_t* polys[LINCOMB_MAX_TERMS];
    const uint64_t* sc_i;   // device: the scalars, I-form
    uint64_t* out;
    size_t m;
    uint32_t n_terms;
};
__global__ __launch_bounds__(256) void k_lincomb(LincombParams p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.m) return;
    Fe acc = f29::zero();
    for (uint32_t t = 0; t < p.n_terms; t++) acc = add(acc, mul(ld(p.polys[t], i), ld(p.sc_i, t)));
    st(p.out, i, acc);
}

// ---- bn254_f29.hpp at given limbs (self-test entry nlx_bn254_f29_ops): one lane per case, every function on the case's
// operands, each result as nine limbs.  The operands are raw limbs, so the loose values the kernels above never meet through the
// public entries (those reduce first) can be passed. ----
constexpr uint32_t F29_OPS_WORDS = NLX_BN254_F29_OPS_WORDS;
static_assert(F29_OPS_WORDS == 11 * f29::NL, "output layout");
template <class M>
__global__ __launch_bounds__(64) void k_f29_ops(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n, uint32_t* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Fe x, y;
#pragma unroll
    for (int i = 0; i < f29::NL; i++) { x.v[i] = a[t * f29::NL + i]; y.v[i] = b[t * f29::NL + i]; }
    uint32_t w[8], c[8];
    f29::to_words256(x, w);
    f29::to_canonical256<M>(x, c);
    Fe zf = f29::zero();
    zf.v[0] = f29::is_zero_mod<M>(x) ? 1u : 0u;
    const Fe res[11] = {f29::mul<M>(x, y), f29::add(x, y), f29::sub<4, M>(x, y), f29::sub<8, M>(x, y), f29::tighten<M>(x), f29::canonical<M>(x), zf,
                        f29::from_mont256<M>(w), f29::from_words256(w), f29::from_words256(c), f29::x32<M>(x)};
    uint32_t* o = out + t * F29_OPS_WORDS;
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int i = 0; i < f29::NL; i++) o[k * f29::NL + i] = res[k].v[i];
    }
}

}  // namespace bnp
}  // namespace nlx

using namespace nlx;

namespace {
// H_j in place over seq (len elements, optionally read backwards); d_zpow: the powers z^(64^k), device, 4 words each
int32_t horner_scan(nlx_ctx* ctx, uint64_t* seq, size_t len, int rev, const uint64_t* d_zpow, uint32_t level, Scratch& scratch) {
    hipStream_t st = ctx->stream;
    const size_t runs = (len + bnp::SCAN_RUN - 1) / bnp::SCAN_RUN;
    if (runs <= 1) {
        hipLaunchKernelGGL(bnp::k_horner_final, dim3(1), dim3(64), 0, st, seq, len, rev, d_zpow + 4 * level, (const uint64_t*)nullptr);
        return NLX_OK;
    }
    uint64_t* d_runs = scratch.alloc_as<uint64_t>(runs * 32);
    if (!d_runs) return NLX_E_NOMEM;
    const unsigned blocks = (unsigned)((runs + 63) / 64);
    hipLaunchKernelGGL(bnp::k_horner_local, dim3(blocks), dim3(64), 0, st, seq, len, rev, d_zpow + 4 * level, d_runs);
    const int32_t rc = horner_scan(ctx, d_runs, runs, 0, d_zpow, level + 1, scratch);
    if (rc) return rc;
    hipLaunchKernelGGL(bnp::k_horner_final, dim3(blocks), dim3(64), 0, st, seq, len, rev, d_zpow + 4 * level, d_runs);
    return NLX_OK;
}

// inclusive product scan of seq (I-form) in place; to_d on the outermost level only
int32_t mul_scan(nlx_ctx* ctx, uint64_t* seq, size_t len, int to_d, Scratch& scratch) {
    hipStream_t st = ctx->stream;
    const size_t runs = (len + bnp::SCAN_RUN - 1) / bnp::SCAN_RUN;
    if (runs <= 1) {
        hipLaunchKernelGGL(bnp::k_mulscan_final, dim3(1), dim3(64), 0, st, seq, len, (const uint64_t*)nullptr, to_d);
        return NLX_OK;
    }
    uint64_t* d_runs = scratch.alloc_as<uint64_t>(runs * 32);
    if (!d_runs) return NLX_E_NOMEM;
    const unsigned blocks = (unsigned)((runs + 63) / 64);
    hipLaunchKernelGGL(bnp::k_mulscan_local, dim3(blocks), dim3(64), 0, st, seq, len, d_runs);
    const int32_t rc = mul_scan(ctx, d_runs, runs, 0, scratch);
    if (rc) return rc;
    hipLaunchKernelGGL(bnp::k_mulscan_final, dim3(blocks), dim3(64), 0, st, seq, len, d_runs, to_d);
    return NLX_OK;
}
}  // namespace

// ---- the quotient chain behind nlx_bn254_plonk_quotient and the resident prover (bn254_plonk_prove.hip) ----
namespace nlx {
namespace bnp {

// polys (values on H or coefficients, never coset values) -> their values on the coset shift * <w_4n>, [count][4n] in d_ev:
// FFTInverse(DIF) for the ones given by values, every coefficient to its bit-reversed place of 4n, FFT(DIT, OnCoset).
// blind: the per-proof group's first column in d_ev and the nine scalars on the device (values-on-H callers), or NULL.
static int32_t to_coset_blinded(nlx_ctx* ctx, uint32_t log_n, const PolyIn* polys, uint32_t count, const uint64_t shift[4], uint64_t* d_ev,
                                Scratch& scratch, uint32_t blind_first, const uint64_t* d_blind) {
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << log_n, N4 = 4 * n;
    uint32_t n_values = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (!polys[i].p) return ctx->fail(NLX_E_INVAL, "NULL polynomial");
        if (polys[i].kind == POLY_VALUES) n_values++;
        else if (polys[i].kind != POLY_COEFFS || polys[i].len > N4 || !is_device_ptr(polys[i].p)) return ctx->fail(NLX_E_INVAL, "coefficients are at most 4 n device elements");
    }
    uint64_t* d_in = n_values ? scratch.alloc_as<uint64_t>((size_t)n_values * n * 32) : nullptr;
    if (n_values && !d_in) return NLX_E_NOMEM;
    uint32_t v = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (polys[i].kind != POLY_VALUES) continue;
        hipError_t e = hipMemcpyAsync(d_in + (size_t)v++ * n * 4, polys[i].p, n * 32,
                                      is_device_ptr(polys[i].p) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync");
    }
    // 1. FFTInverse(DIF): values on H -> coefficients in bit-reversed order
    if (n_values) NLX_RC(nlx_bn254_ntt_batch_coset(ctx, d_in, n_values, log_n, 1, NLX_BN254_MONTGOMERY | NLX_BN254_BITREV_OUT, nullptr));
    // 2. zero-padded to 4n in bit-reversed order (coefficient at position p of n sits at 4 p of 4n), then FFT(DIT, OnCoset)
    hipError_t e = hipMemsetAsync(d_ev, 0, (size_t)count * N4 * 32, st);
    v = 0;
    for (uint32_t i = 0; i < count && e == hipSuccess; i++) {
        uint64_t* col = d_ev + (size_t)i * N4 * 4;
        if (polys[i].kind == POLY_VALUES) e = hipMemcpy2DAsync(col, 128, d_in + (size_t)v++ * n * 4, 32, 32, n, hipMemcpyDeviceToDevice, st);
        else if (polys[i].len) hipLaunchKernelGGL(k_plonk_place_coeffs, dim3((unsigned)((polys[i].len + 255) / 256)), dim3(256), 0, st, polys[i].p, polys[i].len, log_n, col);
    }
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpy2DAsync");
    if (d_blind) hipLaunchKernelGGL(k_plonk_blind, dim3(1), dim3(64), 0, st, d_ev + (size_t)blind_first * N4 * 4, d_blind, log_n);
    return nlx_bn254_ntt_batch_coset(ctx, d_ev, count, log_n + 2, 0, NLX_BN254_MONTGOMERY | NLX_BN254_BITREV_IN, shift);
}

int32_t to_coset(nlx_ctx* ctx, uint32_t log_n, const PolyIn* polys, uint32_t count, const uint64_t shift[4], uint64_t* d_ev) {
    Scratch scratch(ctx);
    return scratch.finish(to_coset_blinded(ctx, log_n, polys, count, shift, d_ev, scratch, 0, nullptr));
}

int32_t quotient_chain(nlx_ctx* ctx, const QuotientIn& q, uint64_t* t_out, size_t t_count, size_t t_keep, int32_t* high_chunk_is_zero) {
    for (const uint64_t* sc : q.scalars)
        if (!sc || is_device_ptr(sc)) return ctx->fail(NLX_E_INVAL, "the challenges and shifts are host values (four words each)");
    for (const uint64_t* sc : q.scalars)
        if (!bnf::below_mod<bnf::RP>(sc)) return ctx->fail(NLX_E_RANGE, "a challenge or shift is not below r (fr.Element words are residues)");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t log_n = q.log_n, K = q.n_commit, nF = 8 + K, nP = 4 + q.has_pi + K;
    const bool fixed_resident = q.fixed[0].kind == POLY_COSET;   // then all of the group: one block, used where it lies
    const uint32_t T = (fixed_resident ? 0 : nF) + nP;
    const bool blinded = q.blinding != nullptr, commit = K != 0;
    const size_t n = (size_t)1 << log_n, N4 = 4 * n;
    Scratch scratch(ctx);
    int32_t rc = NLX_OK;
    uint64_t* d_ev = scratch.alloc_as<uint64_t>((size_t)T * N4 * 32);
    uint64_t* d_x = scratch.alloc_as<uint64_t>(N4 * 32);
    uint64_t* d_linv = scratch.alloc_as<uint64_t>(N4 * 32);
    uint64_t* d_t = scratch.alloc_as<uint64_t>(N4 * 32);
    uint64_t* d_small = scratch.alloc_as<uint64_t>(6 * 32 + sizeof(Consts) + 64 + 9 * 32);
    if (!d_ev || !d_x || !d_linv || !d_t || !d_small) return NLX_E_NOMEM;
    Consts* d_k = (Consts*)(d_small + 6 * 4);
    uint32_t* d_flag = (uint32_t*)((char*)d_k + sizeof(Consts));
    uint64_t* d_blind = (uint64_t*)((char*)d_flag + 64);
    {
        uint64_t h[6 * 4];
        for (int i = 0; i < 6; i++) memcpy(h + 4 * i, q.scalars[i], 32);
        hipError_t e = hipMemcpyAsync(d_small, h, sizeof h, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && blinded) e = hipMemcpyAsync(d_blind, q.blinding, 9 * 32, hipMemcpyHostToDevice, st);   // caller-owned: outlives the sync below
        if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, 8, st);   // [0] high chunk non-zero, [1] Z_H vanishes on the coset
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // h leaves scope
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync");
    }
    hipLaunchKernelGGL(k_plonk_consts, dim3(1), dim3(1), 0, st, d_k, log_n, d_small, d_flag + 1);
    hipLaunchKernelGGL(k_plonk_domain, dim3((unsigned)(((N4 + DOMAIN_RUN - 1) / DOMAIN_RUN + 63) / 64)), dim3(64), 0, st, d_k, log_n, d_x, d_linv);
    PolyIn polys[13 + 2 * NLX_BN254_PLONK_MAX_COMMIT];
    uint32_t t = 0;
    if (!fixed_resident)
        for (uint32_t i = 0; i < nF; i++) polys[t++] = q.fixed[i];
    const uint32_t proof_first = t;
    for (uint32_t i = 0; i < nP; i++) polys[t++] = q.proof[i];
    rc = to_coset_blinded(ctx, log_n, polys, T, q.scalars[0], d_ev, scratch, proof_first, blinded ? d_blind : nullptr);
    if (rc) return rc;
    // 3. the quotient's values on the coset
    QuotientParams qp{fixed_resident ? q.fixed[0].p : d_ev, d_ev + (size_t)proof_first * N4 * 4, d_x, d_linv, d_k, d_t, log_n, q.has_pi, K};
    ctx->begin_kernel("plonk_quotient", 32.0 * N4 * (nF + nP + 4));
    if (commit) hipLaunchKernelGGL(k_plonk_quotient<true>, dim3((unsigned)((N4 + 255) / 256)), dim3(256), 0, st, qp);
    else hipLaunchKernelGGL(k_plonk_quotient<false>, dim3((unsigned)((N4 + 255) / 256)), dim3(256), 0, st, qp);
    ctx->end_kernel();
    // 4. back to coefficients
    rc = nlx_bn254_ntt_batch_coset(ctx, d_t, 1, log_n + 2, 1, NLX_BN254_MONTGOMERY, q.scalars[0]);
    if (rc) return rc;
    // coefficients that must vanish: t_keep .. 4 n - 1 (3 n without blinding; the blinded wires raise the quotient's degree by six)
    hipLaunchKernelGGL(k_any_nonzero, dim3((unsigned)(((N4 - t_keep) * 4 + 255) / 256)), dim3(256), 0, st, d_t + t_keep * 4, (N4 - t_keep) * 4, d_flag);
    uint32_t flags[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(flags, d_flag, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    if (flags[1]) return ctx->fail(NLX_E_INVAL, "coset shift lies in the evaluation subgroup (x^n - 1 vanishes on the coset)");
    e = hipMemcpyAsync(t_out, d_t, t_count * 32, is_device_ptr(t_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return ctx->hip_fail(le, "kernel launch");
    if (high_chunk_is_zero) *high_chunk_is_zero = flags[0] ? 0 : 1;
    return NLX_OK;
}

}  // namespace bnp
}  // namespace nlx

extern "C" {

int32_t nlx_bn254_f29_ops(nlx_ctx* ctx, uint32_t modulus, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!a || !b || !out) return ctx->fail(NLX_E_INVAL, "NULL buffer");
    if (modulus != NLX_BN254_MODULUS_Q && modulus != NLX_BN254_MODULUS_R) return ctx->fail(NLX_E_RANGE, "modulus is NLX_BN254_MODULUS_Q or NLX_BN254_MODULUS_R");
    if (n == 0) return NLX_OK;
    if (n > (size_t)1 << 24) return ctx->fail(NLX_E_RANGE, "n must be <= 2^24");
    (void)hipSetDevice(ctx->device);
    Staged sa(ctx, a, n * f29::NL * 4, true, false), sb(ctx, b, n * f29::NL * 4, true, false), so(ctx, out, n * bnp::F29_OPS_WORDS * 4, false, true);
    if (sa.status) return sa.status;
    if (sb.status) return sb.status;
    if (so.status) return so.status;
    const dim3 grid((unsigned)((n + 63) / 64));
    if (modulus == NLX_BN254_MODULUS_Q) hipLaunchKernelGGL(bnp::k_f29_ops<f29::QMod>, grid, dim3(64), 0, ctx->stream, sa.as<uint32_t>(), sb.as<uint32_t>(), n, so.as<uint32_t>());
    else hipLaunchKernelGGL(bnp::k_f29_ops<f29::RMod>, grid, dim3(64), 0, ctx->stream, sa.as<uint32_t>(), sb.as<uint32_t>(), n, so.as<uint32_t>());
    int32_t rc = so.finish();
    if (rc) return rc;
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_bn254_plonk_grand_product(nlx_ctx* ctx, uint32_t log_n, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                                      const uint64_t* s1, const uint64_t* s2, const uint64_t* s3, const uint64_t beta[4],
                                      const uint64_t gamma[4], const uint64_t k1[4], const uint64_t k2[4], uint64_t* z_out,
                                      int32_t* closes) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!l || !r || !o || !s1 || !s2 || !s3 || !beta || !gamma || !k1 || !k2 || !z_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_n < 1 || log_n > 28) return ctx->fail(NLX_E_RANGE, "log_n must be in [1, 28]");
    if (is_device_ptr(beta) || is_device_ptr(gamma) || is_device_ptr(k1) || is_device_ptr(k2)) return ctx->fail(NLX_E_INVAL, "the challenges and shifts are host values");
    for (const uint64_t* sc : {beta, gamma, k1, k2})
        if (!bnf::below_mod<bnf::RP>(sc)) return ctx->fail(NLX_E_RANGE, "a challenge or shift is not below r (fr.Element words are residues)");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << log_n;
    Scratch scratch(ctx);
    Staged sl(ctx, l, n * 32, true, false), sr(ctx, r, n * 32, true, false), so(ctx, o, n * 32, true, false);
    Staged ss1(ctx, s1, n * 32, true, false), ss2(ctx, s2, n * 32, true, false), ss3(ctx, s3, n * 32, true, false);
    Staged sz(ctx, z_out, n * 32, false, true);
    for (const Staged* s : {&sl, &sr, &so, &ss1, &ss2, &ss3, &sz})
        if (s->status) return s->status;
    uint64_t* d_z = sz.as<uint64_t>();
    uint64_t* d_small = scratch.alloc_as<uint64_t>(4 * 32 + 32 + 64);
    if (!d_small) return NLX_E_NOMEM;
    uint64_t h[16];
    memcpy(h, beta, 32); memcpy(h + 4, gamma, 32); memcpy(h + 8, k1, 32); memcpy(h + 12, k2, 32);
    hipError_t e = hipMemcpyAsync(d_small, h, sizeof h, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // h leaves scope
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync");
    uint32_t* d_flag = (uint32_t*)(d_small + 20);
    bnp::GrandProductParams gp{sl.as<uint64_t>(), sr.as<uint64_t>(), so.as<uint64_t>(), ss1.as<uint64_t>(), ss2.as<uint64_t>(), ss3.as<uint64_t>(),
                               d_small, d_z, d_small + 16, log_n};
    hipLaunchKernelGGL(bnp::k_gp_ratios, dim3((unsigned)(((n + bnp::GP_RUN - 1) / bnp::GP_RUN + 63) / 64)), dim3(64), 0, st, gp);
    int32_t rc = mul_scan(ctx, d_z, n, 1, scratch);
    if (rc) return rc;
    hipLaunchKernelGGL(bnp::k_gp_closes, dim3(1), dim3(1), 0, st, d_z, n, d_small + 16, d_flag);
    uint32_t flag = 0;
    e = hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && sz.finish()) return sz.status;
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // flag is a local
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return ctx->hip_fail(le, "kernel launch");
    if (closes) *closes = flag ? 0 : 1;
    return NLX_OK;
} NLX_CATCH(ctx)

// Host scalars come as fr.Element words (Montgomery residues): bnf::below_mod<RP> refuses anything that is not one - the
// 29-bit-limb arithmetic's bounds would not hold for it.
int32_t nlx_bn254_groth16_quotient(nlx_ctx* ctx, uint32_t log_n, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                                   const uint64_t coset_shift[4], uint64_t* h_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!a || !b || !c || !coset_shift || !h_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_n < 1 || log_n > 28) return ctx->fail(NLX_E_RANGE, "log_n must be in [1, 28]");
    if (is_device_ptr(coset_shift)) return ctx->fail(NLX_E_INVAL, "the coset shift is a host value");
    if (!bnf::below_mod<bnf::RP>(coset_shift)) return ctx->fail(NLX_E_RANGE, "the coset shift is not below r");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << log_n;
    Scratch scratch(ctx);
    uint64_t* d_abc = scratch.alloc_as<uint64_t>(3 * n * 32);   // the call's own copy: a, b, c are transformed in place, the caller's are not
    uint64_t* d_small = scratch.alloc_as<uint64_t>(96);         // shift | 1 / (shift^n - 1) | flag
    if (!d_abc || !d_small) return NLX_E_NOMEM;
    const uint64_t* in[3] = {a, b, c};
    for (int i = 0; i < 3; i++) {
        hipError_t e = hipMemcpyAsync(d_abc + (size_t)i * n * 4, in[i], n * 32, is_device_ptr(in[i]) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync");
    }
    hipError_t e = hipMemcpy(d_small, coset_shift, 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpy");
    hipLaunchKernelGGL(bnp::k_g16_const, dim3(1), dim3(1), 0, st, d_small, log_n, d_small + 4, (uint32_t*)(d_small + 8));
    {
        uint32_t bad = 0;
        e = hipMemcpyAsync(&bad, d_small + 8, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync");
        if (bad) return ctx->fail(NLX_E_INVAL, "coset shift lies in the evaluation subgroup (x^n - 1 vanishes on the coset)");
    }
    // FFTInverse(DIF) -> FFT(DIT, OnCoset): no reordering pass; then a b - c over the coset's constant x^n - 1
    int32_t rc = nlx_bn254_ntt_batch_coset(ctx, d_abc, 3, log_n, 1, NLX_BN254_MONTGOMERY | NLX_BN254_BITREV_OUT, nullptr);
    if (!rc) rc = nlx_bn254_ntt_batch_coset(ctx, d_abc, 3, log_n, 0, NLX_BN254_MONTGOMERY | NLX_BN254_BITREV_IN, coset_shift);
    if (rc) return rc;
    hipLaunchKernelGGL(bnp::k_g16_pointwise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_abc, d_abc + n * 4, d_abc + 2 * n * 4,
                       d_small + 4, d_abc, n);
    rc = nlx_bn254_ntt_batch_coset(ctx, d_abc, 1, log_n, 1, NLX_BN254_MONTGOMERY, coset_shift);
    if (rc) return rc;
    e = hipMemcpyAsync(h_out, d_abc, n * 32, is_device_ptr(h_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return ctx->hip_fail(le, "kernel launch");
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_bn254_fr_lincomb(nlx_ctx* ctx, uint64_t m, uint32_t n_terms, const uint64_t* const* polys, const uint64_t* scalars,
                             uint64_t* out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!polys || !scalars || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (n_terms < 1 || n_terms > bnp::LINCOMB_MAX_TERMS || m < 1 || m > ((uint64_t)1 << 28)) return ctx->fail(NLX_E_RANGE, "1 .. 16 terms of 1 .. 2^28 elements");
    if (is_device_ptr(polys) || is_device_ptr(scalars)) return ctx->fail(NLX_E_INVAL, "the pointer array and the scalars are host arrays");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    Scratch scratch(ctx);
    bnp::LincombParams lp{};
    std::deque<Staged> sp;   // the polynomials are read in place
    for (uint32_t t = 0; t < n_terms; t++) {
        if (!polys[t]) return ctx->fail(NLX_E_INVAL, "NULL polynomial");
        sp.emplace_back(ctx, polys[t], m * 32, true, false);
        if (sp[t].status) return sp[t].status;
        lp.polys[t] = sp[t].as<uint64_t>();
    }
    Staged sout(ctx, out, m * 32, false, true);
    if (sout.status) return sout.status;
    uint64_t* d_sc = scratch.alloc_as<uint64_t>((size_t)n_terms * 32);
    if (!d_sc) return NLX_E_NOMEM;
    hipError_t e = hipMemcpy(d_sc, scalars, (size_t)n_terms * 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpy");
    hipLaunchKernelGGL(bnp::k_to_iform, dim3(1), dim3(64), 0, st, d_sc, n_terms);
    lp.sc_i = d_sc; lp.out = sout.as<uint64_t>(); lp.m = m; lp.n_terms = n_terms;
    hipLaunchKernelGGL(bnp::k_lincomb, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, lp);
    if (sout.finish()) return sout.status;
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return ctx->hip_fail(le, "kernel launch");
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_bn254_plonk_quotient(nlx_ctx* ctx, const nlx_bn254_plonk_quotient_args* a, uint64_t* t_out, int32_t* high_chunk_is_zero) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!a || !t_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    const uint64_t* polys[13] = {a->ql, a->qr, a->qm, a->qo, a->qk, a->s1, a->s2, a->s3, a->l, a->r, a->o, a->z, a->pi};
    for (int i = 0; i < 12; i++)
        if (!polys[i]) return ctx->fail(NLX_E_INVAL, "NULL polynomial");
    if (a->log_n < 2 || a->log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n must be in [2, 26] (the coset has four times the points)");
    const bool blinded = (a->flags & NLX_BN254_PLONK_BLINDED) != 0, commit = (a->flags & NLX_BN254_PLONK_COMMIT) != 0;
    if ((a->flags & ~(NLX_BN254_PLONK_BLINDED | NLX_BN254_PLONK_COMMIT)) != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_UNSUPPORTED, "elements must be fr.Element words (flags = NLX_BN254_MONTGOMERY)");
    if (blinded) {
        if (!a->blinding || is_device_ptr(a->blinding)) return ctx->fail(NLX_E_INVAL, "the blinding scalars are host values (nine elements of four words)");
        if (a->log_n < 3) return ctx->fail(NLX_E_RANGE, "a blinded quotient needs log_n >= 3 (3 n + 6 coefficients on 4 n points)");
        for (int i = 0; i < 9; i++)
            if (!bnf::below_mod<bnf::RP>(a->blinding + 4 * i)) return ctx->fail(NLX_E_RANGE, "a blinding scalar is not below r");
    }
    // n_commit, qcp, pi2 lie behind the struct a caller of the earlier ABI allocated: read only under the flag
    const uint32_t K = commit ? a->n_commit : 0;
    if (commit) {
        if (K < 1 || K > NLX_BN254_PLONK_MAX_COMMIT) return ctx->fail(NLX_E_RANGE, "n_commit must be in [1, 4]");
        if (!a->qcp || !a->pi2 || is_device_ptr(a->qcp) || is_device_ptr(a->pi2)) return ctx->fail(NLX_E_INVAL, "qcp and pi2 are host arrays of n_commit pointers");
        for (uint32_t j = 0; j < K; j++)
            if (!a->qcp[j] || !a->pi2[j]) return ctx->fail(NLX_E_INVAL, "NULL polynomial (qcp / pi2)");
    }
    const size_t n = (size_t)1 << a->log_n;
    bnp::PolyIn fixed[8 + NLX_BN254_PLONK_MAX_COMMIT], proof[5 + NLX_BN254_PLONK_MAX_COMMIT];
    uint32_t np = 0;
    for (int i = 0; i < 8; i++) fixed[i] = bnp::PolyIn{polys[i], bnp::POLY_VALUES, n};
    for (uint32_t j = 0; j < K; j++) fixed[8 + j] = bnp::PolyIn{a->qcp[j], bnp::POLY_VALUES, n};
    for (int i = 8; i < 12; i++) proof[np++] = bnp::PolyIn{polys[i], bnp::POLY_VALUES, n};
    if (a->pi) proof[np++] = bnp::PolyIn{a->pi, bnp::POLY_VALUES, n};
    for (uint32_t j = 0; j < K; j++) proof[np++] = bnp::PolyIn{a->pi2[j], bnp::POLY_VALUES, n};
    bnp::QuotientIn in{a->log_n, a->pi ? 1u : 0u, K, fixed, proof, {a->coset_shift, a->k1, a->k2, a->alpha, a->beta, a->gamma}, blinded ? a->blinding : nullptr};
    return bnp::quotient_chain(ctx, in, t_out, blinded ? 4 * n : 3 * n, blinded ? 3 * n + 6 : 3 * n, high_chunk_is_zero);
} NLX_CATCH(ctx)

int32_t nlx_bn254_kzg_open(nlx_ctx* ctx, const uint64_t* coeffs, uint64_t m, const uint64_t zeta[4], const uint64_t* srs,
                           uint64_t y_out[4], uint64_t* quotient_out, uint64_t proof_out[8]) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!coeffs || !zeta || !y_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (m < 2 || m > ((uint64_t)1 << 28)) return ctx->fail(NLX_E_RANGE, "2 <= coefficients <= 2^28");
    if (proof_out && !srs) return ctx->fail(NLX_E_INVAL, "an opening proof needs the SRS");
    if (is_device_ptr(zeta) || is_device_ptr(y_out)) return ctx->fail(NLX_E_INVAL, "the point and the value are host words");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    Scratch scratch(ctx);
    uint64_t* d_h = scratch.alloc_as<uint64_t>(m * 32);   // the call's own copy: the scan runs in place, the caller's coefficients stay
    uint64_t* d_z = scratch.alloc_as<uint64_t>(32 + 8 * 32);
    if (!d_h || !d_z) return NLX_E_NOMEM;
    hipError_t e = hipMemcpyAsync(d_h, coeffs, m * 32, is_device_ptr(coeffs) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpy(d_z, zeta, 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpy");
    uint32_t levels = 1;
    for (uint64_t len = m; len > bnp::SCAN_RUN; len = (len + bnp::SCAN_RUN - 1) / bnp::SCAN_RUN) levels++;
    hipLaunchKernelGGL(bnp::k_horner_powers, dim3(1), dim3(1), 0, st, d_z, d_z + 4, levels);
    // H_j = p_{m-1-j} + zeta H_{j-1}: the array read from the top coefficient down; afterwards position i holds h_i with
    // h_0 = p(zeta) and q_{i-1} = h_i: the quotient is the array shifted down by one
    int32_t rc = horner_scan(ctx, d_h, m, 1, d_z + 4, 0, scratch);
    if (rc) return rc;
    e = hipMemcpyAsync(y_out, d_h, 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && quotient_out)
        e = hipMemcpyAsync(quotient_out, d_h + 4, (m - 1) * 32, is_device_ptr(quotient_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "copy out");
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return ctx->hip_fail(le, "kernel launch");
    if (proof_out) {
        rc = nlx_bn254_msm_g1(ctx, srs, d_h + 4, m - 1, NLX_BN254_MONTGOMERY, proof_out);
        if (rc) return rc;
    }
    return NLX_OK;
} NLX_CATCH(ctx)

}  // extern "C"
