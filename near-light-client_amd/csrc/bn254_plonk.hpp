// The PLONK quotient chain (bn254_plonk.hip) as the resident prover (bn254_plonk_prove.hip) schedules it: the transform stage
// takes every polynomial in the form its owner already has.
#pragma once
#include <cstddef>
#include <cstdint>
#include "ctx.hpp"

namespace nlx {
namespace bnp {

enum PolyKind : uint32_t {
    POLY_VALUES = 0,   // n values on H, natural order, host or device: FFTInverse(DIF), then FFT(DIT, OnCoset)
    POLY_COEFFS = 1,   // len <= 4 n coefficients, natural order, device: FFT(DIT, OnCoset) only
    POLY_COSET = 2,    // 4 n values on the coset, natural order, device: read where they lie
};
struct PolyIn {
    const uint64_t* p;
    uint32_t kind;
    size_t len;   // POLY_COEFFS: the number of coefficients
};
struct QuotientIn {
    uint32_t log_n, has_pi, n_commit;
    const PolyIn* fixed;   // 8 + n_commit: ql qr qm qo qk s1 s2 s3 (qcp_0 ..); POLY_COSET: all of them, one block [8 + n_commit][4 n] at fixed[0].p
    const PolyIn* proof;   // 4 + has_pi + n_commit: l r o z (pi) (pi2_0 ..); never POLY_COSET
    const uint64_t* scalars[6];   // host: coset_shift k1 k2 alpha beta gamma
    const uint64_t* blinding;     // host, nine elements: patched into l r o z (callers that give them by values on H), or NULL
};
// t_out (host or device) receives the first t_count coefficients of the quotient; *high_chunk_is_zero (may be NULL): whether the
// coefficients from t_keep up vanish
int32_t quotient_chain(nlx_ctx* ctx, const QuotientIn& q, uint64_t* t_out, size_t t_count, size_t t_keep, int32_t* high_chunk_is_zero);
// the transform stage alone: count polynomials (POLY_VALUES / POLY_COEFFS) -> d_ev [count][4 n] on the coset shift * <w_4n>
int32_t to_coset(nlx_ctx* ctx, uint32_t log_n, const PolyIn* polys, uint32_t count, const uint64_t shift[4], uint64_t* d_ev);

}  // namespace bnp
}  // namespace nlx
