// The BN254 pairing on the device and its first user, the Groth16 verifier.  The
// arithmetic is bn254_pairing.hpp (host and device source, checked on the host against the big-integer model); this file holds
// the kernels, the entry points and the verifier's host half.
//
//   k_bn254_pairing_points   one lane per point pair: coordinates below q, on the curve, G2 in the subgroup -> a status word
//   k_bn254_miller           one lane per (check, pair): the pair's Miller value, an Fq12 in the kernels' form
//   k_bn254_final_exp        one lane per check: the product of its Miller values, the final exponentiation, the comparison
//                            with 1 or with the key's e(alpha, beta) -> a result word (and the GT element where asked for)
//   k_bn254_g16_ksum         one lane per (proof, term): scalar times point by double-and-add with bn254_curve29.hpp's group
//                            law; k_bn254_g16_ksum_reduce adds a proof's terms up and writes the affine sum where the Miller
//                            kernel reads it
// Every status / result word is preset to a value no kernel writes (WORD_UNSET); the host answers NLX_E_HIP for such a word and
// never reads it as a pass.  A lane is one long dependent chain over values that rest in scratch between the out-of-line tower
// functions (profiles/bn254_pairing_resource_usage.txt): blocks are one wave wide, so a batch spreads over the compute units.
#include <cstring>
#include <string>
#include <vector>
#include "bn254_curve29.hpp"
#include "bn254_msm.hpp"
#include "bn254_gnark_bytes.hpp"
#include "bn254_pairing.hpp"
#include "bn254_pairing_launch.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

using namespace nlx;
using namespace nlx::pairing;

namespace {

// stride: words between one point and the next (the verifier tests only the first pair of each proof)
__global__ __launch_bounds__(64) void k_bn254_pairing_points(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2, uint32_t n,
                                                             uint32_t g1_stride, uint32_t g2_stride, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t st = g1 ? check_g1(g1 + (size_t)g1_stride * i) : (uint32_t)POINT_OK;
    if (st == POINT_OK && g2) st = check_g2(g2 + (size_t)g2_stride * i);
    status[i] = st;
}

__global__ __launch_bounds__(64) void k_bn254_miller(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2, uint32_t n,
                                                     Fe12* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = miller_loop(g1_load(g1 + 8 * (size_t)i), g2_load(g2 + 16 * (size_t)i));
}

// first: n_checks + 1 offsets into the Miller values (NULL: check i is pair i); checks below n_expected are compared with
// `expected` (48 Montgomery words), the others with 1
__global__ __launch_bounds__(64) void k_bn254_final_exp(const Fe12* __restrict__ miller, const uint32_t* __restrict__ first, uint32_t n_checks,
                                                        uint32_t n_expected, const uint64_t* __restrict__ expected, int montgomery,
                                                        uint64_t* __restrict__ gt_out, uint32_t* __restrict__ result) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_checks) return;
    const uint32_t lo = first ? first[i] : i, hi = first ? first[i + 1] : i + 1;
    Fe12 f = f12_one();
    for (uint32_t k = lo; k < hi; k++) f = f12_mul(f, miller[k]);
    f = final_exponentiation(f);
    if (gt_out) f12_store(f, montgomery != 0, gt_out + 48 * (size_t)i);
    const Fe12 want = i < n_expected ? f12_load(expected) : f12_one();
    result[i] = f12_eq(f, want) ? 1u : 0u;
}

// term t: scalars[t] (a canonical integer below r) times a point - ic[src] for src < 2^31, extra[src - 2^31] otherwise
constexpr uint32_t SRC_EXTRA = 0x80000000u;
__global__ __launch_bounds__(64) void k_bn254_g16_ksum(const uint64_t* __restrict__ ic, const uint64_t* __restrict__ extra,
                                                       const uint32_t* __restrict__ src, const uint64_t* __restrict__ scalars, uint32_t n_terms,
                                                       msm::Jac29* __restrict__ out) {
    using namespace nlx::msm;
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_terms) return;
    const uint32_t s = src[t];
    const uint64_t* w = (s & SRC_EXTRA) ? extra + 8 * (size_t)(s & ~SRC_EXTRA) : ic + 8 * (size_t)s;
    const G1Point p = g1_load(w);
    Jac29 acc = inf29<F1>();
    if (!p.inf) {
        const Aff29 a{p.x, p.y};
        for (int bit = 253; bit >= 0; bit--) {
            acc = jdbl29(acc);
            if ((scalars[4 * (size_t)t + (bit >> 6)] >> (bit & 63)) & 1) acc = jmadd29(acc, a);
        }
    }
    out[t] = acc;
}
// segment s: the sum of terms [first[s], first[s + 1]) as G1Affine words at g1_pairs[dst[s]]
__global__ __launch_bounds__(64) void k_bn254_g16_ksum_reduce(const msm::Jac29* __restrict__ terms, const uint32_t* __restrict__ first,
                                                              const uint32_t* __restrict__ dst, uint32_t n_segments, uint64_t* __restrict__ g1_pairs) {
    using namespace nlx::msm;
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_segments) return;
    Jac29 acc = inf29<F1>();
    for (uint32_t k = first[s]; k < first[s + 1]; k++) acc = jadd29(acc, terms[k]);
    uint64_t* w = g1_pairs + 8 * (size_t)dst[s];
    if (F1::is_zero_exact(acc.z) || F1::is_zero_mod(acc.z)) {
        for (int i = 0; i < 8; i++) w[i] = 0;
        return;
    }
    const Fe zi = fq_inv(F1::tighten(acc.z)), zi2 = F1::sqr(zi);
    fq_store(F1::mul(acc.x, zi2), true, w);
    fq_store(F1::mul(acc.y, F1::mul(zi2, zi)), true, w + 4);
}

inline unsigned blocks64(size_t n) { return (unsigned)((n + 63) / 64); }

const char* status_text(uint32_t st) {
    switch (st) {
        case G1_RANGE: return "the G1 point has a coordinate that is not below q";
        case G1_OFF_CURVE: return "the G1 point is not on the curve";
        case G2_RANGE: return "the G2 point has a coordinate that is not below q";
        case G2_OFF_CURVE: return "the G2 point is not on the twist";
        case G2_NOT_IN_SUBGROUP: return "the G2 point is not in the subgroup of order r";
        default: return "unknown status";
    }
}

}  // namespace

// declared in bn254_pairing_launch.hpp: the PLONK verifier (bn254_plonk_verify.hip) enqueues the same checks
namespace nlx {
namespace pairing {

// The entry checks of n pairs (either side may be NULL): enqueues, reads the status words back, answers NLX_E_RANGE naming the
// first offending pair.  `what`: how the message calls a pair.
int32_t check_points(nlx_ctx* ctx, Scratch& scratch, const uint64_t* d_g1, const uint64_t* d_g2, size_t n, const char* what) {
    if (!n) return NLX_OK;
    uint32_t* d_status = scratch.alloc_as<uint32_t>(n * 4);
    if (!d_status) return ctx->fail(NLX_E_NOMEM, "pairing: device memory for %zu status words", n);
    NLX_HIP(ctx, hipMemsetAsync(d_status, 0xFF, n * 4, ctx->stream));
    ctx->begin_kernel("bn254_pairing_points", 192.0 * (double)n, (double)n);
    hipLaunchKernelGGL(k_bn254_pairing_points, dim3(blocks64(n)), dim3(64), 0, ctx->stream, d_g1, d_g2, (uint32_t)n, 8u, 16u, d_status);
    ctx->end_kernel();
    std::vector<uint32_t> status(n);
    NLX_RC(fetch(ctx, status.data(), d_status, n * 4));
    for (size_t i = 0; i < n; i++) {
        if (status[i] == WORD_UNSET) return ctx->fail(NLX_E_HIP, "pairing: the point check wrote no status for %s %zu", what, i);
        if (status[i] != POINT_OK) return ctx->fail(NLX_E_RANGE, "%s %zu: %s", what, i, status_text(status[i]));
    }
    return NLX_OK;
}

// Miller loops of n_pairs pairs and the final exponentiations of n_checks checks: enqueues only.  d_result: n_checks words,
// preset here.
int32_t enqueue_checks(nlx_ctx* ctx, Scratch& scratch, const uint64_t* d_g1, const uint64_t* d_g2, size_t n_pairs, const uint32_t* d_first,
                       size_t n_checks, size_t n_expected, const uint64_t* d_expected, int montgomery, uint64_t* d_gt, uint32_t* d_result) {
    NLX_HIP(ctx, hipMemsetAsync(d_result, 0xFF, n_checks * 4, ctx->stream));
    Fe12* d_miller = scratch.alloc_as<Fe12>((n_pairs ? n_pairs : 1) * sizeof(Fe12));
    if (!d_miller) return ctx->fail(NLX_E_NOMEM, "pairing: device memory for %zu Miller values", n_pairs);
    if (n_pairs) {
        ctx->begin_kernel("bn254_pairing_miller", (192.0 + sizeof(Fe12)) * (double)n_pairs, (double)n_pairs);
        hipLaunchKernelGGL(k_bn254_miller, dim3(blocks64(n_pairs)), dim3(64), 0, ctx->stream, d_g1, d_g2, (uint32_t)n_pairs, d_miller);
        ctx->end_kernel();
    }
    ctx->begin_kernel("bn254_pairing_final_exp", sizeof(Fe12) * (double)n_pairs + 4.0 * (double)n_checks, (double)n_checks);
    hipLaunchKernelGGL(k_bn254_final_exp, dim3(blocks64(n_checks)), dim3(64), 0, ctx->stream, (const Fe12*)d_miller, d_first, (uint32_t)n_checks,
                       (uint32_t)n_expected, d_expected, montgomery, d_gt, d_result);
    ctx->end_kernel();
    return NLX_OK;
}

int32_t read_results(nlx_ctx* ctx, const uint32_t* d_result, size_t n, std::vector<uint32_t>& out, Scratch* last) {
    out.resize(n);
    NLX_RC(fetch(ctx, out.data(), d_result, n * 4, last));
    for (size_t i = 0; i < n; i++)
        if (out[i] > 1) return ctx->fail(NLX_E_HIP, "pairing: the final exponentiation wrote no result for check %zu", i);
    return NLX_OK;
}

}  // namespace pairing
}  // namespace nlx

namespace {

int32_t pairing_body(nlx_ctx* ctx, Scratch& scratch, const uint64_t* g1, const uint64_t* g2, size_t n, uint32_t flags, uint64_t* gt_out) {
    Staged s1(ctx, g1, n * 64, true, false), s2(ctx, g2, n * 128, true, false);
    if (s1.status) return s1.status;
    if (s2.status) return s2.status;
    NLX_RC(check_points(ctx, scratch, s1.as<uint64_t>(), s2.as<uint64_t>(), n, "pair"));
    Staged so(ctx, gt_out, n * 48 * 8, false, true);
    if (so.status) return so.status;
    uint32_t* d_result = scratch.alloc_as<uint32_t>(n * 4);
    if (!d_result) return ctx->fail(NLX_E_NOMEM, "pairing: device memory");
    NLX_RC(enqueue_checks(ctx, scratch, s1.as<uint64_t>(), s2.as<uint64_t>(), n, nullptr, n, 0, nullptr, (flags & NLX_BN254_MONTGOMERY) ? 1 : 0,
                          so.as<uint64_t>(), d_result));
    // the result words first: nothing goes to the caller's buffer unless every lane vouched for its value
    std::vector<uint32_t> res;
    NLX_RC(read_results(ctx, d_result, n, res, nullptr));
    NLX_RC(so.finish());
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the copy-out is done before `so` gives its block back
    return NLX_OK;
}

int32_t pairing_check_body(nlx_ctx* ctx, Scratch& scratch, const uint64_t* g1, const uint64_t* g2, const uint32_t* n_pairs, size_t n_checks,
                           uint8_t* ok_out) {
    std::vector<uint32_t> first(n_checks + 1, 0);
    size_t total = 0;
    for (size_t c = 0; c < n_checks; c++) {
        total += n_pairs[c];
        if (total > MAX_PAIRS) return ctx->fail(NLX_E_RANGE, "at most 2^20 pairs per call");
        first[c + 1] = (uint32_t)total;
    }
    Staged s1(ctx, g1, (total ? total : 1) * 64, total != 0, false), s2(ctx, g2, (total ? total : 1) * 128, total != 0, false);
    if (total && s1.status) return s1.status;
    if (total && s2.status) return s2.status;
    NLX_RC(check_points(ctx, scratch, s1.as<uint64_t>(), s2.as<uint64_t>(), total, "pair"));
    uint32_t* d_first = scratch.alloc_as<uint32_t>(first.size() * 4);
    uint32_t* d_result = scratch.alloc_as<uint32_t>(n_checks * 4);
    if (!d_first || !d_result) return ctx->fail(NLX_E_NOMEM, "pairing: device memory");
    NLX_HIP(ctx, hipMemcpyAsync(d_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    NLX_RC(enqueue_checks(ctx, scratch, s1.as<uint64_t>(), s2.as<uint64_t>(), total, d_first, n_checks, 0, nullptr, 0, nullptr, d_result));
    std::vector<uint32_t> res;
    NLX_RC(read_results(ctx, d_result, n_checks, res, nullptr));   // synchronises: `first` has been read by then
    for (size_t c = 0; c < n_checks; c++) ok_out[c] = (uint8_t)res[c];
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_pairing(nlx_ctx* ctx, const uint64_t* g1, const uint64_t* g2, size_t n, uint32_t flags, uint64_t* gt_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n && (!g1 || !g2 || !gt_out)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (flags & ~(uint32_t)NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "unknown flag");
    if (n > MAX_PAIRS) return ctx->fail(NLX_E_RANGE, "at most 2^20 pairs per call");
    if (!n) return NLX_OK;
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    return scratch.finish(pairing_body(ctx, scratch, g1, g2, n, flags, gt_out));
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_pairing_check(nlx_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint32_t* n_pairs, size_t n_checks,
                                           uint32_t flags, uint8_t* ok_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n_checks && (!n_pairs || !ok_out)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (flags) return ctx->fail(NLX_E_RANGE, "unknown flag");
    if (n_checks > MAX_PAIRS) return ctx->fail(NLX_E_RANGE, "at most 2^20 checks per call");
    if (is_device_ptr(n_pairs) || is_device_ptr(ok_out)) return ctx->fail(NLX_E_INVAL, "n_pairs and ok_out are host arrays");
    size_t total = 0;
    for (size_t c = 0; c < n_checks; c++) total += n_pairs[c];
    if (total && (!g1 || !g2)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (!n_checks) return NLX_OK;
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    return scratch.finish(pairing_check_body(ctx, scratch, g1, g2, n_pairs, n_checks, ok_out));
} NLX_CATCH(ctx)

// ==== Groth16 ====
struct nlx_bn254_groth16_vk {
    nlx_ctx* ctx = nullptr;
    uint32_t n_public = 0, k = 0;
    std::vector<std::vector<uint32_t>> hashed;   // per commitment: ids into ic's index space
    uint64_t neg_gamma[16], neg_delta[16], ped_g[16], ped_grs[16];
    uint64_t* d_ic = nullptr;    // (n_public + k) x 8 words
    uint64_t* d_eab = nullptr;   // e(alpha, beta): 48 Montgomery words
    std::vector<void*> blocks;
};

namespace {

using bnf::QP;
using bnf::RP;
typedef bnf::Fp<QP> Fq;
typedef bnf::Fp<RP> Fr;
typedef msm::H2 H2;
using ppr::fq_from_be;
using ppr::fq_sqrt;
using ppr::fr_to_be;
using ppr::g1_decode;
using ppr::g1_marshal;
using ppr::lex_largest;
using ppr::rest_zero;

void vk_free(nlx_bn254_groth16_vk* vk) {
    if (!vk) return;
    if (vk->ctx) {
        (void)hipStreamSynchronize(vk->ctx->stream);
        for (void* p : vk->blocks) vk->ctx->release(p);
    }
    delete vk;
}

// a square root in Fq2 by the complex method: the norm's root, then two roots in Fq
bool f2_sqrt_host(const H2::T& a, H2::T& out) {
    Fq y;
    if (bnf::is_zero(a.c1)) {
        if (fq_sqrt(a.c0, y)) {
            out = H2::T{y, bnf::zero<QP>()};
            return true;
        }
        if (!fq_sqrt(bnf::neg(a.c0), y)) return false;   // -1 is no square: exactly one of a0, -a0 is
        out = H2::T{bnf::zero<QP>(), y};
        return true;
    }
    Fq s;
    if (!fq_sqrt(bnf::add(bnf::sqr(a.c0), bnf::sqr(a.c1)), s)) return false;
    const Fq half = bnf::inv_host(bnf::add(bnf::one<QP>(), bnf::one<QP>()));
    Fq x0;
    if (!fq_sqrt(bnf::mul(bnf::add(a.c0, s), half), x0) && !fq_sqrt(bnf::mul(bnf::sub(a.c0, s), half), x0)) return false;
    if (bnf::is_zero(x0)) return false;
    out = H2::T{x0, bnf::mul(a.c1, bnf::inv_host(bnf::add(x0, x0)))};
    const H2::T sq = H2::mul(out, out);
    return bnf::equal(sq.c0, a.c0) && bnf::equal(sq.c1, a.c1);
}
// G2Affine.SetBytes on 64 bytes: X.A1 || X.A0
bool g2_decode(const uint8_t* b, uint64_t w[16]) {
    memset(w, 0, 128);
    const unsigned flag = b[0] >> 6;
    if (flag == 1) return b[0] == 0x40 && rest_zero(b, 64);
    if (flag == 0) return false;
    H2::T x, y;
    if (!fq_from_be(b, true, x.c1) || !fq_from_be(b + 32, false, x.c0)) return false;
    const Fq one = bnf::one<QP>(), three = bnf::add(one, bnf::add(one, one));
    Fq nine = bnf::add(three, bnf::add(three, three));
    const H2::T b2 = H2::mul(H2::T{three, bnf::zero<QP>()}, H2::inv(H2::T{nine, one}));   // 3 / (9 + u)
    if (!f2_sqrt_host(H2::add(H2::mul(H2::mul(x, x), x), b2), y)) return false;
    const bool largest = bnf::is_zero(y.c1) ? lex_largest(y.c0) : lex_largest(y.c1);
    if (largest != (flag == 3)) y = H2::neg(y);
    H2::store(x, w);
    H2::store(y, w + 8);
    return true;
}
void g2_negate(const uint64_t* in, uint64_t* out) {
    memcpy(out, in, 128);
    uint64_t o = 0;
    for (int i = 0; i < 16; i++) o |= in[i];
    if (o) H2::store(H2::neg(H2::load(in + 8)), out + 8);
}

int32_t vk_build(nlx_ctx* ctx, const nlx_bn254_groth16_vk_desc* d, nlx_bn254_groth16_vk* vk) {
    const uint32_t k = d->n_commitments;
    if (d->n_public == 0) return ctx->fail(NLX_E_RANGE, "n_public counts the constant wire: at least 1");
    if (k > NLX_BN254_GROTH16_MAX_COMMITMENTS) return ctx->fail(NLX_E_RANGE, "%u commitments: at most %d", k, NLX_BN254_GROTH16_MAX_COMMITMENTS);
    if (d->n_ic != (uint64_t)d->n_public + k) return ctx->fail(NLX_E_RANGE, "ic holds %llu points, the key has %u public wires and %u commitments",
                                                                  (unsigned long long)d->n_ic, d->n_public, k);
    if (d->n_public > (1u << 20)) return ctx->fail(NLX_E_RANGE, "at most 2^20 public wires");
    if (!d->g1_alpha || !d->g2_beta || !d->g2_gamma || !d->g2_delta || !d->ic) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (k && (!d->n_hashed || !d->pedersen_g || !d->pedersen_g_root_sigma_neg)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    vk->n_public = d->n_public;
    vk->k = k;
    size_t at = 0;
    for (uint32_t j = 0; j < k; j++) {
        if (d->n_hashed[j] && !d->hashed) return ctx->fail(NLX_E_INVAL, "NULL argument");
        std::vector<uint32_t> ids;
        if (d->n_hashed[j]) ids.assign(d->hashed + at, d->hashed + at + d->n_hashed[j]);
        at += d->n_hashed[j];
        for (uint32_t id : ids)
            if (id >= d->n_public + j) return ctx->fail(NLX_E_RANGE, "commitment %u hashes wire id %u: not a public wire or an earlier commitment's", j, id);
        vk->hashed.push_back(ids);
    }
    // every point through the device's checks: G1 = alpha, ic; G2 = beta, gamma, delta (, the Pedersen pair)
    const size_t n1 = 1 + d->n_ic, n2 = 3 + (k ? 2 : 0);
    std::vector<uint64_t> g1(n1 * 8), g2(n2 * 16);
    memcpy(g1.data(), d->g1_alpha, 64);
    memcpy(g1.data() + 8, d->ic, d->n_ic * 64);
    const uint64_t* g2src[5] = {d->g2_beta, d->g2_gamma, d->g2_delta, d->pedersen_g, d->pedersen_g_root_sigma_neg};
    for (size_t i = 0; i < n2; i++) memcpy(g2.data() + 16 * i, g2src[i], 128);
    Scratch scratch(ctx);
    uint64_t* d_g1 = scratch.alloc_as<uint64_t>(g1.size() * 8);
    uint64_t* d_g2 = scratch.alloc_as<uint64_t>(g2.size() * 8);
    uint32_t* d_result = scratch.alloc_as<uint32_t>(4);
    vk->d_ic = (uint64_t*)ctx->alloc(d->n_ic * 64);
    if (vk->d_ic) vk->blocks.push_back(vk->d_ic);
    vk->d_eab = (uint64_t*)ctx->alloc(48 * 8);
    if (vk->d_eab) vk->blocks.push_back(vk->d_eab);
    if (!d_g1 || !d_g2 || !d_result || !vk->d_ic || !vk->d_eab) return scratch.finish(ctx->fail(NLX_E_NOMEM, "verifying key: device memory"));
    auto body = [&]() -> int32_t {
        NLX_HIP(ctx, hipMemcpyAsync(d_g1, g1.data(), g1.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        NLX_HIP(ctx, hipMemcpyAsync(d_g2, g2.data(), g2.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        NLX_RC(check_points(ctx, scratch, d_g1, nullptr, n1, "verifying key G1 point (alpha, then ic)"));
        NLX_RC(check_points(ctx, scratch, nullptr, d_g2, n2, "verifying key G2 point (beta, gamma, delta, the Pedersen pair)"));
        NLX_HIP(ctx, hipMemcpyAsync(vk->d_ic, d_g1 + 8, d->n_ic * 64, hipMemcpyDeviceToDevice, ctx->stream));
        NLX_RC(enqueue_checks(ctx, scratch, d_g1, d_g2, 1, nullptr, 1, 0, nullptr, 1, vk->d_eab, d_result));   // e(alpha, beta)
        std::vector<uint32_t> res;
        return read_results(ctx, d_result, 1, res, nullptr);
    };
    const int32_t rc = scratch.finish(body());
    if (rc) return rc;
    g2_negate(d->g2_gamma, vk->neg_gamma);
    g2_negate(d->g2_delta, vk->neg_delta);
    if (k) {
        memcpy(vk->ped_g, d->pedersen_g, 128);
        memcpy(vk->ped_grs, d->pedersen_g_root_sigma_neg, 128);
    }
    return NLX_OK;
}

const uint8_t COMMITMENT_DST[] = "bsb22-commitment", FOLD_DST[] = "G16-BSB22";

struct Decoded {
    bool ok = false;
    uint32_t bad_index = 0;
    uint64_t ar[8], bs[16], krs[8], pok[8];
    std::vector<uint64_t> cs;       // k x 8
    std::vector<Fr> challenges;     // canonical values of the commitment wires
    std::vector<Fr> rho_pow;        // canonical rho^j
};

// the host half of one proof: bytes -> points, the commitment wires' values, rho
int32_t decode_proof(const nlx_bn254_groth16_vk* vk, const uint8_t* p, size_t len, const Fr* publics /* canonical, n_public - 1 */, Decoded& o) {
    const uint32_t k = vk->k;
    o.ok = false;
    o.bad_index = 0;
    if (len < 164) return NLX_OK;
    const uint32_t count = ((uint32_t)p[128] << 24) | ((uint32_t)p[129] << 16) | ((uint32_t)p[130] << 8) | p[131];
    if (count != k || len != 164 + 32 * (size_t)k) return NLX_OK;
    o.cs.assign((size_t)k * 8, 0);
    if (!g1_decode(p, o.ar)) return NLX_OK;
    o.bad_index = 1;
    if (!g2_decode(p + 32, o.bs)) return NLX_OK;
    o.bad_index = 2;
    if (!g1_decode(p + 96, o.krs)) return NLX_OK;
    for (uint32_t j = 0; j < k; j++) {
        o.bad_index = 3 + j;
        if (!g1_decode(p + 132 + 32 * j, o.cs.data() + 8 * j)) return NLX_OK;
    }
    o.bad_index = 3 + k;
    if (!g1_decode(p + 132 + 32 * k, o.pok)) return NLX_OK;
    o.bad_index = 0;
    o.challenges.clear();
    o.rho_pow.clear();
    std::vector<uint8_t> msg;
    Fr one_c = bnf::zero<RP>();
    one_c.v[0] = 1;
    for (uint32_t j = 0; j < k; j++) {
        msg.assign(64, 0);
        g1_marshal(o.cs.data() + 8 * j, msg.data());
        for (uint32_t id : vk->hashed[j]) {
            const Fr v = id == 0 ? one_c : id < vk->n_public ? publics[id - 1] : o.challenges[id - vk->n_public];
            msg.resize(msg.size() + 32);
            fr_to_be(v, msg.data() + msg.size() - 32);
        }
        uint64_t h[4];
        const int32_t rc = nlx_bn254_hash_to_field(msg.data(), msg.size(), COMMITMENT_DST, sizeof COMMITMENT_DST - 1, h);
        if (rc) return rc;
        o.challenges.push_back(bnf::from_mont(bnf::load_words<RP>(h)));
    }
    if (k) {
        msg.assign((size_t)k * 32, 0);
        for (uint32_t j = 0; j < k; j++) fr_to_be(o.challenges[j], msg.data() + 32 * j);
        uint64_t h[4];
        const int32_t rc = nlx_bn254_hash_to_field(msg.data(), msg.size(), FOLD_DST, sizeof FOLD_DST - 1, h);
        if (rc) return rc;
        const Fr rho = bnf::load_words<RP>(h);   // Montgomery
        Fr pw = bnf::one<RP>();
        for (uint32_t j = 0; j < k; j++) {
            o.rho_pow.push_back(bnf::from_mont(pw));
            pw = bnf::mul(pw, rho);
        }
    }
    o.ok = true;
    return NLX_OK;
}

const char* reason_text(uint32_t r) {
    return r == NLX_BN254_VERIFY_MALFORMED ? "malformed" : r == NLX_BN254_VERIFY_PEDERSEN ? "the Pedersen proof of knowledge fails"
         : r == NLX_BN254_VERIFY_PAIRING ? "the pairing equation fails" : "accepted";
}

int32_t verify_body(const nlx_bn254_groth16_vk* vk, Scratch& scratch, const uint8_t* const* proofs, const size_t* lens, size_t n,
                    const uint64_t* public_inputs, nlx_bn254_verdict* verdicts) {
    nlx_ctx* ctx = vk->ctx;
    const uint32_t k = vk->k, np1 = vk->n_public - 1;
    // the callers' scalars: below r, canonical
    std::vector<Fr> publics(n * (size_t)np1);
    for (size_t i = 0; i < publics.size(); i++) {
        if (!bnf::below_mod<RP>(public_inputs + 4 * i))
            return ctx->fail(NLX_E_RANGE, "proof %zu, public input %zu is not below r", i / np1, i % np1 + 1);
        publics[i] = bnf::from_mont(bnf::load_words<RP>(public_inputs + 4 * i));
    }
    std::vector<Decoded> dec(n);
    for (size_t i = 0; i < n; i++) NLX_RC(decode_proof(vk, proofs[i], lens[i], publics.data() + i * np1, dec[i]));
    // pairs: check i < n is proof i's pairing check (Ar, Bs) (kSum, -gamma) (Krs, -delta), compared with e(alpha, beta);
    // check n + i its Pedersen check (sum_j rho^j C_j, [-1/sigma]_2) (Pok, [1]_2), compared with 1.  A malformed proof's pairs
    // stay at infinity and its results are not read.
    const size_t n_checks = k ? 2 * n : n, n_pairs = (k ? 5 : 3) * n;
    if (n_pairs > MAX_PAIRS) return ctx->fail(NLX_E_RANGE, "at most 2^20 pairs per call");
    std::vector<uint64_t> g1(n_pairs * 8, 0), g2(n_pairs * 16, 0);
    std::vector<uint32_t> first(n_checks + 1);
    for (size_t i = 0; i <= n; i++) first[i] = (uint32_t)(3 * i);
    for (size_t i = 1; k && i <= n; i++) first[n + i] = (uint32_t)(3 * n + 2 * i);
    // terms of the sums: segment i < n is kSum_i, segment n + i the folded commitment
    const size_t terms_per = (size_t)vk->n_public + 2 * k, n_seg = k ? 2 * n : n;
    std::vector<uint32_t> src, seg_first(1, 0), seg_dst;
    std::vector<uint64_t> scalars, extra(n * (size_t)k * 8 + 8, 0);
    src.reserve(n * (terms_per + k));
    const uint64_t one_words[4] = {1, 0, 0, 0};
    auto push = [&](uint32_t s, const uint64_t* w) {
        src.push_back(s);
        scalars.insert(scalars.end(), w, w + 4);
    };
    auto fr_words = [](const Fr& a, uint64_t* w) { bnf::store_words(a, w); };
    for (size_t i = 0; i < n; i++) {
        const Decoded& d = dec[i];
        if (d.ok) {
            memcpy(&g1[8 * (3 * i)], d.ar, 64);
            memcpy(&g2[16 * (3 * i)], d.bs, 128);
            memcpy(&g2[16 * (3 * i + 1)], vk->neg_gamma, 128);
            memcpy(&g1[8 * (3 * i + 2)], d.krs, 64);
            memcpy(&g2[16 * (3 * i + 2)], vk->neg_delta, 128);
            if (k) memcpy(&extra[8 * i * k], d.cs.data(), (size_t)k * 64);
            push(0, one_words);
            uint64_t w[4];
            for (uint32_t t = 0; t < np1; t++) {
                fr_words(publics[i * np1 + t], w);
                push(1 + t, w);
            }
            for (uint32_t j = 0; j < k; j++) {
                fr_words(d.challenges[j], w);
                push(vk->n_public + j, w);
                push(SRC_EXTRA | (uint32_t)(i * k + j), one_words);
            }
        }
        seg_first.push_back((uint32_t)src.size());
        seg_dst.push_back((uint32_t)(3 * i + 1));
    }
    for (size_t i = 0; k && i < n; i++) {
        const Decoded& d = dec[i];
        if (d.ok) {
            memcpy(&g2[16 * (3 * n + 2 * i)], vk->ped_grs, 128);
            memcpy(&g1[8 * (3 * n + 2 * i + 1)], d.pok, 64);
            memcpy(&g2[16 * (3 * n + 2 * i + 1)], vk->ped_g, 128);
            uint64_t w[4];
            for (uint32_t j = 0; j < k; j++) {
                fr_words(d.rho_pow[j], w);
                push(SRC_EXTRA | (uint32_t)(i * k + j), w);
            }
        }
        seg_first.push_back((uint32_t)src.size());
        seg_dst.push_back((uint32_t)(3 * n + 2 * i));
    }
    const size_t n_terms = src.size();
    if (n_terms >= SRC_EXTRA) return ctx->fail(NLX_E_RANGE, "too many terms");
    uint64_t* d_g1 = scratch.alloc_as<uint64_t>(g1.size() * 8);
    uint64_t* d_g2 = scratch.alloc_as<uint64_t>(g2.size() * 8);
    uint64_t* d_extra = scratch.alloc_as<uint64_t>(extra.size() * 8);
    uint64_t* d_scalars = scratch.alloc_as<uint64_t>((n_terms + 1) * 32);
    // one block of words: src | seg_first | seg_dst | first, and one of answers: status (n) | result (n_checks)
    std::vector<uint32_t> words;
    words.insert(words.end(), src.begin(), src.end());
    const size_t o_segf = words.size();
    words.insert(words.end(), seg_first.begin(), seg_first.end());
    const size_t o_segd = words.size();
    words.insert(words.end(), seg_dst.begin(), seg_dst.end());
    const size_t o_first = words.size();
    words.insert(words.end(), first.begin(), first.end());
    uint32_t* d_words = scratch.alloc_as<uint32_t>(words.size() * 4);
    uint32_t* d_answers = scratch.alloc_as<uint32_t>((n + n_checks) * 4);
    msm::Jac29* d_terms = scratch.alloc_as<msm::Jac29>((n_terms + 1) * sizeof(msm::Jac29));
    if (!d_g1 || !d_g2 || !d_extra || !d_scalars || !d_words || !d_answers || !d_terms) return ctx->fail(NLX_E_NOMEM, "groth16 verify: device memory");
    hipStream_t st = ctx->stream;
    NLX_HIP(ctx, hipMemcpyAsync(d_g1, g1.data(), g1.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_g2, g2.data(), g2.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_extra, extra.data(), extra.size() * 8, hipMemcpyHostToDevice, st));
    if (n_terms) NLX_HIP(ctx, hipMemcpyAsync(d_scalars, scalars.data(), scalars.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_words, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemsetAsync(d_answers, 0xFF, (n + n_checks) * 4, st));
    ctx->begin_kernel("bn254_groth16_ksum", 96.0 * (double)n_terms, (double)n_terms);
    if (n_terms)
        hipLaunchKernelGGL(k_bn254_g16_ksum, dim3(blocks64(n_terms)), dim3(64), 0, st, (const uint64_t*)vk->d_ic, (const uint64_t*)d_extra,
                           (const uint32_t*)d_words, (const uint64_t*)d_scalars, (uint32_t)n_terms, d_terms);
    hipLaunchKernelGGL(k_bn254_g16_ksum_reduce, dim3(blocks64(n_seg)), dim3(64), 0, st, (const msm::Jac29*)d_terms, (const uint32_t*)(d_words + o_segf),
                       (const uint32_t*)(d_words + o_segd), (uint32_t)n_seg, d_g1);
    ctx->end_kernel();
    // the subgroup test of Bs: pair 3 i of the G2 side (the G1 side is on the curve by decompression)
    ctx->begin_kernel("bn254_pairing_points", 128.0 * (double)n, (double)n);
    hipLaunchKernelGGL(k_bn254_pairing_points, dim3(blocks64(n)), dim3(64), 0, st, (const uint64_t*)nullptr, (const uint64_t*)d_g2, (uint32_t)n, 0u, 48u,
                       d_answers);
    ctx->end_kernel();
    NLX_RC(enqueue_checks(ctx, scratch, d_g1, d_g2, n_pairs, d_words + o_first, n_checks, n, vk->d_eab, 0, nullptr, d_answers + n));
    std::vector<uint32_t> ans(n + n_checks);
    NLX_RC(fetch(ctx, ans.data(), d_answers, ans.size() * 4));
    bool named = false;
    for (size_t i = 0; i < n; i++) {
        nlx_bn254_verdict& v = verdicts[i];
        if (!dec[i].ok) {
            v.reason = NLX_BN254_VERIFY_MALFORMED;
            v.index = dec[i].bad_index;
        } else {
            const uint32_t sub = ans[i], pairing_ok = ans[n + i], pedersen_ok = k ? ans[2 * n + i] : 1u;
            if (sub == WORD_UNSET || pairing_ok > 1 || pedersen_ok > 1) return ctx->fail(NLX_E_HIP, "groth16 verify: a kernel wrote no answer for proof %zu", i);
            if (sub != POINT_OK) {
                v.reason = NLX_BN254_VERIFY_MALFORMED;
                v.index = 1;
            } else if (!pedersen_ok) {
                v.reason = NLX_BN254_VERIFY_PEDERSEN;
            } else if (!pairing_ok) {
                v.reason = NLX_BN254_VERIFY_PAIRING;
            } else {
                v.accepted = 1;
            }
        }
        if (!v.accepted && !named) {
            named = true;
            ctx->fail(NLX_OK, "proof %zu rejected: %s (point %u)", i, reason_text(v.reason), v.index);
        }
    }
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_groth16_vk_create(nlx_ctx* ctx, const nlx_bn254_groth16_vk_desc* desc, nlx_bn254_groth16_vk** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    nlx_bn254_groth16_vk* vk = new nlx_bn254_groth16_vk();
    vk->ctx = ctx;
    const int32_t rc = vk_build(ctx, desc, vk);
    if (rc) {
        vk_free(vk);
        return rc;
    }
    *out = vk;
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_groth16_vk_destroy(nlx_bn254_groth16_vk* vk) NLX_TRY {
    vk_free(vk);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_groth16_verify_batch(const nlx_bn254_groth16_vk* vk, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                                                  const uint64_t* public_inputs, nlx_bn254_verdict* verdicts) NLX_TRY {
    if (!vk) return NLX_E_INVAL;
    nlx_ctx* ctx = vk->ctx;
    for (size_t i = 0; verdicts && i < n_proofs; i++) verdicts[i] = nlx_bn254_verdict{0, 0, 0};
    if (n_proofs && (!proofs || !lens || !verdicts || (vk->n_public > 1 && !public_inputs))) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (n_proofs > ((size_t)1 << 17)) return ctx->fail(NLX_E_RANGE, "at most 2^17 proofs per call");
    if (!n_proofs) return NLX_OK;
    (void)hipSetDevice(ctx->device);
    if (vk->n_public > 1 && is_device_ptr(public_inputs)) return ctx->fail(NLX_E_INVAL, "public_inputs is a host array");
    Scratch scratch(ctx);
    return scratch.finish(verify_body(vk, scratch, proofs, lens, n_proofs, public_inputs, verdicts));
} NLX_CATCH(vk ? vk->ctx : nullptr)

extern "C" int32_t nlx_bn254_groth16_verify(const nlx_bn254_groth16_vk* vk, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                                            nlx_bn254_verdict* verdict) NLX_TRY {
    if (!vk) return NLX_E_INVAL;
    if (verdict) *verdict = nlx_bn254_verdict{0, 0, 0};
    if (!proof || !verdict) return vk->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_bn254_groth16_verify_batch(vk, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(vk ? vk->ctx : nullptr)
