// Segmented G1 linear combinations: out[s] = sum_t scalars[t] * points[t] over the
// terms of segment s - many short sums at once, one per proof and digest of a verifier's batch.  Neither the bucket MSM (built
// for 2^20 points of one sum) nor the Groth16 verifier's public sum (a lane per term, then one lane walking a segment's terms).
//
//   k_bn254_g1_lincomb_check  one lane per term: the point as nlx_bn254_pairing checks a G1 point, the scalar below r -> a
//                             status word
//   k_bn254_g1_lincomb        one wave per segment, the lane is the term: lane l takes terms l, l + 64, .. of its segment, each
//                             by double-and-add on bn254_curve29.hpp's group law, into one partial sum; the 64 partial sums
//                             are added as a tree over the wave through LDS in six rounds of jadd29 (one Jac29 is 108 bytes:
//                             6912 bytes a block); lane 0 inverts z once and writes the affine words
// The points are chosen by whoever wrote the proof, so the tree must be right for P + P, P + (-P), P + O and O + O: jadd29
// answers the first by its doubling, the second by the point at infinity and passes the other two through.  A scalar of 0 and a
// lane without a term contribute the point at infinity.  No loop bound depends on a value: the ladder runs 254 steps, the tree
// six rounds; the scalars are public, so the ladder branches on their bits.
#include <vector>
#include "bn254_curve29.hpp"
#include "bn254_g1_lincomb.hpp"
#include "bn254_pairing.hpp"
#include "bn254_pairing_launch.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

using namespace nlx;

namespace {

using pairing::WORD_UNSET;
constexpr uint32_t TERM_OK = pairing::POINT_OK, TERM_SCALAR_RANGE = 6;   // between them: pairing::G1_RANGE, G1_OFF_CURVE

__global__ __launch_bounds__(64) void k_bn254_g1_lincomb_check(const uint64_t* __restrict__ points, const uint64_t* __restrict__ scalars, uint32_t n,
                                                               uint32_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    uint32_t st = pairing::check_g1(points + 8 * (size_t)t);
    if (st == TERM_OK && !bnf::below_mod<bnf::RP>(scalars + 4 * (size_t)t)) st = TERM_SCALAR_RANGE;
    status[t] = st;
}

__global__ __launch_bounds__(64) void k_bn254_g1_lincomb(const uint64_t* __restrict__ points, const uint32_t* __restrict__ src,
                                                         const uint64_t* __restrict__ scalars, const uint32_t* __restrict__ first,
                                                         uint32_t n_segments, uint64_t* __restrict__ out) {
    using namespace nlx::msm;
    __shared__ Jac29 part[64];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_segments) return;   // block-uniform
    const uint32_t lo = first[s], hi = first[s + 1];
    Jac29 acc = inf29<F1>();
#pragma unroll 1
    for (uint32_t t = lo + lane; t < hi; t += 64) {
        const pairing::G1Point p = pairing::g1_load(points + 8 * (size_t)(src ? src[t] : t));
        if (p.inf) continue;
        const Aff29 a{p.x, p.y};
        const uint64_t* k = scalars + 4 * (size_t)t;
        Jac29 term = inf29<F1>();
#pragma unroll 1
        for (int bit = 253; bit >= 0; bit--) {
            term = jdbl29(term);
            if ((k[bit >> 6] >> (bit & 63)) & 1) term = jmadd29(term, a);
        }
        acc = jadd29(acc, term);
    }
    part[lane] = acc;
    __syncthreads();
#pragma unroll 1
    for (uint32_t stride = 32; stride > 0; stride >>= 1) {
        if (lane < stride) {
            acc = jadd29(acc, part[lane + stride]);
            part[lane] = acc;
        }
        __syncthreads();
    }
    if (lane != 0) return;
    uint64_t* w = out + 8 * (size_t)s;
    if (F1::is_zero_exact(acc.z) || F1::is_zero_mod(acc.z)) {
        for (int i = 0; i < 8; i++) w[i] = 0;
        return;
    }
    const Fe zi = pairing::fq_inv(F1::tighten(acc.z)), zi2 = F1::sqr(zi);
    pairing::fq_store(F1::mul(acc.x, zi2), true, w);
    pairing::fq_store(F1::mul(acc.y, F1::mul(zi2, zi)), true, w + 4);
}

const char* term_text(uint32_t st) {
    return st == pairing::G1_RANGE ? "the point has a coordinate that is not below q" : st == pairing::G1_OFF_CURVE ? "the point is not on the curve"
         : st == TERM_SCALAR_RANGE ? "the scalar is not below r" : "unknown status";
}

int32_t lincomb_body(nlx_ctx* ctx, Scratch& scratch, const uint64_t* points, const uint64_t* scalars, const uint32_t* first, size_t n_segments,
                     uint64_t* out) {
    const size_t n_terms = first[n_segments];
    Staged sp(ctx, points, (n_terms ? n_terms : 1) * 64, n_terms != 0, false), ss(ctx, scalars, (n_terms ? n_terms : 1) * 32, n_terms != 0, false);
    if (n_terms && sp.status) return sp.status;
    if (n_terms && ss.status) return ss.status;
    uint32_t* d_first = scratch.alloc_as<uint32_t>((n_segments + 1) * 4);
    uint32_t* d_status = scratch.alloc_as<uint32_t>((n_terms ? n_terms : 1) * 4);
    if (!d_first || !d_status) return ctx->fail(NLX_E_NOMEM, "g1_lincomb: device memory");
    if (n_terms) {
        NLX_HIP(ctx, hipMemsetAsync(d_status, 0xFF, n_terms * 4, ctx->stream));
        ctx->begin_kernel("bn254_g1_lincomb_check", 100.0 * (double)n_terms, (double)n_terms);
        hipLaunchKernelGGL(k_bn254_g1_lincomb_check, dim3((unsigned)((n_terms + 63) / 64)), dim3(64), 0, ctx->stream, sp.as<uint64_t>(), ss.as<uint64_t>(),
                           (uint32_t)n_terms, d_status);
        ctx->end_kernel();
        std::vector<uint32_t> status(n_terms);
        NLX_RC(fetch(ctx, status.data(), d_status, n_terms * 4));
        for (size_t t = 0; t < n_terms; t++) {
            if (status[t] == WORD_UNSET) return ctx->fail(NLX_E_HIP, "g1_lincomb: the check wrote no status for term %zu", t);
            if (status[t] != TERM_OK) return ctx->fail(NLX_E_RANGE, "term %zu: %s", t, term_text(status[t]));
        }
    }
    Staged so(ctx, out, n_segments * 64, false, true);
    if (so.status) return so.status;
    NLX_HIP(ctx, hipMemcpyAsync(d_first, first, (n_segments + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    NLX_RC(lincomb::enqueue(ctx, sp.as<uint64_t>(), nullptr, ss.as<uint64_t>(), d_first, n_segments, n_terms, so.as<uint64_t>()));
    NLX_RC(so.finish());
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `first` has been read and the copy-out is done before `so` gives its block back
    return NLX_OK;
}

}  // namespace

int32_t nlx::lincomb::enqueue(nlx_ctx* ctx, const uint64_t* d_points, const uint32_t* d_src, const uint64_t* d_scalars, const uint32_t* d_first,
                              size_t n_segments, size_t n_terms, uint64_t* d_out, const char* name) {
    if (!n_segments) return NLX_OK;
    ctx->begin_kernel(name, 96.0 * (double)n_terms + 64.0 * (double)n_segments, (double)n_terms);
    hipLaunchKernelGGL(k_bn254_g1_lincomb, dim3((unsigned)n_segments), dim3(64), 0, ctx->stream, d_points, d_src, d_scalars, d_first,
                       (uint32_t)n_segments, d_out);
    ctx->end_kernel();
    return NLX_OK;
}

extern "C" int32_t nlx_bn254_g1_lincomb(nlx_ctx* ctx, const uint64_t* points, const uint64_t* scalars, const uint32_t* first, size_t n_segments,
                                        uint64_t* out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!n_segments) return NLX_OK;
    if (!first || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    (void)hipSetDevice(ctx->device);
    if (is_device_ptr(first)) return ctx->fail(NLX_E_INVAL, "first is a host array");
    if (n_segments > lincomb::MAX_SEGMENTS) return ctx->fail(NLX_E_RANGE, "at most 2^20 segments per call");
    if (first[0] != 0) return ctx->fail(NLX_E_RANGE, "first[0] must be 0");
    for (size_t s = 0; s < n_segments; s++)
        if (first[s + 1] < first[s]) return ctx->fail(NLX_E_RANGE, "first must ascend: segment %zu", s);
    if (first[n_segments] > lincomb::MAX_TERMS) return ctx->fail(NLX_E_RANGE, "at most 2^24 terms per call");
    if (first[n_segments] && (!points || !scalars)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    Scratch scratch(ctx);
    return scratch.finish(lincomb_body(ctx, scratch, points, scalars, first, n_segments, out));
} NLX_CATCH(ctx)
