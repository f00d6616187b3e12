// Segmented G1 linear combinations on the device (bn254_g1_lincomb.hip): many short sums of scalar times
// point at once, one wave per segment.  What the PLONK verifier (bn254_plonk_verify.hip) calls twice per batch.
#pragma once
#include <cstddef>
#include <cstdint>
#include "ctx.hpp"

namespace nlx {
namespace lincomb {

constexpr size_t MAX_TERMS = (size_t)1 << 24, MAX_SEGMENTS = (size_t)1 << 20;

// out[s] = sum of scalars[t] * points[src ? src[t] : t] over first[s] <= t < first[s + 1], as G1Affine words (all zero: the
// point at infinity).  Every pointer is a device pointer; src may be NULL.  The points are taken to be on the curve and the
// scalars to be canonical integers below r: the callers have checked.  Enqueues one launch under the kernel-timing name `name`.
int32_t enqueue(nlx_ctx* ctx, const uint64_t* d_points, const uint32_t* d_src, const uint64_t* d_scalars, const uint32_t* d_first,
                size_t n_segments, size_t n_terms, uint64_t* d_out, const char* name = "bn254_g1_lincomb");

}  // namespace lincomb
}  // namespace nlx
