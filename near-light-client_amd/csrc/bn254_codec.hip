// gnark-crypto's point bytes on the device: what lets a kzg.SRS or a groth16
// ProvingKey that rests in a file come into HBM, and go back, at the speed the device makes them.  The arithmetic and every byte
// rule are bn254_codec.hpp (host and device source, checked on the host against tools/gnark_bytes_model.py); this file holds the
// four kernels and the entry points.
//
//   k_bn254_g1_decode   one lane per point: 32 or 64 bytes as 16-byte loads, the flag, the range, compressed: the fixed chain
//                       (x^3 + 3)^((q - 3) / 4) -> y and its check, raw: the curve equation; 8 Montgomery words, a status word
//   k_bn254_g2_decode   the same over Fq2 (two chains), then the pairing's subgroup test unless switched off
//   k_bn254_g1_encode / k_bn254_g2_encode   words -> bytes; a status word (OK or RANGE)
// The chains run over the bits of a compile-time constant, so a wave never diverges on them; a lane leaves early only for a bad
// point.  Every status word is preset to WORD_UNSET, which no kernel writes; k_bn254_status_lowest_bad then finds the lowest index
// that is not OK, so one word comes back to the host whatever n is.  Block sizes: the G1 kernels and the encoders hold
// a few field elements (profiles/bn254_codec_resource_usage.txt) and n is in the millions, so they run four waves a block; the
// G2 decoder carries the subgroup test's call tree, whose values rest in scratch as the pairing kernels' do, and keeps their one
// wave a block.
#include <cstring>
#include "bn254_codec.hpp"
#include "bn254_pairing_launch.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

using namespace nlx;
using nlx::pairing::WORD_UNSET;

static_assert(codec::ST_OK == NLX_BN254_POINT_OK && codec::ST_BAD_FLAG == NLX_BN254_POINT_BAD_FLAG && codec::ST_RANGE == NLX_BN254_POINT_RANGE &&
              codec::ST_BAD_INFINITY == NLX_BN254_POINT_BAD_INFINITY && codec::ST_OFF_CURVE == NLX_BN254_POINT_OFF_CURVE &&
              codec::ST_NOT_IN_SUBGROUP == NLX_BN254_POINT_NOT_IN_SUBGROUP, "the header's status values are the codec's");

namespace {

constexpr int BLOCK_G1 = 256, BLOCK_G2_DECODE = 64, BLOCK_G2_ENCODE = 256;
constexpr uint64_t MAX_POINTS = (uint64_t)1 << 28;

// Q 16-byte pieces of point i (all pointers handed to the kernels are 16-byte aligned: the entry points see to it)
template <int MAXQ>
__device__ __forceinline__ void load_pieces(const uint4* __restrict__ src, int q, uint32_t* m) {
#pragma unroll
    for (int k = 0; k < MAXQ; k++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < q) v = src[k];
        m[4 * k] = v.x, m[4 * k + 1] = v.y, m[4 * k + 2] = v.z, m[4 * k + 3] = v.w;
    }
}
template <int MAXQ>
__device__ __forceinline__ void store_pieces(uint4* __restrict__ dst, int q, const uint32_t* m) {
#pragma unroll
    for (int k = 0; k < MAXQ; k++)
        if (k < q) dst[k] = make_uint4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
}
template <int WORDS>
__device__ __forceinline__ void store_words(uint4* __restrict__ dst, const uint64_t* w) {
#pragma unroll
    for (int k = 0; k < WORDS / 2; k++)
        dst[k] = make_uint4((uint32_t)w[2 * k], (uint32_t)(w[2 * k] >> 32), (uint32_t)w[2 * k + 1], (uint32_t)(w[2 * k + 1] >> 32));
}
template <int WORDS>
__device__ __forceinline__ void load_words(const uint4* __restrict__ src, uint64_t* w) {
#pragma unroll
    for (int k = 0; k < WORDS / 2; k++) {
        const uint4 v = src[k];
        w[2 * k] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        w[2 * k + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
}

__global__ __launch_bounds__(BLOCK_G1) void k_bn254_g1_decode(const uint4* __restrict__ bytes, uint64_t n, int raw, uint4* __restrict__ points,
                                                              uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK_G1 + threadIdx.x;
    if (i >= n) return;
    const int q = raw ? 4 : 2;
    uint32_t m[16];
    uint64_t w[8];
    load_pieces<4>(bytes + i * q, q, m);
    const uint32_t st = codec::g1_decode(m, raw != 0, w);
    store_words<8>(points + i * 4, w);
    status[i] = st;
}

__global__ __launch_bounds__(BLOCK_G2_DECODE) void k_bn254_g2_decode(const uint4* __restrict__ bytes, uint64_t n, int raw, int subgroup,
                                                                     uint4* __restrict__ points, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK_G2_DECODE + threadIdx.x;
    if (i >= n) return;
    const int q = raw ? 8 : 4;
    uint32_t m[32];
    uint64_t w[16];
    load_pieces<8>(bytes + i * q, q, m);
    const uint32_t st = codec::g2_decode(m, raw != 0, subgroup != 0, w);
    store_words<16>(points + i * 8, w);
    status[i] = st;
}

__global__ __launch_bounds__(BLOCK_G1) void k_bn254_g1_encode(const uint4* __restrict__ points, uint64_t n, int raw, uint4* __restrict__ bytes,
                                                              uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK_G1 + threadIdx.x;
    if (i >= n) return;
    const int q = raw ? 4 : 2;
    uint64_t w[8];
    uint32_t m[16];
    load_words<8>(points + i * 4, w);
    const uint32_t st = codec::g1_encode(w, raw != 0, m);
    store_pieces<4>(bytes + i * q, q, m);
    status[i] = st;
}

__global__ __launch_bounds__(BLOCK_G2_ENCODE) void k_bn254_g2_encode(const uint4* __restrict__ points, uint64_t n, int raw, uint4* __restrict__ bytes,
                                                                     uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK_G2_ENCODE + threadIdx.x;
    if (i >= n) return;
    const int q = raw ? 8 : 4;
    uint64_t w[16];
    uint32_t m[32];
    load_words<16>(points + i * 8, w);
    const uint32_t st = codec::g2_encode(w, raw != 0, m);
    store_pieces<8>(bytes + i * q, q, m);
    status[i] = st;
}

// The lowest index whose status is not OK - a word no lane wrote counts - so that one word comes back to the host, not n.
// *lowest is preset to WORD_UNSET (n <= 2^28: no index reaches it); bad points are rare, so the atomics are too.
__global__ __launch_bounds__(BLOCK_G1) void k_bn254_status_lowest_bad(const uint32_t* __restrict__ status, uint64_t n, uint32_t* __restrict__ lowest) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK_G1 + threadIdx.x;
    if (i >= n) return;
    if (status[i] != codec::ST_OK) atomicMin(lowest, (uint32_t)i);
}

const char* status_text(uint32_t st) {
    switch (st) {
        case codec::ST_BAD_FLAG: return "the flag bits are not valid in this mode";
        case codec::ST_RANGE: return "a coordinate is not below q";
        case codec::ST_BAD_INFINITY: return "the infinity flag with another bit set";
        case codec::ST_OFF_CURVE: return "not on the curve (no square root, or a raw point off the curve)";
        case codec::ST_NOT_IN_SUBGROUP: return "not in the subgroup of order r";
        default: return "unknown status";
    }
}

struct Shape {
    bool g2, decode;
    const char* name;      // the kernel-timing name, and how messages call the call
    size_t bytes, words;   // of one point
};

// A 16-byte aligned device view of a staged buffer: the buffer itself, or a scratch copy of it (a caller's device pointer into
// the middle of a file's bytes can start anywhere; the kernels load and store 16 bytes at a time).
struct Aligned {
    void* p = nullptr;
    void* origin = nullptr;
    size_t bytes = 0;
    int32_t init(nlx_ctx* ctx, Scratch& scratch, void* dev, size_t nbytes, bool copy_in) {
        origin = dev, bytes = nbytes, p = dev;
        if (((uintptr_t)dev & 15) == 0) return NLX_OK;
        p = scratch.alloc(nbytes);
        if (!p) return ctx->fail(NLX_E_NOMEM, "point bytes: device memory for an aligned copy of %zu bytes", nbytes);
        if (copy_in) NLX_HIP(ctx, hipMemcpyAsync(p, dev, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
        return NLX_OK;
    }
    int32_t copy_back(nlx_ctx* ctx) {
        if (p != origin) NLX_HIP(ctx, hipMemcpyAsync(origin, p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return NLX_OK;
    }
};

inline unsigned blocks_of(uint64_t n, int block) { return (unsigned)((n + block - 1) / block); }

int32_t codec_body(nlx_ctx* ctx, Scratch& scratch, const Shape& sh, const void* in, uint64_t n, uint32_t flags, void* out, uint32_t* status_out) {
    const bool raw = (flags & NLX_BN254_POINTS_RAW) != 0;
    const size_t point_bytes = sh.bytes * (raw ? 2 : 1);
    const size_t in_bytes = n * (sh.decode ? point_bytes : sh.words * 8), out_bytes = n * (sh.decode ? sh.words * 8 : point_bytes);
    Staged s_in(ctx, in, in_bytes, true, false), s_out(ctx, out, out_bytes, false, true);
    if (s_in.status) return s_in.status == NLX_E_NOMEM ? ctx->fail(NLX_E_NOMEM, "%s: device memory for %zu bytes", sh.name, in_bytes) : s_in.status;
    if (s_out.status) return s_out.status == NLX_E_NOMEM ? ctx->fail(NLX_E_NOMEM, "%s: device memory for %zu bytes", sh.name, out_bytes) : s_out.status;
    Aligned a_in, a_out;
    NLX_RC(a_in.init(ctx, scratch, s_in.dev, in_bytes, true));
    NLX_RC(a_out.init(ctx, scratch, s_out.dev, out_bytes, false));
    uint32_t* d_status = scratch.alloc_as<uint32_t>((n + 1) * 4);   // word n: the lowest bad index, preset to "none" with the rest
    if (!d_status) return ctx->fail(NLX_E_NOMEM, "%s: device memory for %llu status words", sh.name, (unsigned long long)n);
    NLX_HIP(ctx, hipMemsetAsync(d_status, 0xFF, (n + 1) * 4, ctx->stream));
    ctx->begin_kernel(sh.name, (double)(in_bytes + out_bytes + 4 * n), (double)n);
    const uint4* src = (const uint4*)a_in.p;
    uint4* dst = (uint4*)a_out.p;
    if (sh.decode && !sh.g2)
        hipLaunchKernelGGL(k_bn254_g1_decode, dim3(blocks_of(n, BLOCK_G1)), dim3(BLOCK_G1), 0, ctx->stream, src, n, raw ? 1 : 0, dst, d_status);
    else if (sh.decode)
        hipLaunchKernelGGL(k_bn254_g2_decode, dim3(blocks_of(n, BLOCK_G2_DECODE)), dim3(BLOCK_G2_DECODE), 0, ctx->stream, src, n, raw ? 1 : 0,
                           (flags & NLX_BN254_POINTS_NO_SUBGROUP) ? 0 : 1, dst, d_status);
    else if (!sh.g2)
        hipLaunchKernelGGL(k_bn254_g1_encode, dim3(blocks_of(n, BLOCK_G1)), dim3(BLOCK_G1), 0, ctx->stream, src, n, raw ? 1 : 0, dst, d_status);
    else
        hipLaunchKernelGGL(k_bn254_g2_encode, dim3(blocks_of(n, BLOCK_G2_ENCODE)), dim3(BLOCK_G2_ENCODE), 0, ctx->stream, src, n, raw ? 1 : 0, dst,
                           d_status);
    ctx->end_kernel();
    hipLaunchKernelGGL(k_bn254_status_lowest_bad, dim3(blocks_of(n, BLOCK_G1)), dim3(BLOCK_G1), 0, ctx->stream, (const uint32_t*)d_status, n, d_status + n);
    NLX_RC(a_out.copy_back(ctx));
    // one word comes back, not n: the lowest index that is not OK; the caller's status array, if any, is copied as a whole
    uint32_t lowest = 0, st = codec::ST_OK;
    NLX_RC(fetch(ctx, &lowest, d_status + n, 4));
    if (lowest != WORD_UNSET) {
        if (lowest >= n) return ctx->fail(NLX_E_HIP, "%s: the status scan answered index %u of %llu", sh.name, lowest, (unsigned long long)n);
        NLX_RC(fetch(ctx, &st, d_status + lowest, 4));
        if (st == WORD_UNSET) return ctx->fail(NLX_E_HIP, "%s: the kernel wrote no status for point %u", sh.name, lowest);
    }
    if (status_out) {
        if (is_device_ptr(status_out)) NLX_HIP(ctx, hipMemcpyAsync(status_out, d_status, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        else NLX_RC(fetch(ctx, status_out, d_status, n * 4));
    }
    NLX_RC(s_out.finish());
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the copy-out is done before `s_out` gives its block back
    if (lowest != WORD_UNSET)
        return ctx->fail(sh.decode ? NLX_E_INVAL : NLX_E_RANGE, "%s: point %u: %s", sh.name, lowest, status_text(st));
    return NLX_OK;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

int32_t codec_entry(nlx_ctx* ctx, const Shape& sh, const void* in, uint64_t n, uint32_t flags, void* out, uint32_t* status_out) {
    if (!ctx) return NLX_E_INVAL;
    const uint32_t mode = flags & (NLX_BN254_POINTS_COMPRESSED | NLX_BN254_POINTS_RAW);
    const uint32_t known = NLX_BN254_POINTS_COMPRESSED | NLX_BN254_POINTS_RAW | (sh.g2 && sh.decode ? NLX_BN254_POINTS_NO_SUBGROUP : 0u);
    if (flags & ~known) return ctx->fail(NLX_E_RANGE, "%s: unknown flag", sh.name);
    if (mode != NLX_BN254_POINTS_COMPRESSED && mode != NLX_BN254_POINTS_RAW)
        return ctx->fail(NLX_E_RANGE, "%s: exactly one of NLX_BN254_POINTS_COMPRESSED and NLX_BN254_POINTS_RAW", sh.name);
    if (!n) return NLX_OK;
    if (n > MAX_POINTS) return ctx->fail(NLX_E_RANGE, "%s: at most 2^28 points per call", sh.name);
    if (!in || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    const size_t point_bytes = sh.bytes * (mode == NLX_BN254_POINTS_RAW ? 2 : 1);
    const size_t in_bytes = n * (sh.decode ? point_bytes : sh.words * 8), out_bytes = n * (sh.decode ? sh.words * 8 : point_bytes);
    if (overlap(in, in_bytes, out, out_bytes) || (status_out && (overlap(in, in_bytes, status_out, n * 4) || overlap(out, out_bytes, status_out, n * 4))))
        return ctx->fail(NLX_E_INVAL, "%s: input and output overlap", sh.name);
    if (((uintptr_t)(sh.decode ? out : in) & 7) || ((uintptr_t)status_out & 3)) return ctx->fail(NLX_E_INVAL, "%s: words are 8-byte aligned", sh.name);
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    return scratch.finish(codec_body(ctx, scratch, sh, in, n, flags, out, status_out));
}

}  // namespace

extern "C" int32_t nlx_bn254_g1_decode(nlx_ctx* ctx, const uint8_t* bytes, uint64_t n, uint32_t flags, uint64_t* points_out, uint32_t* status_out) NLX_TRY {
    return codec_entry(ctx, Shape{false, true, "bn254_g1_decode", 32, 8}, bytes, n, flags, points_out, status_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_g2_decode(nlx_ctx* ctx, const uint8_t* bytes, uint64_t n, uint32_t flags, uint64_t* points_out, uint32_t* status_out) NLX_TRY {
    return codec_entry(ctx, Shape{true, true, "bn254_g2_decode", 64, 16}, bytes, n, flags, points_out, status_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_g1_encode(nlx_ctx* ctx, const uint64_t* points, uint64_t n, uint32_t flags, uint8_t* bytes_out) NLX_TRY {
    return codec_entry(ctx, Shape{false, false, "bn254_g1_encode", 32, 8}, points, n, flags, bytes_out, nullptr);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_g2_encode(nlx_ctx* ctx, const uint64_t* points, uint64_t n, uint32_t flags, uint8_t* bytes_out) NLX_TRY {
    return codec_entry(ctx, Shape{true, false, "bn254_g2_encode", 64, 16}, points, n, flags, bytes_out, nullptr);
} NLX_CATCH(ctx)
