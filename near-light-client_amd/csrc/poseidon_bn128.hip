// PoseidonBN128 kernels for gfx950 (the Merkle hash of plonky2x's PoseidonBN128GoldilocksConfig; spec: tools/gen_poseidon_bn128.py,
// DESIGN.md §16): batched permutation, hash_or_noop of row-major rows and of the rows of a commitment's LDE table, Merkle levels
// with two_to_one, the commit-phase leaves of a FRI layer - and their C-ABI entry points.
//
// One state per lane: four Fr elements on nine 29-bit limbs in Montgomery form (36 VGPRs), the permutation of
// poseidon_bn128.hpp (round constants by scalar loads, one loop over the 64 rounds).  Digests leave the kernels canonical, four
// little-endian u64 words each, so cap / digest / path buffers have the shapes of the Goldilocks ones.
// Short Merkle levels and FRI leaf layers (at most nlx_ctx::pbn_quad_max_parents items) run the lane-split form instead: one state
// per quad of lanes (pbn::permute_quad), for the latency of a launch that does not fill the chip.
// A <= 4-element input whose packed value is not below r has no digest (plonky2x's from_bytes fails there): the kernel sets
// *bad and the entry point returns NLX_E_RANGE.
#include <hip/hip_runtime.h>
#include "commit.hpp"
#include "gl.hpp"
#include "poseidon_bn128_path.hpp"

namespace nlx {

using pbn::Fe;

__device__ __forceinline__ void pbn_store(uint64_t* __restrict__ out, size_t idx, const Fe& d) {
    uint64_t w[4];
    pbn::to_words(d, w);
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + idx * 4);
    dst[0] = make_ulonglong2(w[0], w[1]);
    dst[1] = make_ulonglong2(w[2], w[3]);
}

// hash_or_noop's no-op branch: <= 4 canonical Goldilocks elements are the digest, sum e_i 2^(64 i), when that is below r
__device__ __forceinline__ void pbn_noop(uint64_t* __restrict__ out, size_t idx, const uint64_t (&e)[4], uint32_t* bad) {
    if (!pbn::lt_r(e[0], e[1], e[2], e[3])) {
        atomicOr(bad, 1u);
        return;
    }
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + idx * 4);
    dst[0] = make_ulonglong2(e[0], e[1]);
    dst[1] = make_ulonglong2(e[2], e[3]);
}

// hash_no_pad's absorption of one chunk of `rem` (>= 1, wave-uniform) elements e[0..min(rem, 9)): group g of <= 3 elements
// OVERWRITES slot g + 1; slots a short chunk does not reach keep their value
__device__ __forceinline__ void pbn_absorb(Fe (&s)[pbn::T], const uint64_t (&e)[pbn::CHUNK], uint32_t rem) {
#pragma unroll
    for (int g = 0; g < 3; g++)
        if ((uint32_t)(3 * g) < rem) s[g + 1] = pbn::from_gl3(e[3 * g], e[3 * g + 1], e[3 * g + 2]);
}

// states: n x 16 words (four canonical Fr elements of four words), permuted in place; a non-canonical state is left as it is
__global__ __launch_bounds__(256) void k_pbn_permute_batch(uint64_t* __restrict__ states, size_t n, uint32_t* __restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint64_t* p = states + t * 16;
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const ulonglong2 v = reinterpret_cast<const ulonglong2*>(p)[i];
        w[2 * i] = v.x;
        w[2 * i + 1] = v.y;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < pbn::T; i++) ok = ok && pbn::lt_r(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    if (!ok) {
        atomicOr(bad, 1u);
        return;
    }
    Fe s[pbn::T];
#pragma unroll
    for (int i = 0; i < pbn::T; i++) s[i] = pbn::from_words(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    pbn::permute(s);
#pragma unroll
    for (int i = 0; i < pbn::T; i++) pbn_store(p, i, s[i]);
}

// hash_or_noop of every row of a row-major matrix (inputs taken mod p)
__global__ __launch_bounds__(256) void k_pbn_hash_rows(const uint64_t* __restrict__ rows, uint32_t row_len, size_t n_rows,
                                                       uint64_t* __restrict__ digests, uint32_t* __restrict__ bad) {
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const uint64_t* p = rows + row * (size_t)row_len;
    if (row_len <= 4) {
        uint64_t e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((uint32_t)c < row_len) e[c] = gl::canon(p[c]);
        pbn_noop(digests, row, e, bad);
        return;
    }
    Fe s[pbn::T];
#pragma unroll
    for (int i = 0; i < pbn::T; i++) s[i] = f29::zero();
#pragma unroll 1
    for (uint32_t c = 0; c < row_len; c += pbn::CHUNK) {   // one call site of the permutation; the chunk length is wave-uniform
        const uint32_t rem = row_len - c;
        uint64_t e[pbn::CHUNK];
#pragma unroll
        for (int j = 0; j < pbn::CHUNK; j++) e[j] = (uint32_t)j < rem ? gl::canon(p[c + j]) : 0;
        pbn_absorb(s, e, rem);
        pbn::permute(s);
    }
    pbn_store(digests, row, s[0]);
}

// Leaf digests of a commitment's LDE table ([col][r][k], the value at g w_L^(8k + r)): the same row -> tree position map as
// k_hash_lde_leaves (bitrev(r) n + bitrev(k)), hash_or_noop of the n_cols values of the row
__global__ __launch_bounds__(256) void k_pbn_hash_lde_leaves(const uint64_t* __restrict__ lde, size_t col_stride, uint32_t n_cols,
                                                             unsigned log_n, unsigned rate_bits, uint64_t* __restrict__ digests,
                                                             uint32_t* __restrict__ bad) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >> (log_n + rate_bits)) return;
    const uint64_t* p = lde + pos;
    const uint32_t r = (uint32_t)(pos >> log_n), k = (uint32_t)(pos & (((size_t)1 << log_n) - 1));
    const size_t leaf = ((size_t)gl::bitrev32(r, rate_bits) << log_n) + gl::bitrev32(k, log_n);
    if (n_cols <= 4) {
        uint64_t e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((uint32_t)c < n_cols) e[c] = gl::canon(p[(size_t)c * col_stride]);
        pbn_noop(digests, leaf, e, bad);
        return;
    }
    Fe s[pbn::T];
#pragma unroll
    for (int i = 0; i < pbn::T; i++) s[i] = f29::zero();
#pragma unroll 1
    for (uint32_t c = 0; c < n_cols; c += pbn::CHUNK) {   // ceil(n_cols / 9) permutations, wave-uniform
        const uint32_t rem = n_cols - c;
        uint64_t e[pbn::CHUNK];
#pragma unroll
        for (int j = 0; j < pbn::CHUNK; j++) e[j] = (uint32_t)j < rem ? gl::canon(p[(size_t)(c + j) * col_stride]) : 0;
        pbn_absorb(s, e, rem);
        pbn::permute(s);
    }
    pbn_store(digests, leaf, s[0]);
}

// one interior level: parent[i] = two_to_one(child[2i], child[2i+1]) = permute([0, 0, a, b])[0]
__global__ __launch_bounds__(256) void k_pbn_merkle_level(const uint64_t* __restrict__ children, uint64_t* __restrict__ parents,
                                                          size_t n_parents) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents) return;
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(children + i * 8);
    const ulonglong2 a0 = src[0], a1 = src[1], b0 = src[2], b1 = src[3];
    Fe s[pbn::T];
    s[0] = f29::zero();
    s[1] = f29::zero();
    s[2] = pbn::from_words(a0.x, a0.y, a1.x, a1.y);
    s[3] = pbn::from_words(b0.x, b0.y, b1.x, b1.y);
    pbn::permute(s);
    pbn_store(parents, i, s[0]);
}

// the same level with one parent per quad of lanes (pbn::permute_quad): lane q holds element q of [0, 0, a, b]
__global__ __launch_bounds__(256) void k_pbn_merkle_level_quad(const uint64_t* __restrict__ children, uint64_t* __restrict__ parents,
                                                               size_t n_parents) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = (uint32_t)(t & 3);
    const bool live = (t >> 2) < n_parents;
    const size_t i = live ? t >> 2 : n_parents - 1;   // spare quads redo the last parent and store nothing: a quad stays whole
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(children + i * 8 + (q & 1) * 4);
    const ulonglong2 a0 = src[0], a1 = src[1];
    Fe s = pbn::from_words(a0.x, a0.y, a1.x, a1.y);
#pragma unroll
    for (int l = 0; l < pbn::NL; l++) s.v[l] = q >= 2 ? s.v[l] : 0u;
    const pbn::QuadRow row = pbn::quad_row(q);
    pbn::permute_quad(s, q, row);
    if (live && q == 0) pbn_store(parents, i, s);
}

// Commit-phase leaf digests of a FRI layer (the index maps and the output layout of k_fri_leaves, prover_kernels.hip): the
// leaf's 2 arity words in slot order, hash_no_pad: ceil(2 arity / 9) = 1, 2 or 4 permutations.  Word w of a leaf is component
// w & 1 of the extension element in slot w >> 1.
__device__ __forceinline__ uint64_t pbn_fri_word(const uint64_t* __restrict__ v, size_t np, uint32_t w, int arity_bits) {
    const uint32_t mm = __brev(w >> 1) >> (32 - arity_bits);
    return gl::canon(v[((size_t)mm * np) * 2 + (w & 1)]);
}
template <int ARITY_BITS>
__global__ __launch_bounds__(256) void k_pbn_fri_leaves(const uint64_t* __restrict__ values, unsigned log_n, unsigned rate_bits,
                                                        uint64_t* __restrict__ digests) {
    constexpr uint32_t WORDS = 2u << ARITY_BITS;
    const unsigned log_np = log_n - ARITY_BITS;
    const size_t jp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (jp >> (log_np + rate_bits)) return;
    const size_t np = (size_t)1 << log_np, n = (size_t)1 << log_n;
    const uint32_t r = (uint32_t)(jp >> log_np), kp = (uint32_t)(jp & (np - 1));
    const uint64_t* v = values + ((size_t)r * n + kp) * 2;
    Fe s[pbn::T];
#pragma unroll
    for (int i = 0; i < pbn::T; i++) s[i] = f29::zero();
#pragma unroll 1
    for (uint32_t c = 0; c < WORDS; c += pbn::CHUNK) {
        const uint32_t rem = WORDS - c;
        uint64_t e[pbn::CHUNK];
#pragma unroll
        for (int j = 0; j < pbn::CHUNK; j++) e[j] = (uint32_t)j < rem ? pbn_fri_word(v, np, c + j, ARITY_BITS) : 0;
        pbn_absorb(s, e, rem);
        pbn::permute(s);
    }
    const size_t leaf = ((size_t)gl::bitrev32(r, rate_bits) << log_np) + gl::bitrev32(kp, log_np);
    pbn_store(digests, leaf, s[0]);
}
// the same with one leaf per quad: lane q >= 1 packs group q - 1 of the chunk into its slot, lane 0 keeps the capacity slot
template <int ARITY_BITS>
__global__ __launch_bounds__(256) void k_pbn_fri_leaves_quad(const uint64_t* __restrict__ values, unsigned log_n, unsigned rate_bits,
                                                             uint64_t* __restrict__ digests) {
    constexpr uint32_t WORDS = 2u << ARITY_BITS;
    const unsigned log_np = log_n - ARITY_BITS;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = (uint32_t)(t & 3);
    const size_t n_leaves = (size_t)1 << (log_np + rate_bits);
    const bool live = (t >> 2) < n_leaves;
    const size_t jp = live ? t >> 2 : n_leaves - 1;
    const size_t np = (size_t)1 << log_np, n = (size_t)1 << log_n;
    const uint32_t r = (uint32_t)(jp >> log_np), kp = (uint32_t)(jp & (np - 1));
    const uint64_t* v = values + ((size_t)r * n + kp) * 2;
    const pbn::QuadRow row = pbn::quad_row(q);
    const uint32_t g3 = 3 * ((q + 3) & 3);   // first word of this lane's group within a chunk (lane 0: past every chunk)
    Fe s = f29::zero();
#pragma unroll 1
    for (uint32_t c = 0; c < WORDS; c += pbn::CHUNK) {
        const uint32_t rem = WORDS - c;
        const bool mine = q != 0 && g3 < rem;
        uint64_t e[3];
#pragma unroll
        for (int j = 0; j < 3; j++) e[j] = (mine && g3 + j < rem) ? pbn_fri_word(v, np, c + g3 + j, ARITY_BITS) : 0;
        const Fe in = pbn::from_gl3(e[0], e[1], e[2]);
#pragma unroll
        for (int l = 0; l < pbn::NL; l++) s.v[l] = mine ? in.v[l] : s.v[l];
        pbn::permute_quad(s, q, row);
    }
    const size_t leaf = ((size_t)gl::bitrev32(r, rate_bits) << log_np) + gl::bitrev32(kp, log_np);
    if (live && q == 0) pbn_store(digests, leaf, s);
}

// verify_merkle_proof_to_cap of n (leaf, index, path) triples against one cap: one quad of lanes each, the quad's work being
// pbn::quad_merkle_path - the code the proof verifier's path kernel runs (fri_verify.hip).  leaves [n][leaf_len] (taken mod p),
// indices [n] (below 2^(path_len + cap_height): the host has checked), siblings [n][path_len][4] and cap [2^cap_height][4]
// (digests below r: the host has checked).  A leaf of <= 4 words is its own digest (hash_or_noop's no-op branch, its value below
// r by the host's check): it starts on lane 0 and nothing is absorbed.  ok[i] = 1: the path reaches the cap.  Spare quads redo
// the last item and store nothing.
__global__ __launch_bounds__(64) void k_pbn_merkle_verify(const uint64_t* __restrict__ leaves, uint32_t n, uint32_t leaf_len,
                                                          const uint64_t* __restrict__ indices, const uint64_t* __restrict__ siblings,
                                                          uint32_t path_len, const uint64_t* __restrict__ cap, uint8_t* __restrict__ ok) {
    const uint32_t q = threadIdx.x & 3;
    const uint32_t raw = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool live = raw < n;
    const uint32_t item = live ? raw : n - 1;
    const uint64_t* row = leaves + (size_t)item * leaf_len;
    const uint64_t index = indices[item];
    Fe s = f29::zero();
    if (leaf_len <= 4) {   // kernel-uniform
        uint64_t e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((uint32_t)c < leaf_len) e[c] = gl::canon(row[c]);
        const Fe d = pbn::from_words(e[0], e[1], e[2], e[3]);
#pragma unroll
        for (int l = 0; l < pbn::NL; l++) s.v[l] = q == 0 ? d.v[l] : 0u;
    }
    const pbn::QuadRow qrow = pbn::quad_row(q);
    // only the low path_len bits of the index steer the path (path_len <= 31)
    s = pbn::quad_merkle_path(s, row, leaf_len <= 4 ? 0 : leaf_len, (uint32_t)index, siblings + (size_t)item * path_len * 4, path_len, q, qrow);
    uint64_t d[4];
    pbn::to_words(s, d);
    const uint64_t* c = cap + (size_t)(index >> path_len) * 4;
    const bool good = d[0] == c[0] && d[1] == c[1] && d[2] == c[2] && d[3] == c[3];
    if (live && q == 0) ok[item] = good ? 1 : 0;
}

// ---- host launchers (stream-ordered, no synchronisation); `bad`: a device word the caller zeroed ----
static unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

void launch_pbn_hash_lde_leaves(hipStream_t st, const uint64_t* d_lde, size_t col_stride, uint32_t n_cols, unsigned log_n,
                                unsigned rate_bits, uint64_t* d_digests, uint32_t* d_bad) {
    const size_t rows = (size_t)1 << (log_n + rate_bits);
    hipLaunchKernelGGL(k_pbn_hash_lde_leaves, dim3(blocks_of(rows)), dim3(256), 0, st, d_lde, col_stride, n_cols, log_n, rate_bits,
                       d_digests, d_bad);
}

// level-major digests from the leaf level down to the cap level; returns the cap inside d_digests.  Every level is one launch:
// below ~2^16 parents a level no longer fills the chip and costs one permutation's latency, which the lane-split kernel shortens.
// Levels of at most quad_max_parents parents go through the lane-split kernel (nlx_ctx::pbn_quad_max_parents).
const uint64_t* launch_pbn_merkle_levels(hipStream_t st, uint64_t* d_digests, size_t n_leaves, unsigned cap_height,
                                         size_t quad_max_parents) {
    const size_t cap = (size_t)1 << cap_height;
    uint64_t* cur = d_digests;
    size_t lvl = n_leaves;
    while (lvl > cap) {
        uint64_t* nxt = cur + lvl * 4;
        const size_t half = lvl >> 1;
        if (half <= quad_max_parents) hipLaunchKernelGGL(k_pbn_merkle_level_quad, dim3(blocks_of(4 * half)), dim3(256), 0, st, cur, nxt, half);
        else hipLaunchKernelGGL(k_pbn_merkle_level, dim3(blocks_of(half)), dim3(256), 0, st, cur, nxt, half);
        cur = nxt;
        lvl = half;
    }
    return cur;
}

void launch_pbn_fri_leaves(hipStream_t st, const uint64_t* d_values, unsigned log_n, unsigned rate_bits, unsigned arity_bits,
                           uint64_t* d_digests, size_t quad_max_leaves) {
    const size_t leaves = (size_t)1 << (log_n - arity_bits + rate_bits);
    const bool quad = leaves <= quad_max_leaves;
    const dim3 grid(blocks_of(quad ? 4 * leaves : leaves)), block(256);
#define NLX_PBN_FRI(AB)                                                                                                   \
    if (quad) hipLaunchKernelGGL(k_pbn_fri_leaves_quad<AB>, grid, block, 0, st, d_values, log_n, rate_bits, d_digests);   \
    else hipLaunchKernelGGL(k_pbn_fri_leaves<AB>, grid, block, 0, st, d_values, log_n, rate_bits, d_digests)
    if (arity_bits == 4) { NLX_PBN_FRI(4); }
    else if (arity_bits == 3) { NLX_PBN_FRI(3); }
    else if (arity_bits == 2) { NLX_PBN_FRI(2); }
#undef NLX_PBN_FRI
}

}  // namespace nlx

using namespace nlx;

extern "C" {

int32_t nlx_poseidon_bn128_permute_batch(nlx_ctx* ctx, uint64_t* states, size_t n) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n == 0) return NLX_OK;
    if (!states) return ctx->fail(NLX_E_INVAL, "states is NULL");
    (void)hipSetDevice(ctx->device);
    Staged s(ctx, states, n * 16 * 8, true, true);
    if (s.status) return s.status;
    RangeFlag bad(ctx);
    if (!bad.d) return NLX_E_NOMEM;
    hipLaunchKernelGGL(k_pbn_permute_batch, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, s.as<uint64_t>(), n, bad.d);
    NLX_HIP(ctx, hipGetLastError());
    int32_t rc = bad.check("nlx_poseidon_bn128_permute_batch");
    if (rc) return rc;
    rc = s.finish();
    if (rc) return rc;
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_poseidon_bn128_hash_rows(nlx_ctx* ctx, const uint64_t* rows, size_t n_rows, size_t row_len, uint64_t* digests_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n_rows == 0) return NLX_OK;
    if (!digests_out || (!rows && row_len)) return ctx->fail(NLX_E_INVAL, "NULL buffer");
    if (row_len > 0xFFFFFFFFull) return ctx->fail(NLX_E_RANGE, "row_len too large");
    (void)hipSetDevice(ctx->device);
    Staged in(ctx, rows, n_rows * row_len * 8, true, false);
    Staged out(ctx, digests_out, n_rows * 32, false, true);
    if (in.status) return in.status;
    if (out.status) return out.status;
    RangeFlag bad(ctx);
    if (!bad.d) return NLX_E_NOMEM;
    hipLaunchKernelGGL(k_pbn_hash_rows, dim3(blocks_of(n_rows)), dim3(256), 0, ctx->stream, in.as<uint64_t>(), (uint32_t)row_len,
                       n_rows, out.as<uint64_t>(), bad.d);
    NLX_HIP(ctx, hipGetLastError());
    int32_t rc = bad.check("nlx_poseidon_bn128_hash_rows");
    if (rc) return rc;
    rc = out.finish();
    if (rc) return rc;
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_poseidon_bn128_merkle_build(nlx_ctx* ctx, const uint64_t* leaves, size_t n_leaves, size_t leaf_len, uint32_t cap_height,
                                        uint64_t* digests_out, uint64_t* cap_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n_leaves == 0 || (n_leaves & (n_leaves - 1))) return ctx->fail(NLX_E_INVAL, "n_leaves must be a power of two");
    if (cap_height > 63 || ((size_t)1 << cap_height) > n_leaves)
        return ctx->fail(NLX_E_RANGE, "cap_height %u exceeds log2(n_leaves)", cap_height);
    if (!cap_out || (!leaves && leaf_len)) return ctx->fail(NLX_E_INVAL, "NULL buffer");
    if (leaf_len > 0xFFFFFFFFull) return ctx->fail(NLX_E_RANGE, "leaf_len too large");
    (void)hipSetDevice(ctx->device);
    const size_t words = merkle_digest_words(n_leaves, cap_height);
    Staged in(ctx, leaves, n_leaves * leaf_len * 8, true, false);
    if (in.status) return in.status;
    Staged dig(ctx, digests_out ? (void*)digests_out : nullptr, words * 8, false, digests_out != nullptr);
    if (dig.status) return dig.status;
    Scratch scratch(ctx);
    uint64_t* d_dig = digests_out ? dig.as<uint64_t>() : scratch.alloc_as<uint64_t>(words * 8);
    if (!d_dig) return NLX_E_NOMEM;
    RangeFlag bad(ctx);
    int32_t rc = bad.d ? NLX_OK : NLX_E_NOMEM;
    if (!rc) {
        hipLaunchKernelGGL(k_pbn_hash_rows, dim3(blocks_of(n_leaves)), dim3(256), 0, ctx->stream, in.as<uint64_t>(),
                           (uint32_t)leaf_len, n_leaves, d_dig, bad.d);
        ctx->begin_kernel("merkle_levels_bn128", 64.0 * n_leaves, (double)n_leaves - (double)((size_t)1 << cap_height));
        const uint64_t* d_cap = launch_pbn_merkle_levels(ctx->stream, d_dig, n_leaves, cap_height, ctx->pbn_quad_max_parents);
        ctx->end_kernel();
        const hipError_t le = hipGetLastError();
        rc = le != hipSuccess ? ctx->hip_fail(le, "kernel launch") : bad.check("nlx_poseidon_bn128_merkle_build");
        if (!rc) {
            hipError_t e = hipMemcpyAsync(cap_out, d_cap, ((size_t)32) << cap_height,
                                          is_device_ptr(cap_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream);
            if (e != hipSuccess) rc = ctx->hip_fail(e, "hipMemcpyAsync(cap)");
        }
        if (!rc && digests_out) rc = dig.finish();
        const hipError_t e = scratch.drain();
        if (!rc && e != hipSuccess) rc = ctx->hip_fail(e, "hipStreamSynchronize");
    }
    return rc;
} NLX_CATCH(ctx)

int32_t nlx_poseidon_bn128_merkle_verify_batch(nlx_ctx* ctx, const uint64_t* leaves, size_t n, size_t leaf_len, const uint64_t* indices,
                                               const uint64_t* siblings, uint32_t path_len, const uint64_t* cap, uint32_t cap_height,
                                               uint8_t* ok_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (n == 0) return NLX_OK;
    if (!indices || !cap || !ok_out || (!leaves && leaf_len) || (!siblings && path_len)) return ctx->fail(NLX_E_INVAL, "NULL buffer");
    if (is_device_ptr(leaves) || is_device_ptr(indices) || is_device_ptr(siblings) || is_device_ptr(cap) || is_device_ptr(ok_out))
        return ctx->fail(NLX_E_INVAL, "nlx_poseidon_bn128_merkle_verify_batch takes host arrays");
    if (leaf_len > 0xFFFFFFFFull) return ctx->fail(NLX_E_RANGE, "leaf_len too large");
    if (n > 0x0FFFFFFFull) return ctx->fail(NLX_E_RANGE, "too many paths in one call");
    if (path_len > 31 || cap_height > 31 || path_len + cap_height > 32) return ctx->fail(NLX_E_RANGE, "a tree of more than 2^32 leaves");
    // the range rules, on the host: what the device indexes with, and every value that must be a digest
    for (size_t i = 0; i < n; i++)
        if (indices[i] >> (path_len + cap_height)) return ctx->fail(NLX_E_RANGE, "index %llu is not below 2^(path_len + cap_height)", (unsigned long long)i);
    const size_t n_cap = (size_t)1 << cap_height;
    for (size_t i = 0; i < n_cap; i++)
        if (!bnf::below_mod<bnf::RP>(cap + 4 * i)) return ctx->fail(NLX_E_RANGE, "cap entry %llu is not below r", (unsigned long long)i);
    for (size_t i = 0; i < n * path_len; i++)
        if (!bnf::below_mod<bnf::RP>(siblings + 4 * i))
            return ctx->fail(NLX_E_RANGE, "sibling %llu of path %llu is not below r", (unsigned long long)(i % path_len), (unsigned long long)(i / path_len));
    if (leaf_len <= 4)   // hash_or_noop's no-op branch, as nlx_poseidon_bn128_hash_rows: the packed row is the digest
        for (size_t i = 0; i < n; i++) {
            uint64_t e[4] = {0, 0, 0, 0};
            for (size_t c = 0; c < leaf_len; c++) e[c] = gl::canon(leaves[i * leaf_len + c]);
            if (!bnf::below_mod<bnf::RP>(e)) return ctx->fail(NLX_E_RANGE, "leaf %llu packs to a value that is not below r", (unsigned long long)i);
        }
    (void)hipSetDevice(ctx->device);
    Staged d_leaves(ctx, leaves, n * leaf_len * 8, true, false);
    Staged d_idx(ctx, indices, n * 8, true, false);
    Staged d_sib(ctx, siblings, n * path_len * 32, true, false);
    Staged d_cap(ctx, cap, n_cap * 32, true, false);
    Staged d_ok(ctx, ok_out, n, false, true);
    for (const Staged* st : {&d_leaves, &d_idx, &d_sib, &d_cap, &d_ok})
        if (st->status) return st->status;
    const size_t chunks = leaf_len <= 4 ? 0 : (leaf_len + pbn::CHUNK - 1) / pbn::CHUNK;
    ctx->begin_kernel("merkle_verify_bn128", 8.0 * n * (leaf_len + 4.0 * path_len), (double)n * (double)(chunks + path_len));
    hipLaunchKernelGGL(k_pbn_merkle_verify, dim3((unsigned)((n + 15) / 16)), dim3(64), 0, ctx->stream, d_leaves.as<uint64_t>(), (uint32_t)n,
                       (uint32_t)leaf_len, d_idx.as<uint64_t>(), d_sib.as<uint64_t>(), path_len, d_cap.as<uint64_t>(), d_ok.as<uint8_t>());
    ctx->end_kernel();
    NLX_HIP(ctx, hipGetLastError());
    const int32_t rc = d_ok.finish();
    if (rc) return rc;
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NLX_OK;
} NLX_CATCH(ctx)

}  // extern "C"
