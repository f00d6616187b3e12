// Fixed-base batch scalar multiplication over BN254: out[i] = k_i * base for a
// vector of scalars - the one primitive a Groth16 setup, a KZG SRS [tau^i]_1 and every honest test key are made of.  Neither
// the bucket MSM (one sum of many points) nor nlx_bn254_g1_multiples (consecutive multiples: one addition each).
//
//   k_fb_table   table[j][d - 1] = d * 2^(8 j) * base for d = 1 .. 255, j < 32, affine, in the MSM's packed form: 8 160 entries,
//                510 KiB for G1 and 1 020 KiB for G2 - resident in L2 while the main kernel gathers from it.  Lane (j, c) doubles
//                the base 8 j times, reaches (32 c + 1) 2^(8 j) base by double-and-add and walks its 32 digits by Jacobian
//                additions; one inversion per lane (Montgomery's trick over the lane's entries) takes them to affine.  No entry
//                is the point at infinity: d 2^(8 j) < 2^256 is no multiple of the prime r > 2^253, and the base has order r
//                (G2: checked).
//   k_fb_run     lane t takes scalars t, t + L, t + 2 L, .. (L lanes in all: neighbouring lanes read and write neighbouring
//                elements): per scalar the canonical integer's 32 digits, one mixed addition (bn254_curve29.hpp's
//                jmadd29_common, the accumulator in registers) per non-zero digit, the Jacobian result and the running product of
//                the Z's to scratch in HBM; then ONE inversion per lane and the walk back to affine Montgomery words.  The partial
//                sum below window j is smaller than any d 2^(8 j) and the whole scalar is below r, so the addition never meets its
//                own point or its negative - the rare cases are handled all the same.  A scalar of 0 leaves Z exactly zero: it
//                stays out of the product and gives the all-zero words.
// Bound: integer VALU, as the bucket kernel: 32 x (7 M + 4 S) per scalar and ~12 products for the way back to affine, against
// ~380 for the lane's inversion, which a lane shares among its scalars.
#include <cstring>
#include <vector>
#include "bn254_curve29.hpp"
#include "bn254_fixed_base.hpp"
#include "bn254_fp.hpp"
#include "bn254_pairing.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace fixed_base {

using namespace msm;
typedef bnf::Fp<bnf::RP> Fr;

constexpr int TB_CHUNK = 32;                                            // table digits per lane
constexpr int TB_CHUNKS = (N_DIGITS + TB_CHUNK - 1) / TB_CHUNK;
constexpr int TABLE_ENTRIES = N_WINDOWS * N_DIGITS;
constexpr size_t RUN_SLAB = (size_t)1 << 22;                            // scalars per launch: bounds the Jacobian scratch
constexpr size_t RUN_MIN_PER_LANE = 8, RUN_MAX_LANES = (size_t)1 << 18;
static_assert(WINDOW_BITS >= 2 && WINDOW_BITS <= 16, "a digit is shifted out of the low limb");

template <class F> __device__ __forceinline__ typename F::T finv(const typename F::T& a);
template <> __device__ __forceinline__ Fe finv<F1>(const Fe& a) { return pairing::fq_inv(F1::tighten(a)); }
template <> __device__ __forceinline__ f29::Fe2 finv<F2>(const f29::Fe2& a) { return pairing::f2_inv(a); }
// a coordinate as gnark-crypto's words (Montgomery, R = 2^256)
__device__ __forceinline__ void store_coord(const Fe& a, uint64_t* w) { pairing::fq_store(a, true, w); }
__device__ __forceinline__ void store_coord(const f29::Fe2& a, uint64_t* w) {
    pairing::fq_store(a.c0, true, w);
    pairing::fq_store(a.c1, true, w + 4);
}

template <class F>
__device__ __forceinline__ void fb_table(PackedT<F> base_packed, JacT<F>* __restrict__ jac /* [TABLE_ENTRIES] */,
                                         typename F::T* __restrict__ prefix /* [TABLE_ENTRIES] */, PackedT<F>* __restrict__ table) {
    typedef typename F::T T;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)(N_WINDOWS * TB_CHUNKS)) return;
    const uint32_t j = t / TB_CHUNKS, c = t % TB_CHUNKS;
    const uint32_t d0 = c * TB_CHUNK + 1, d1 = d0 + TB_CHUNK <= (uint32_t)N_DIGITS + 1 ? d0 + TB_CHUNK : (uint32_t)N_DIGITS + 1;   // [d0, d1)
    const AffT<F> b = unpack(base_packed);
    JacT<F> p{b.x, b.y, F::one()};
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)WINDOW_BITS * j; k++) p = jdbl29(p);
    JacT<F> acc = inf29<F>();
#pragma unroll 1
    for (int bit = WINDOW_BITS - 1; bit >= 0; bit--) {   // d0 * p
        acc = jdbl29(acc);
        if ((d0 >> bit) & 1) acc = jadd29(acc, p);
    }
    T run = F::one();
    const size_t at = (size_t)j * N_DIGITS - 1;           // entry of digit d: at + d
#pragma unroll 1
    for (uint32_t d = d0; d < d1; d++) {
        if (d != d0) acc = jadd29(acc, p);
        jac[at + d] = acc;
        prefix[at + d] = run;
        run = F::mul(run, acc.z);
    }
    T inv = finv<F>(run);
#pragma unroll 1
    for (uint32_t d = d1; d-- > d0;) {
        const JacT<F> q = jac[at + d];
        const T zi = F::mul(inv, prefix[at + d]);
        inv = F::mul(inv, q.z);
        const T zi2 = F::sqr(zi);
        PackedT<F> o;
        F::to_words(F::mul(q.x, zi2), o.x);
        F::to_words(F::mul(q.y, F::mul(zi2, zi)), o.y);
        table[at + d] = o;
    }
}
__global__ __launch_bounds__(64) void k_fb_table_g1(PackedT<F1> base, JacT<F1>* __restrict__ jac, Fe* __restrict__ prefix, PackedT<F1>* __restrict__ table) {
    fb_table<F1>(base, jac, prefix, table);
}
__global__ __launch_bounds__(64) void k_fb_table_g2(PackedT<F2> base, JacT<F2>* __restrict__ jac, f29::Fe2* __restrict__ prefix, PackedT<F2>* __restrict__ table) {
    fb_table<F2>(base, jac, prefix, table);
}

__global__ __launch_bounds__(256) void k_fb_check_scalars(const uint64_t* __restrict__ scalars, size_t n, uint32_t* __restrict__ first_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !bnf::below_mod<bnf::RP>(scalars + 4 * i)) atomicMin(first_bad, (uint32_t)i);
}

template <class F>
__device__ __forceinline__ void fb_run(const PackedT<F>* __restrict__ table, const uint64_t* __restrict__ scalars, size_t n, int montgomery,
                                       JacT<F>* __restrict__ jac /* [n] */, typename F::T* __restrict__ prefix /* [n] */, uint64_t* __restrict__ out) {
    typedef typename F::T T;
    constexpr int OUT_WORDS = F::WORDS;       // 64-bit words per point: two coordinates of WORDS / 2 each
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (size_t)gridDim.x * blockDim.x;
    if (t >= n) return;
    T run = F::one();
#pragma unroll 1
    for (size_t i = t; i < n; i += lanes) {
        Fr s = bnf::load<bnf::RP>(scalars, i);
        if (montgomery) s = bnf::from_mont(s);
        JacT<F> acc = inf29<F>();
#pragma unroll 1
        for (int j = 0; j < N_WINDOWS; j++) {
            const uint32_t d = s.v[0] & (uint32_t)N_DIGITS;
#pragma unroll
            for (int l = 0; l < 7; l++) s.v[l] = (s.v[l] >> WINDOW_BITS) | (s.v[l + 1] << (32 - WINDOW_BITS));   // static indices: no scratch
            s.v[7] >>= WINDOW_BITS;
            if (d == 0) continue;
            const AffT<F> q = unpack(table[(size_t)j * N_DIGITS + d - 1]);
            if (F::is_zero_exact(acc.z)) {
                acc = JacT<F>{q.x, q.y, F::one()};
                continue;
            }
            const int st = jmadd29_common(acc, q);
            if (st == 1) acc = jdbl29(JacT<F>{q.x, q.y, F::one()});
            else if (st == 2) acc = inf29<F>();
        }
        jac[i] = acc;
        prefix[i] = run;
        if (!F::is_zero_exact(acc.z)) run = F::mul(run, acc.z);
    }
    T inv = finv<F>(run);
#pragma unroll 1
    for (size_t c = (n - 1 - t) / lanes + 1; c-- > 0;) {
        const size_t i = t + c * lanes;
        uint64_t* w = out + (size_t)OUT_WORDS * i;
        const JacT<F> p = jac[i];
        if (F::is_zero_exact(p.z)) {
#pragma unroll
            for (int k = 0; k < OUT_WORDS; k++) w[k] = 0;
            continue;
        }
        const T zi = F::mul(inv, prefix[i]);
        inv = F::mul(inv, p.z);
        const T zi2 = F::sqr(zi);
        store_coord(F::mul(p.x, zi2), w);
        store_coord(F::mul(p.y, F::mul(zi2, zi)), w + OUT_WORDS / 2);
    }
}
__global__ __launch_bounds__(64) void k_fb_run_g1(const PackedT<F1>* __restrict__ table, const uint64_t* __restrict__ scalars, size_t n, int montgomery,
                                                  JacT<F1>* __restrict__ jac, Fe* __restrict__ prefix, uint64_t* __restrict__ out) {
    fb_run<F1>(table, scalars, n, montgomery, jac, prefix, out);
}
__global__ __launch_bounds__(64) void k_fb_run_g2(const PackedT<F2>* __restrict__ table, const uint64_t* __restrict__ scalars, size_t n, int montgomery,
                                                  JacT<F2>* __restrict__ jac, f29::Fe2* __restrict__ prefix, uint64_t* __restrict__ out) {
    fb_run<F2>(table, scalars, n, montgomery, jac, prefix, out);
}

size_t table_bytes(int g2) { return (size_t)TABLE_ENTRIES * (g2 ? sizeof(PackedT<F2>) : sizeof(PackedT<F1>)); }

int32_t check_base(nlx_ctx* ctx, const uint64_t* base, int g2) {
    if (pairing::words_zero(base, g2 ? 16 : 8)) return ctx->fail(NLX_E_INVAL, "the base is the point at infinity");
    const uint32_t st = g2 ? pairing::check_g2(base) : pairing::check_g1(base);
    if (st == pairing::G1_RANGE || st == pairing::G2_RANGE) return ctx->fail(NLX_E_RANGE, "the base has a coordinate that is not below q");
    if (st == pairing::G1_OFF_CURVE || st == pairing::G2_OFF_CURVE) return ctx->fail(NLX_E_RANGE, "the base is not on the curve");
    if (st != pairing::POINT_OK) return ctx->fail(NLX_E_RANGE, "the base is not in the subgroup of order r");
    return NLX_OK;
}

// the base's words -> the packed form, on the host (F::from_mont256 is the conversion kernel's own arithmetic)
template <class F>
static PackedT<F> pack_base(const uint64_t* base) {
    uint32_t w[2 * F::WORDS];
    for (int k = 0; k < F::WORDS; k++) {
        w[2 * k] = (uint32_t)base[k];
        w[2 * k + 1] = (uint32_t)(base[k] >> 32);
    }
    PackedT<F> p;
    F::to_words(F::from_mont256(w), p.x);
    F::to_words(F::from_mont256(w + F::WORDS), p.y);
    return p;
}

int32_t build_table(nlx_ctx* ctx, Scratch& scratch, const uint64_t* base, int g2, void* d_table) {
    NLX_RC(check_base(ctx, base, g2));
    void* d_jac = scratch.alloc((size_t)TABLE_ENTRIES * (g2 ? sizeof(JacT<F2>) : sizeof(JacT<F1>)));
    void* d_prefix = scratch.alloc((size_t)TABLE_ENTRIES * (g2 ? sizeof(f29::Fe2) : sizeof(Fe)));
    if (!d_jac || !d_prefix) return ctx->fail(NLX_E_NOMEM, "fixed-base table: device memory");
    constexpr unsigned blocks = (N_WINDOWS * TB_CHUNKS + 63) / 64;
    ctx->begin_kernel("bn254_fixed_base_table", (double)table_bytes(g2), (double)TABLE_ENTRIES);
    if (g2) hipLaunchKernelGGL(k_fb_table_g2, dim3(blocks), dim3(64), 0, ctx->stream, pack_base<F2>(base), (JacT<F2>*)d_jac, (f29::Fe2*)d_prefix, (PackedT<F2>*)d_table);
    else hipLaunchKernelGGL(k_fb_table_g1, dim3(blocks), dim3(64), 0, ctx->stream, pack_base<F1>(base), (JacT<F1>*)d_jac, (Fe*)d_prefix, (PackedT<F1>*)d_table);
    ctx->end_kernel();
    return NLX_OK;
}

void check_scalars(nlx_ctx* ctx, const uint64_t* d_scalars, size_t n, uint32_t* d_first_bad) {
    if (n) hipLaunchKernelGGL(k_fb_check_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_scalars, n, d_first_bad);
}

int32_t run(nlx_ctx* ctx, Scratch& scratch, const void* d_table, const uint64_t* d_scalars, size_t n, int montgomery, int g2, uint64_t* d_out) {
    if (!n) return NLX_OK;
    const size_t slab = n < RUN_SLAB ? n : RUN_SLAB;
    void* d_jac = scratch.alloc(slab * (g2 ? sizeof(JacT<F2>) : sizeof(JacT<F1>)));
    void* d_prefix = scratch.alloc(slab * (g2 ? sizeof(f29::Fe2) : sizeof(Fe)));
    if (!d_jac || !d_prefix) return ctx->fail(NLX_E_NOMEM, "fixed-base multiples of %zu scalars: device memory", n);
    ctx->begin_kernel(g2 ? "bn254_fixed_base_g2" : "bn254_fixed_base_g1", (32.0 + (g2 ? 128.0 : 64.0)) * (double)n, (double)n);
    for (size_t first = 0; first < n; first += slab) {   // the stream runs the slabs in order on the same scratch
        const size_t m = n - first < slab ? n - first : slab;
        size_t lanes = (m + RUN_MIN_PER_LANE - 1) / RUN_MIN_PER_LANE;
        if (lanes > RUN_MAX_LANES) lanes = RUN_MAX_LANES;
        const unsigned blocks = (unsigned)((lanes + 63) / 64);
        if (g2) hipLaunchKernelGGL(k_fb_run_g2, dim3(blocks), dim3(64), 0, ctx->stream, (const PackedT<F2>*)d_table, d_scalars + 4 * first, m, montgomery,
                                   (JacT<F2>*)d_jac, (f29::Fe2*)d_prefix, d_out + 16 * first);
        else hipLaunchKernelGGL(k_fb_run_g1, dim3(blocks), dim3(64), 0, ctx->stream, (const PackedT<F1>*)d_table, d_scalars + 4 * first, m, montgomery,
                                (JacT<F1>*)d_jac, (Fe*)d_prefix, d_out + 8 * first);
    }
    ctx->end_kernel();
    return NLX_OK;
}

}  // namespace fixed_base
}  // namespace nlx

using namespace nlx;

namespace {

int32_t scalar_muls_body(nlx_ctx* ctx, Scratch& scratch, const uint64_t* base, const uint64_t* scalars, uint64_t n, uint32_t flags, int g2, uint64_t* out) {
    Staged ss(ctx, scalars, (size_t)n * 32, true, false);
    if (ss.status) return ss.status;
    uint32_t* d_bad = scratch.alloc_as<uint32_t>(64);
    void* d_table = scratch.alloc(fixed_base::table_bytes(g2));
    if (!d_bad || !d_table) return ctx->fail(NLX_E_NOMEM, "fixed-base multiples: device memory");
    uint32_t first_bad = 0xFFFFFFFFu;
    NLX_HIP(ctx, hipMemcpyAsync(d_bad, &first_bad, 4, hipMemcpyHostToDevice, ctx->stream));
    fixed_base::check_scalars(ctx, ss.as<uint64_t>(), (size_t)n, d_bad);
    NLX_RC(fetch(ctx, &first_bad, d_bad, 4));
    if (first_bad != 0xFFFFFFFFu) return ctx->fail(NLX_E_RANGE, "scalar %u is not below r", first_bad);
    Staged so(ctx, out, (size_t)n * (g2 ? 128 : 64), false, true);
    if (so.status) return so.status;
    NLX_RC(fixed_base::build_table(ctx, scratch, base, g2, d_table));
    NLX_RC(fixed_base::run(ctx, scratch, d_table, ss.as<uint64_t>(), (size_t)n, (flags & NLX_BN254_MONTGOMERY) ? 1 : 0, g2, so.as<uint64_t>()));
    NLX_RC(so.finish());
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the copy-out is done before `so` gives its block back
    return NLX_OK;
}

int32_t scalar_muls(nlx_ctx* ctx, const uint64_t* base, const uint64_t* scalars, uint64_t n, uint32_t flags, int g2, uint64_t* out) {
    if (!ctx) return NLX_E_INVAL;
    if (!base || (n && (!scalars || !out))) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (flags & ~(uint32_t)NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "unknown flag");
    if (n > fixed_base::MAX_SCALARS) return ctx->fail(NLX_E_RANGE, "at most 2^27 scalars per call");
    (void)hipSetDevice(ctx->device);
    if (is_device_ptr(base)) return ctx->fail(NLX_E_INVAL, "the base is a host value");
    NLX_RC(fixed_base::check_base(ctx, base, g2));
    if (n == 0) return NLX_OK;
    Scratch scratch(ctx);
    return scratch.finish(scalar_muls_body(ctx, scratch, base, scalars, n, flags, g2, out));
}

}  // namespace

extern "C" int32_t nlx_bn254_g1_scalar_muls(nlx_ctx* ctx, const uint64_t base[8], const uint64_t* scalars, uint64_t n, uint32_t flags,
                                            uint64_t* out) NLX_TRY {
    return scalar_muls(ctx, base, scalars, n, flags, 0, out);
} NLX_CATCH(ctx)
extern "C" int32_t nlx_bn254_g2_scalar_muls(nlx_ctx* ctx, const uint64_t base[16], const uint64_t* scalars, uint64_t n, uint32_t flags,
                                            uint64_t* out) NLX_TRY {
    return scalar_muls(ctx, base, scalars, n, flags, 1, out);
} NLX_CATCH(ctx)
