// Row f.4, the Groth16 half: gnark's groth16.Setup(r1cs) from a trapdoor, on the device - R1CS in,
// gnark's ProvingKey arrays and what nlx_bn254_groth16_vk_desc needs out, resident; nlx_bn254_groth16_setup_key builds the
// resident proving key from them through nlx_bn254_groth16_key_create[_committed].
//
// The rules are rule 3 of tools/groth16_model.py and rule 1 of tools/groth16_commit_model.py, the places of record: RECALLED from
// gnark v0.9 (backend/groth16/bn254 setup.go), UNPINNED - there is no Go source and no gnark-produced vector to compare with
// (DESIGN.md sections 19 and 22).
//
// The scalar side, Fr in Montgomery form on bn254_fp.hpp's eight 32-bit limbs:
//   k_g16s_lagrange      L_j(tau) = w^j Z_H(tau) / (n (tau - w^j)), j < n.  Lane t takes j = t, t + L, ..: the denominators and
//                        the running products forward, ONE inversion per lane (a^(r - 2)), the walk back (Montgomery's trick).
//                        tau^n != 1 is checked on the host first: no denominator is zero.
//   hipcub radix sort    per matrix, the terms' (wire id, term index) pairs by wire id: the column order (Fr has no atomic add);
//   k_g16s_ranges        reads every wire's first and last position off the sorted keys; k_g16s_term_rows finds every term's row
//                        in the row pointers (a binary search per term: no row is walked by one lane);
//   k_g16s_wire_sums     A_i(tau) (B_i, C_i) = sum over the wire's terms of coeff * L_row: a lane per wire of at most 64 terms,
//   k_g16s_long_wires    a wave per wire above that (wire 0, ONE, can sit in nearly every row), joined by shuffles;
//   k_g16s_masks         InfinityA[i] = (A_i(tau) == 0), InfinityB likewise: absent from the matrix or cancelled, the same;
//   k_g16s_gather / k_g16s_k / k_g16s_z   the scalars of every key array, in the arrays' order, through index lists the host
//                        makes from the masks (which the key's creation needs on the host anyway) and the committed sets.
// The group side: ONE fixed-base launch over all G1 scalars and one over the G2 scalars (bn254_fixed_base.hip), on one table
// each.  Both results stay in one device block per group; an array of the key is a slice.
#include <hipcub/hipcub.hpp>
#include <cstring>
#include <memory>
#include <vector>
#include "bn254_fixed_base.hpp"
#include "bn254_fp.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace g16s {

using namespace bnf;
typedef Fp<RP> Fr;

constexpr uint32_t LONG_WIRE = 64;      // wires with more terms than this go one per wave
constexpr size_t INV_CHUNK = 32;        // Lagrange values per lane: one inversion (~380 products) among them

__device__ __forceinline__ Fr fr_inv(const Fr& a) {   // a^(r - 2), a != 0
    Fr r = one<RP>();
#pragma unroll 1
    for (int bit = 253; bit >= 0; bit--) {
        r = sqr(r);
        const uint32_t word = RP::mod(bit >> 5) - ((bit >> 5) == 0 ? 2u : 0u);   // r ends in ...1: no borrow
        if ((word >> (bit & 31)) & 1) r = mul(r, a);
    }
    return r;
}
__device__ __forceinline__ Fr fr_pow(Fr b, uint64_t e) {
    Fr r = one<RP>();
#pragma unroll 1
    for (; e; e >>= 1) {
        if (e & 1) r = mul(r, b);
        b = sqr(b);
    }
    return r;
}

struct LagrangeParams {
    Fr tau, w, w_step, w_step_inv, scale;   // w: the domain's generator; w_step = w^lanes; scale = Z_H(tau) / n
    uint64_t n, lanes;
};
__global__ __launch_bounds__(256) void k_g16s_lagrange(LagrangeParams p, uint64_t* __restrict__ prefix /* [n][4] */, uint64_t* __restrict__ lag /* [n][4] */) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.lanes) return;
    Fr x = fr_pow(p.w, t), run = one<RP>();
    uint64_t count = 0;
#pragma unroll 1
    for (uint64_t j = t; j < p.n; j += p.lanes, count++) {
        const Fr den = sub(p.tau, x);
        store(prefix, j, run);
        store(lag, j, den);
        run = mul(run, den);
        x = mul(x, p.w_step);
    }
    Fr inv = fr_inv(run);
#pragma unroll 1
    for (uint64_t c = count; c-- > 0;) {
        const uint64_t j = t + c * p.lanes;
        x = mul(x, p.w_step_inv);                     // w^j again
        const Fr den = load<RP>(lag, j), dinv = mul(inv, load<RP>(prefix, j));
        inv = mul(inv, den);
        store(lag, j, mul(mul(x, p.scale), dinv));
    }
}

__global__ __launch_bounds__(256) void k_g16s_iota(uint32_t* __restrict__ v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}
// position p opens wire key[p]'s range if it differs from its left neighbour and closes it if it differs from its right one
// (wires without a term keep lo = hi = 0)
__global__ __launch_bounds__(256) void k_g16s_ranges(const uint32_t* __restrict__ sorted_keys, size_t n, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = sorted_keys[p];
    if (p == 0 || sorted_keys[p - 1] != k) lo[k] = (uint32_t)p;
    if (p + 1 == n || sorted_keys[p + 1] != k) hi[k] = (uint32_t)p + 1;
}
// the row of term k: the last row whose pointer is <= k (empty rows repeat a pointer: the LAST of them owns the term)
__global__ __launch_bounds__(256) void k_g16s_term_rows(const uint32_t* __restrict__ row_ptr, uint32_t n_rows, size_t nnz, uint32_t* __restrict__ term_row) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    uint32_t lo = 0, hi = n_rows;   // row_ptr[lo] <= k < row_ptr[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= (uint32_t)k) lo = mid;
        else hi = mid;
    }
    term_row[k] = lo;
}

struct Column {
    const uint32_t *lo, *hi;        // [n_wires] positions in `terms`
    const uint32_t* terms;          // [nnz] term indices sorted by wire id
    const uint32_t* term_row;       // [nnz]
    const uint32_t* coeff_id;       // [nnz]
    const uint64_t* coeffs;         // [n_coeffs][4]
    const uint64_t* lag;            // [n][4]
};
__device__ __forceinline__ Fr column_term(const Column& c, uint32_t p, const Fr& acc) {
    const uint32_t k = c.terms[p];
    return add(acc, mul(load<RP>(c.coeffs, c.coeff_id[k]), load<RP>(c.lag, c.term_row[k])));
}
__global__ __launch_bounds__(256) void k_g16s_wire_sums(Column c, size_t n_wires, uint64_t* __restrict__ out /* [n_wires][4] */) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    const uint32_t lo = c.lo[i], hi = c.hi[i];
    if (hi - lo > LONG_WIRE) return;   // the other kernel's
    Fr acc = zero<RP>();
#pragma unroll 1
    for (uint32_t p = lo; p < hi; p++) acc = column_term(c, p, acc);
    store(out, i, acc);
}
__global__ __launch_bounds__(256) void k_g16s_long_wires(Column c, const uint32_t* __restrict__ long_wires, uint32_t n_long, uint64_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (j >= n_long) return;   // whole waves leave together
    const uint32_t i = long_wires[j];
    const uint32_t lo = c.lo[i], hi = c.hi[i];
    Fr acc = zero<RP>();
#pragma unroll 1
    for (uint32_t p = lo + lane; p < hi; p += 64) acc = column_term(c, p, acc);
#pragma unroll 1
    for (int d = 32; d > 0; d >>= 1) {
        Fr o;
#pragma unroll
        for (int l = 0; l < 8; l++) o.v[l] = (uint32_t)__shfl_down((int)acc.v[l], d, 64);
        acc = add(acc, o);
    }
    if (lane == 0) store(out, i, acc);
}

__global__ __launch_bounds__(256) void k_g16s_masks(const uint64_t* __restrict__ at, const uint64_t* __restrict__ bt, size_t n_wires, uint8_t* __restrict__ masks /* [2][n_wires] */) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    masks[i] = is_zero(load<RP>(at, i)) ? 1 : 0;
    masks[n_wires + i] = is_zero(load<RP>(bt, i)) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_g16s_gather(const uint32_t* __restrict__ src, size_t count, const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < count) store(out, p, load<RP>(in, src[p]));
}
// out[p] = (beta A_i + alpha B_i + C_i) factor for i = src[p]
struct KParams {
    Fr alpha, beta, factor;
};
__global__ __launch_bounds__(256) void k_g16s_k(const uint32_t* __restrict__ src, size_t count, const uint64_t* __restrict__ at, const uint64_t* __restrict__ bt,
                                                const uint64_t* __restrict__ ct, KParams p, uint64_t* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t i = src[t];
    const Fr v = add(add(mul(p.beta, load<RP>(at, i)), mul(p.alpha, load<RP>(bt, i))), load<RP>(ct, i));
    store(out, t, mul(v, p.factor));
}
// out[i] = tau^i factor, i < count
__global__ __launch_bounds__(256) void k_g16s_z(Fr tau, Fr factor, size_t count, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) store(out, i, mul(fr_pow(tau, i), factor));
}

}  // namespace g16s
}  // namespace nlx

using namespace nlx;
using g16s::Fr;

// The result.  g1: [A | B | K | Z | alpha beta delta | Basis | BasisExpSigma | IC], g2: [B | beta delta gamma | (k > 0: [1]_2
// [-sigma]_2)] - gnark-crypto's words, each a device block of the context.
struct nlx_bn254_groth16_setup {
    nlx_ctx* ctx = nullptr;
    uint32_t log_n = 0, k = 0;
    uint64_t n_wires = 0, n_public = 0, n_constraints = 0;
    uint64_t n_a = 0, n_b = 0, n_k = 0, n_z = 0, m = 0, n_ic = 0, n_wave_wires = 0;
    uint64_t *g1 = nullptr, *g2 = nullptr;
    uint64_t n_g1 = 0, n_g2 = 0;
    uint64_t o_a = 0, o_b = 0, o_k = 0, o_z = 0, o_single = 0, o_basis = 0, o_basis_sigma = 0, o_ic = 0;   // in points
    std::vector<uint8_t> mask_a, mask_b;
    // the caller's R1CS and committed sets, kept on the host for the key's creation
    std::vector<uint64_t> row_ptr[3], coeffs, counts;
    std::vector<uint32_t> wire[3], coeff_id[3], ids, commitment_wires;
    std::vector<uint8_t> committed;   // per wire: 1 committed, 2 a commitment's wire
    Fr tau, alpha, beta, gamma, delta, sigma;
    // what queued copies read until the call's last synchronise
    std::vector<uint32_t> row_ptr32[3], long_wires[3], src_a, src_b, src_k, src_ic;
    std::vector<uint64_t> singles1, singles2;
};
typedef struct nlx_bn254_groth16_setup Setup;   // the plain name is the entry point's

namespace {

template <class T>
int32_t to_host(nlx_ctx* ctx, const T* p, size_t count, std::vector<T>& out) {
    out.resize(count);
    if (!count) return NLX_OK;
    NLX_HIP(ctx, hipMemcpy(out.data(), p, count * sizeof(T), hipMemcpyDefault));
    return NLX_OK;
}

void setup_free(Setup* s) {
    if (!s) return;
    if (s->ctx) {
        (void)hipStreamSynchronize(s->ctx->stream);
        if (s->g1) s->ctx->release(s->g1);
        if (s->g2) s->ctx->release(s->g2);
    }
    delete s;
}

int32_t trapdoor_value(nlx_ctx* ctx, const char* name, const uint64_t* w, Fr* out) {
    if (!w) return ctx->fail(NLX_E_INVAL, "NULL argument (%s)", name);
    if (is_device_ptr(w)) return ctx->fail(NLX_E_INVAL, "%s is a host value", name);
    if (!bnf::below_mod<bnf::RP>(w)) return ctx->fail(NLX_E_RANGE, "the trapdoor's %s is not below r", name);
    *out = bnf::load_words<bnf::RP>(w);
    if (bnf::is_zero(*out)) return ctx->fail(NLX_E_RANGE, "the trapdoor's %s is zero", name);
    return NLX_OK;
}

// every refusal, on the host, before anything is allocated on the device; fills the result's host side
int32_t load_and_check(nlx_ctx* ctx, const nlx_bn254_groth16_setup_desc* d, Setup& s) {
    if (d->flags != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "flags must be NLX_BN254_MONTGOMERY");
    if (d->log_n < 1 || d->log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n must be in [1, 26]");
    const uint64_t n = (uint64_t)1 << d->log_n;
    if (d->n_constraints > n) return ctx->fail(NLX_E_RANGE, "n_constraints exceeds 2^log_n");
    if (d->n_wires < 1 || d->n_wires > ((uint64_t)1 << 27) || d->n_public < 1 || d->n_public > d->n_wires)
        return ctx->fail(NLX_E_RANGE, "1 <= n_public <= n_wires <= 2^27");
    if (d->n_commitments > NLX_BN254_GROTH16_MAX_COMMITMENTS) return ctx->fail(NLX_E_RANGE, "0 .. %d commitments", NLX_BN254_GROTH16_MAX_COMMITMENTS);
    s.ctx = ctx;
    s.log_n = d->log_n, s.k = d->n_commitments;
    s.n_wires = d->n_wires, s.n_public = d->n_public, s.n_constraints = d->n_constraints;
    NLX_RC(trapdoor_value(ctx, "tau", d->tau, &s.tau));
    NLX_RC(trapdoor_value(ctx, "alpha", d->alpha, &s.alpha));
    NLX_RC(trapdoor_value(ctx, "beta", d->beta, &s.beta));
    NLX_RC(trapdoor_value(ctx, "gamma", d->gamma, &s.gamma));
    NLX_RC(trapdoor_value(ctx, "delta", d->delta, &s.delta));
    if (s.k) NLX_RC(trapdoor_value(ctx, "sigma", d->sigma, &s.sigma));
    if (bnf::equal(bnf::pow_host(s.tau, n), bnf::one<bnf::RP>())) return ctx->fail(NLX_E_RANGE, "tau^(2^log_n) = 1: tau lies in the domain");
    // the R1CS
    if (!d->coeffs) return ctx->fail(NLX_E_INVAL, "NULL argument (the setup needs the R1CS)");
    if (d->n_coeffs == 0 || d->n_coeffs > ((1u << 30) - 1)) return ctx->fail(NLX_E_RANGE, "the coefficient table holds 1 .. 2^30 - 1 entries");
    NLX_RC(to_host(ctx, d->coeffs, (size_t)d->n_coeffs * 4, s.coeffs));
    for (uint64_t i = 0; i < d->n_coeffs; i++)
        if (!bnf::below_mod<bnf::RP>(&s.coeffs[4 * i])) return ctx->fail(NLX_E_RANGE, "coefficient %llu is not below r", (unsigned long long)i);
    const uint64_t* rp[3] = {d->a_row_ptr, d->b_row_ptr, d->c_row_ptr};
    const uint32_t* wi[3] = {d->a_wire, d->b_wire, d->c_wire};
    const uint32_t* ci[3] = {d->a_coeff_id, d->b_coeff_id, d->c_coeff_id};
    const uint64_t nc = d->n_constraints;
    for (int m = 0; m < 3; m++) {
        if (!rp[m] || !wi[m] || !ci[m]) return ctx->fail(NLX_E_INVAL, "NULL argument (the three matrices come together)");
        NLX_RC(to_host(ctx, rp[m], (size_t)nc + 1, s.row_ptr[m]));
        const std::vector<uint64_t>& row_ptr = s.row_ptr[m];
        if (row_ptr[0] != 0) return ctx->fail(NLX_E_RANGE, "matrix %d: row pointers do not start at 0", m);
        for (uint64_t r = 0; r < nc; r++)
            if (row_ptr[r + 1] < row_ptr[r]) return ctx->fail(NLX_E_RANGE, "matrix %d: row pointers decrease at row %llu", m, (unsigned long long)r);
        const uint64_t nnz = row_ptr[nc];
        if (nnz >= ((uint64_t)1 << 31)) return ctx->fail(NLX_E_RANGE, "matrix %d: at most 2^31 - 1 terms (the sort's positions)", m);
        NLX_RC(to_host(ctx, wi[m], (size_t)nnz, s.wire[m]));
        NLX_RC(to_host(ctx, ci[m], (size_t)nnz, s.coeff_id[m]));
        std::vector<uint32_t> count((size_t)d->n_wires, 0);
        for (uint64_t k = 0; k < nnz; k++) {
            if (s.wire[m][k] >= d->n_wires) return ctx->fail(NLX_E_RANGE, "matrix %d, term %llu: wire %u of %llu", m, (unsigned long long)k, s.wire[m][k], (unsigned long long)d->n_wires);
            if (s.coeff_id[m][k] >= d->n_coeffs) return ctx->fail(NLX_E_RANGE, "matrix %d, term %llu: coefficient %u of %llu", m, (unsigned long long)k, s.coeff_id[m][k], (unsigned long long)d->n_coeffs);
            count[s.wire[m][k]]++;
        }
        for (uint64_t i = 0; i < d->n_wires; i++)
            if (count[i] > g16s::LONG_WIRE) s.long_wires[m].push_back((uint32_t)i);
        s.n_wave_wires += s.long_wires[m].size();
        s.row_ptr32[m].resize((size_t)nc + 1);
        for (uint64_t r = 0; r <= nc; r++) s.row_ptr32[m][r] = (uint32_t)row_ptr[r];
    }
    // the committed sets: nlx_bn254_groth16_key_create_committed's rules
    s.committed.assign((size_t)d->n_wires, 0);
    const uint32_t k = s.k;
    if (k) {
        if (!d->n_private || !d->commitment_wires) return ctx->fail(NLX_E_INVAL, "NULL argument");
        NLX_RC(to_host(ctx, d->n_private, (size_t)k, s.counts));
        NLX_RC(to_host(ctx, d->commitment_wires, (size_t)k, s.commitment_wires));
        for (uint32_t j = 0; j < k; j++) {
            if (s.counts[j] > d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u commits more wires than the key has", j);
            s.m += s.counts[j];
        }
        if (s.m + k > d->n_wires - d->n_public) return ctx->fail(NLX_E_RANGE, "more committed and commitment wires than private wires");
        if (s.m && !d->private_wires) return ctx->fail(NLX_E_INVAL, "NULL argument");
        NLX_RC(to_host(ctx, d->private_wires, (size_t)s.m, s.ids));
        size_t t = 0;
        for (uint32_t j = 0; j < k; j++)
            for (uint64_t i = 0; i < s.counts[j]; i++, t++) {
                const uint32_t id = s.ids[t];
                if (id < d->n_public || id >= d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u: wire %u is not a private wire", j, id);
                if (i && id <= s.ids[t - 1]) return ctx->fail(NLX_E_RANGE, "commitment %u: the committed wire ids do not ascend at %u", j, id);
                if (s.committed[id]) return ctx->fail(NLX_E_RANGE, "commitment %u: wire %u is committed twice", j, id);
                s.committed[id] = 1;
            }
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t id = s.commitment_wires[j];
            if (id < d->n_public || id >= d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u: its wire %u is not a private wire", j, id);
            if (s.committed[id]) return ctx->fail(NLX_E_RANGE, "commitment %u: its wire %u is committed or listed twice", j, id);
            s.committed[id] = 2;
        }
    }
    return NLX_OK;
}

template <class T>
int32_t upload(nlx_ctx* ctx, Scratch& scratch, const std::vector<T>& v, const T** out) {
    T* d = scratch.alloc_as<T>(v.size() * sizeof(T) + 16);
    if (!d) return ctx->fail(NLX_E_NOMEM, "Groth16 setup: device memory");
    if (!v.empty()) NLX_HIP(ctx, hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));   // v lives in the result
    *out = d;
    return NLX_OK;
}
inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

using fixed_base::G1_GEN;
using fixed_base::G2_GEN;

void push_words(std::vector<uint64_t>& v, const Fr& x) {
    uint64_t w[4];
    bnf::store_words(x, w);
    v.insert(v.end(), w, w + 4);
}

int32_t setup_body(nlx_ctx* ctx, Scratch& scratch, Setup& s) {
    using namespace nlx::g16s;
    hipStream_t st = ctx->stream;
    const uint64_t n = (uint64_t)1 << s.log_n, nw = s.n_wires;
    const Fr one_m = bnf::one<bnf::RP>();
    const Fr zh = bnf::sub(bnf::pow_host(s.tau, n), one_m);
    Fr n_m = bnf::zero<bnf::RP>();
    n_m.v[0] = (uint32_t)n;
    const Fr n_inv = bnf::inv_host(bnf::to_mont(n_m)), dinv = bnf::inv_host(s.delta), ginv = bnf::inv_host(s.gamma);
    struct Timed {   // the sample is closed on every way out
        nlx_ctx* ctx;
        bool open = true;
        void close() {
            if (open) ctx->end_kernel();
            open = false;
        }
        ~Timed() { close(); }
    } timed{ctx};
    ctx->begin_kernel("bn254_groth16_setup_scalars", 32.0 * (double)(n + 3 * nw), (double)(s.wire[0].size() + s.wire[1].size() + s.wire[2].size()));
    // L_j(tau)
    uint64_t* d_lag = scratch.alloc_as<uint64_t>(n * 32);
    uint64_t* d_prefix = scratch.alloc_as<uint64_t>(n * 32);
    uint64_t* d_abc = scratch.alloc_as<uint64_t>(3 * nw * 32);   // A_i(tau) | B_i(tau) | C_i(tau)
    uint8_t* d_masks = scratch.alloc_as<uint8_t>(2 * nw);
    if (!d_lag || !d_prefix || !d_abc || !d_masks) return ctx->fail(NLX_E_NOMEM, "Groth16 setup: device memory");
    {
        LagrangeParams p;
        p.tau = s.tau;
        p.w = bnf::pow_host(bnf::root28(), (uint64_t)1 << (28 - s.log_n));
        p.n = n;
        p.lanes = n >= INV_CHUNK ? n / INV_CHUNK : 1;
        p.w_step = bnf::pow_host(p.w, p.lanes);
        p.w_step_inv = bnf::inv_host(p.w_step);
        p.scale = bnf::mul(zh, n_inv);
        hipLaunchKernelGGL(k_g16s_lagrange, dim3(blocks_of(p.lanes)), dim3(256), 0, st, p, d_prefix, d_lag);
    }
    // the transposed products, one matrix after the other on the same scratch
    size_t max_nnz = 1;
    for (int m = 0; m < 3; m++) max_nnz = s.wire[m].size() > max_nnz ? s.wire[m].size() : max_nnz;
    int end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) < nw) end_bit++;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)max_nnz, 0, end_bit, (hipStream_t)nullptr);
    if (!tmp_bytes) tmp_bytes = 16;
    void* d_tmp = scratch.alloc(tmp_bytes);
    uint32_t* d_iota = scratch.alloc_as<uint32_t>(max_nnz * 4);
    uint32_t* d_keys = scratch.alloc_as<uint32_t>(max_nnz * 4);
    uint32_t* d_terms = scratch.alloc_as<uint32_t>(max_nnz * 4);
    uint32_t* d_term_row = scratch.alloc_as<uint32_t>(max_nnz * 4);
    uint32_t* d_lohi = scratch.alloc_as<uint32_t>(2 * nw * 4);
    const uint64_t* d_coeffs = nullptr;
    if (!d_tmp || !d_iota || !d_keys || !d_terms || !d_term_row || !d_lohi) return ctx->fail(NLX_E_NOMEM, "Groth16 setup: device memory");
    NLX_RC(upload(ctx, scratch, s.coeffs, &d_coeffs));
    hipLaunchKernelGGL(k_g16s_iota, dim3(blocks_of(max_nnz)), dim3(256), 0, st, d_iota, max_nnz);
    for (int m = 0; m < 3; m++) {
        const size_t nnz = s.wire[m].size();
        uint64_t* d_out = d_abc + (size_t)m * nw * 4;
        NLX_HIP(ctx, hipMemsetAsync(d_out, 0, nw * 32, st));
        if (!nnz) continue;
        const uint32_t *d_wire = nullptr, *d_cid = nullptr, *d_row_ptr = nullptr, *d_long = nullptr;
        NLX_RC(upload(ctx, scratch, s.wire[m], &d_wire));
        NLX_RC(upload(ctx, scratch, s.coeff_id[m], &d_cid));
        NLX_RC(upload(ctx, scratch, s.row_ptr32[m], &d_row_ptr));
        NLX_RC(upload(ctx, scratch, s.long_wires[m], &d_long));
        NLX_HIP(ctx, hipMemsetAsync(d_lohi, 0, 2 * nw * 4, st));
        size_t tb = tmp_bytes;
        NLX_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, d_wire, d_keys, d_iota, d_terms, (int)nnz, 0, end_bit, st));
        hipLaunchKernelGGL(k_g16s_ranges, dim3(blocks_of(nnz)), dim3(256), 0, st, d_keys, nnz, d_lohi, d_lohi + nw);
        hipLaunchKernelGGL(k_g16s_term_rows, dim3(blocks_of(nnz)), dim3(256), 0, st, d_row_ptr, (uint32_t)s.n_constraints, nnz, d_term_row);
        const Column c{d_lohi, d_lohi + nw, d_terms, d_term_row, d_cid, d_coeffs, d_lag};
        hipLaunchKernelGGL(k_g16s_wire_sums, dim3(blocks_of(nw)), dim3(256), 0, st, c, (size_t)nw, d_out);
        const uint32_t n_long = (uint32_t)s.long_wires[m].size();
        if (n_long) hipLaunchKernelGGL(k_g16s_long_wires, dim3((n_long + 3) / 4), dim3(256), 0, st, c, d_long, n_long, d_out);
    }
    const uint64_t *d_at = d_abc, *d_bt = d_abc + nw * 4, *d_ct = d_abc + 2 * nw * 4;
    hipLaunchKernelGGL(k_g16s_masks, dim3(blocks_of(nw)), dim3(256), 0, st, d_at, d_bt, (size_t)nw, d_masks);
    // the masks on the host: the filtered arrays' index lists
    std::vector<uint8_t> masks(2 * nw);
    NLX_RC(fetch(ctx, masks.data(), d_masks, 2 * nw));
    s.mask_a.assign(masks.begin(), masks.begin() + nw);
    s.mask_b.assign(masks.begin() + nw, masks.end());
    for (uint64_t i = 0; i < nw; i++) {
        if (!s.mask_a[i]) s.src_a.push_back((uint32_t)i);
        if (!s.mask_b[i]) s.src_b.push_back((uint32_t)i);
        if (i >= s.n_public && !s.committed[i]) s.src_k.push_back((uint32_t)i);
    }
    for (uint64_t i = 0; i < s.n_public; i++) s.src_ic.push_back((uint32_t)i);
    s.src_ic.insert(s.src_ic.end(), s.commitment_wires.begin(), s.commitment_wires.end());
    s.n_a = s.src_a.size(), s.n_b = s.src_b.size(), s.n_k = s.src_k.size(), s.n_z = n - 1, s.n_ic = s.src_ic.size();
    s.o_a = 0, s.o_b = s.n_a, s.o_k = s.o_b + s.n_b, s.o_z = s.o_k + s.n_k, s.o_single = s.o_z + s.n_z;
    s.o_basis = s.o_single + 3, s.o_basis_sigma = s.o_basis + s.m, s.o_ic = s.o_basis_sigma + s.m;
    s.n_g1 = s.o_ic + s.n_ic;
    s.n_g2 = s.n_b + 3 + (s.k ? 2 : 0);
    // the scalars, in the arrays' order
    uint64_t* d_s1 = scratch.alloc_as<uint64_t>((size_t)s.n_g1 * 32);
    uint64_t* d_s2 = scratch.alloc_as<uint64_t>((size_t)s.n_g2 * 32);
    if (!d_s1 || !d_s2) return ctx->fail(NLX_E_NOMEM, "Groth16 setup: device memory");
    const uint32_t *d_src_a = nullptr, *d_src_b = nullptr, *d_src_k = nullptr, *d_src_ic = nullptr, *d_src_basis = nullptr;
    NLX_RC(upload(ctx, scratch, s.src_a, &d_src_a));
    NLX_RC(upload(ctx, scratch, s.src_b, &d_src_b));
    NLX_RC(upload(ctx, scratch, s.src_k, &d_src_k));
    NLX_RC(upload(ctx, scratch, s.src_ic, &d_src_ic));
    NLX_RC(upload(ctx, scratch, s.ids, &d_src_basis));
    if (s.n_a) hipLaunchKernelGGL(k_g16s_gather, dim3(blocks_of(s.n_a)), dim3(256), 0, st, d_src_a, (size_t)s.n_a, d_at, d_s1 + 4 * s.o_a);
    if (s.n_b) {
        hipLaunchKernelGGL(k_g16s_gather, dim3(blocks_of(s.n_b)), dim3(256), 0, st, d_src_b, (size_t)s.n_b, d_bt, d_s1 + 4 * s.o_b);
        hipLaunchKernelGGL(k_g16s_gather, dim3(blocks_of(s.n_b)), dim3(256), 0, st, d_src_b, (size_t)s.n_b, d_bt, d_s2);
    }
    auto k_scalars = [&](const uint32_t* d_src, uint64_t count, const Fr& factor, uint64_t offset) {
        if (count) hipLaunchKernelGGL(k_g16s_k, dim3(blocks_of(count)), dim3(256), 0, st, d_src, (size_t)count, d_at, d_bt, d_ct, KParams{s.alpha, s.beta, factor}, d_s1 + 4 * offset);
    };
    k_scalars(d_src_k, s.n_k, dinv, s.o_k);
    k_scalars(d_src_basis, s.m, ginv, s.o_basis);
    if (s.k) k_scalars(d_src_basis, s.m, bnf::mul(ginv, s.sigma), s.o_basis_sigma);
    k_scalars(d_src_ic, s.n_ic, ginv, s.o_ic);
    hipLaunchKernelGGL(k_g16s_z, dim3(blocks_of(s.n_z)), dim3(256), 0, st, s.tau, bnf::mul(zh, dinv), (size_t)s.n_z, d_s1 + 4 * s.o_z);
    for (const Fr* x : {&s.alpha, &s.beta, &s.delta}) push_words(s.singles1, *x);
    for (const Fr* x : {&s.beta, &s.delta, &s.gamma}) push_words(s.singles2, *x);
    if (s.k) {
        push_words(s.singles2, one_m);
        push_words(s.singles2, bnf::neg(s.sigma));   // BasisExpSigma = sigma Basis (rule 1), so e(C, [-sigma]_2) e(Pok, [1]_2) = 1
    }
    NLX_HIP(ctx, hipMemcpyAsync(d_s1 + 4 * s.o_single, s.singles1.data(), s.singles1.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_s2 + 4 * s.n_b, s.singles2.data(), s.singles2.size() * 8, hipMemcpyHostToDevice, st));
    timed.close();
    // the group side: the result's two blocks
    s.g1 = (uint64_t*)ctx->alloc((size_t)s.n_g1 * 64);
    s.g2 = (uint64_t*)ctx->alloc((size_t)s.n_g2 * 128);
    void* d_table1 = scratch.alloc(fixed_base::table_bytes(0));
    void* d_table2 = scratch.alloc(fixed_base::table_bytes(1));
    if (!s.g1 || !s.g2 || !d_table1 || !d_table2) return ctx->fail(NLX_E_NOMEM, "Groth16 setup: device memory for %llu G1 and %llu G2 points", (unsigned long long)s.n_g1, (unsigned long long)s.n_g2);
    NLX_RC(fixed_base::build_table(ctx, scratch, G1_GEN, 0, d_table1));
    NLX_RC(fixed_base::build_table(ctx, scratch, G2_GEN, 1, d_table2));
    NLX_RC(fixed_base::run(ctx, scratch, d_table1, d_s1, (size_t)s.n_g1, 1, 0, s.g1));
    NLX_RC(fixed_base::run(ctx, scratch, d_table2, d_s2, (size_t)s.n_g2, 1, 1, s.g2));
    return NLX_OK;
}

// what the queued copies read has been read: the call's last synchronise is behind us
void drop_staging(Setup& s) {
    for (int m = 0; m < 3; m++) {
        std::vector<uint32_t>().swap(s.row_ptr32[m]);
        std::vector<uint32_t>().swap(s.long_wires[m]);
    }
    for (std::vector<uint32_t>* v : {&s.src_a, &s.src_b, &s.src_k, &s.src_ic}) std::vector<uint32_t>().swap(*v);
}

}  // namespace

extern "C" int32_t nlx_bn254_groth16_setup(nlx_ctx* ctx, const nlx_bn254_groth16_setup_desc* desc, struct nlx_bn254_groth16_setup** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<Setup, void (*)(Setup*)> s(new Setup, setup_free);
    int32_t rc = load_and_check(ctx, desc, *s);
    if (rc) {
        s->ctx = nullptr;   // nothing of the device is held: nothing to wait for
        return rc;
    }
    {
        Scratch scratch(ctx);
        rc = scratch.finish(setup_body(ctx, scratch, *s));
    }
    if (rc) return rc;   // setup_free gives the two blocks back
    drop_staging(*s);
    *out = s.release();
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_groth16_setup_destroy(struct nlx_bn254_groth16_setup* setup) NLX_TRY {
    setup_free(setup);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_groth16_setup_info(const struct nlx_bn254_groth16_setup* setup, uint64_t out[NLX_BN254_GROTH16_SETUP_INFO_WORDS]) NLX_TRY {
    if (!setup || !out) return NLX_E_INVAL;
    const uint64_t v[NLX_BN254_GROTH16_SETUP_INFO_WORDS] = {setup->n_a, setup->n_b, setup->n_k, setup->n_z, setup->m, setup->k, setup->n_ic, setup->n_wave_wires};
    memcpy(out, v, sizeof v);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" int32_t nlx_bn254_groth16_setup_read(const struct nlx_bn254_groth16_setup* setup, uint32_t which, void* out) NLX_TRY {
    if (!setup) return NLX_E_INVAL;
    nlx_ctx* ctx = setup->ctx;
    const Setup& s = *setup;
    const void* src = nullptr;
    size_t bytes = 0;
    auto g1 = [&](uint64_t offset, uint64_t count) { src = s.g1 + 8 * offset, bytes = (size_t)count * 64; };
    auto g2 = [&](uint64_t offset, uint64_t count) { src = s.g2 + 16 * offset, bytes = (size_t)count * 128; };
    switch (which) {
        case NLX_G16_SETUP_G1_A: g1(s.o_a, s.n_a); break;
        case NLX_G16_SETUP_G1_B: g1(s.o_b, s.n_b); break;
        case NLX_G16_SETUP_G2_B: g2(0, s.n_b); break;
        case NLX_G16_SETUP_G1_K: g1(s.o_k, s.n_k); break;
        case NLX_G16_SETUP_G1_Z: g1(s.o_z, s.n_z); break;
        case NLX_G16_SETUP_INFINITY_A: src = s.mask_a.data(), bytes = s.mask_a.size(); break;
        case NLX_G16_SETUP_INFINITY_B: src = s.mask_b.data(), bytes = s.mask_b.size(); break;
        case NLX_G16_SETUP_G1_ALPHA: g1(s.o_single, 1); break;
        case NLX_G16_SETUP_G1_BETA: g1(s.o_single + 1, 1); break;
        case NLX_G16_SETUP_G1_DELTA: g1(s.o_single + 2, 1); break;
        case NLX_G16_SETUP_G2_BETA: g2(s.n_b, 1); break;
        case NLX_G16_SETUP_G2_DELTA: g2(s.n_b + 1, 1); break;
        case NLX_G16_SETUP_BASIS: g1(s.o_basis, s.m); break;
        case NLX_G16_SETUP_BASIS_EXP_SIGMA: g1(s.o_basis_sigma, s.k ? s.m : 0); break;
        case NLX_G16_SETUP_G2_GAMMA: g2(s.n_b + 2, 1); break;
        case NLX_G16_SETUP_IC: g1(s.o_ic, s.n_ic); break;
        case NLX_G16_SETUP_PEDERSEN_G:
        case NLX_G16_SETUP_PEDERSEN_G_ROOT_SIGMA_NEG:
            if (!s.k) return ctx->fail(NLX_E_RANGE, "the setup carries no commitment: there is no Pedersen verifying key");
            g2(s.n_b + 3 + (which == NLX_G16_SETUP_PEDERSEN_G ? 0 : 1), 1);
            break;
        default: return ctx->fail(NLX_E_RANGE, "unknown array %u", which);
    }
    if (!bytes) return NLX_OK;
    if (!out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    (void)hipSetDevice(ctx->device);
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    NLX_HIP(ctx, hipMemcpy(out, src, bytes, hipMemcpyDefault));
    return NLX_OK;
} NLX_CATCH(setup ? setup->ctx : nullptr)

extern "C" int32_t nlx_bn254_groth16_setup_key(const struct nlx_bn254_groth16_setup* setup, nlx_bn254_groth16_key** out) NLX_TRY {
    if (!setup) return NLX_E_INVAL;
    nlx_ctx* ctx = setup->ctx;
    if (!out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    const Setup& s = *setup;
    nlx_bn254_groth16_key_desc d{};
    d.log_n = s.log_n, d.flags = NLX_BN254_MONTGOMERY;
    d.n_wires = s.n_wires, d.n_public = s.n_public, d.n_constraints = s.n_constraints;
    d.g1_a = s.g1 + 8 * s.o_a, d.n_g1_a = s.n_a;
    d.g1_b = s.g1 + 8 * s.o_b, d.n_g1_b = s.n_b;
    d.g2_b = s.g2, d.n_g2_b = s.n_b;
    d.g1_k = s.g1 + 8 * s.o_k, d.n_g1_k = s.n_k;
    d.g1_z = s.g1 + 8 * s.o_z, d.n_g1_z = s.n_z;
    d.infinity_a = s.mask_a.data(), d.infinity_b = s.mask_b.data();
    d.g1_alpha = s.g1 + 8 * s.o_single, d.g1_beta = d.g1_alpha + 8, d.g1_delta = d.g1_alpha + 16;
    d.g2_beta = s.g2 + 16 * s.n_b, d.g2_delta = d.g2_beta + 16;
    d.a_row_ptr = s.row_ptr[0].data(), d.b_row_ptr = s.row_ptr[1].data(), d.c_row_ptr = s.row_ptr[2].data();
    d.a_wire = s.wire[0].data(), d.b_wire = s.wire[1].data(), d.c_wire = s.wire[2].data();
    d.a_coeff_id = s.coeff_id[0].data(), d.b_coeff_id = s.coeff_id[1].data(), d.c_coeff_id = s.coeff_id[2].data();
    d.coeffs = s.coeffs.data(), d.n_coeffs = s.coeffs.size() / 4;
    d.n_commitments = s.k;
    if (!s.k) return nlx_bn254_groth16_key_create(ctx, &d, out);
    nlx_bn254_groth16_commit_desc cd{};
    cd.n_commitments = s.k;
    cd.n_private = s.counts.data(), cd.private_wires = s.ids.data(), cd.commitment_wires = s.commitment_wires.data();
    cd.basis = s.g1 + 8 * s.o_basis, cd.basis_exp_sigma = s.g1 + 8 * s.o_basis_sigma;
    return nlx_bn254_groth16_key_create_committed(ctx, &d, &cd, out);
} NLX_CATCH(setup ? setup->ctx : nullptr)
