// Row f.4, the PLONK half: whole gnark-shaped proofs from a proving key resident in HBM.
//
// What near-light-client_amd/bn254_plonk.py prove_gnark orchestrates in Python - gnark's backend/plonk/bn254 `Prove` restated from
// the published protocol, parity with gnark-produced bytes UNPINNED - behind two calls: a key object that converts the circuit
// once, and a prove entry that returns Proof.WriteTo's bytes.  Resident per key: the 8 + k fixed polynomials' coefficients
// (padded to n + 3, the length every polynomial of the last round is combined at), s1 s2 s3 by values on H (the grand product
// reads them), the first n + 3 SRS points in the bucket kernels' form, the 8 + k commitments, and with
// NLX_BN254_PLONK_KEY_COSET the fixed polynomials' values on the quotient's coset.  Per proof: the wires' inverse transforms, the
// blinding patches, pi2_j, the grand product, the quotient of the per-proof group, one pass that evaluates every opened
// polynomial at zeta (k_fr_eval_many), two Horner scans, and the MSMs over the resident points (bn254_msm.hpp's phases; no
// point conversion).  The host side is the SHA-256 fiat-shamir, hash_to_field and the handful of scalars of the last round.
//
// Fr here is bn254_fp.hpp's eight 32-bit limbs in Montgomery form - the element as it lies in memory.
#include <cstring>
#include <deque>
#include <vector>
#include "bn254_fp.hpp"
#include "bn254_gnark_bytes.hpp"
#include "bn254_msm.hpp"
#include "bn254_plonk.hpp"
#include "bn254_plonk_key.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace ppr {

using namespace bnf;
typedef Fp<RP> Fr;

// ---- many polynomials at one point in one pass ----
// A block of EVAL_LANES lanes covers EVAL_LANES * run consecutive coefficients of ONE polynomial.  Lane l takes the
// coefficients l, l + 256, l + 512 .. of the block's chunk - neighbouring lanes read neighbouring 32-byte elements - as a Horner
// chain in z^256, multiplies by z^l and the block sums its lanes through LDS: the chunk's value sum_j c_j z^(j - chunk start).
// The second launch is the same kernel over the per-block values with the point z^(256 run) and a run that lets one block
// cover them all.  A lane holds the accumulator, the step z^256 and a CIOS product's ten words: run = 16 keeps a chunk at 4096
// coefficients (128 KB), so a 2^20 polynomial is 257 blocks and the 5 + k polynomials of a proof fill the device several times.
constexpr uint32_t EVAL_LANES = 256, EVAL_RUN = 16, EVAL_MAX = 16;
struct EvalParams {
    const uint64_t* poly[EVAL_MAX];
    uint64_t len[EVAL_MAX];
    uint64_t* out[EVAL_MAX];       // one element per block of the polynomial
    uint32_t block0[EVAL_MAX];     // the polynomial's first block in the grid; the grid's size for unused entries
    uint64_t run;                  // coefficients per lane
    Fr z;                          // Montgomery
};
__global__ __launch_bounds__(EVAL_LANES) void k_fr_eval_many(EvalParams p) {
    __shared__ uint32_t part[8][EVAL_LANES];   // limb-major: a wave's accesses to one limb are consecutive words
    int q = 0;
#pragma unroll
    for (int i = 1; i < (int)EVAL_MAX; i++) q += blockIdx.x >= p.block0[i];   // block-uniform
    const uint32_t l = threadIdx.x;
    const uint64_t len = p.len[q], chunk = (uint64_t)EVAL_LANES * p.run, base = (uint64_t)(blockIdx.x - p.block0[q]) * chunk;
    const uint64_t end = base + chunk < len ? base + chunk : len;
    const uint64_t* __restrict__ c = p.poly[q];
    Fr zs = p.z;
#pragma unroll 1
    for (int i = 0; i < 8; i++) zs = sqr(zs);   // z^256
    Fr h = zero<RP>();
    if (base + l < end) {
        const uint64_t count = (end - base - l + EVAL_LANES - 1) / EVAL_LANES;
#pragma unroll 1
        for (uint64_t i = count; i-- > 0;) h = add(load<RP>(c, base + l + (uint64_t)EVAL_LANES * i), mul(h, zs));
        Fr zl = one<RP>(), b = p.z;   // z^l
#pragma unroll 1
        for (uint32_t e = l; e; e >>= 1) {
            if (e & 1) zl = mul(zl, b);
            b = sqr(b);
        }
        h = mul(h, zl);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) part[i][l] = h.v[i];
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = EVAL_LANES / 2; s > 0; s >>= 1) {
        if (l < s) {
            Fr o;
#pragma unroll
            for (int i = 0; i < 8; i++) o.v[i] = part[i][l + s];
            h = add(h, o);
#pragma unroll
            for (int i = 0; i < 8; i++) part[i][l] = h.v[i];
        }
        __syncthreads();
    }
    if (l == 0) store(p.out[q], blockIdx.x - p.block0[q], h);
}

// ---- blinding in coefficient form: p(X) += (b_0 + b_1 X + ..)(X^n - 1) on natural-order arrays padded to n + 3 ----
// job t = (scalar t / 2, side t % 2) of the nine scalars l l r r o o z z z; a NULL array's jobs are skipped
__global__ void k_blind_coeffs(uint64_t* pl, uint64_t* pr, uint64_t* po, uint64_t* pz, size_t n, const uint64_t* __restrict__ b) {
    const uint32_t t = threadIdx.x;
    if (t >= 18) return;
    const uint32_t j = t >> 1, add_side = t & 1;
    uint64_t* col = j < 2 ? pl : j < 4 ? pr : j < 6 ? po : pz;
    if (!col) return;
    const size_t idx = (add_side ? n : 0) + (j < 6 ? (j & 1) : j - 6);
    const Fr cur = load<RP>(col, idx), bj = load<RP>(b, j);
    store(col, idx, add_side ? add(cur, bj) : sub(cur, bj));
}

// ---- pi2_j on H: the committed L values into a zeroed column, then (a launch of its own, so that the order holds) the two
// blinding values: the commitment row first, last_row second ----
__global__ __launch_bounds__(256) void k_pi2_gather(const uint64_t* __restrict__ l, const uint32_t* __restrict__ rows, uint32_t count,
                                                    uint64_t* __restrict__ col) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t row = rows[t];
    store(col, row, load<RP>(l, row));
}
__global__ void k_pi2_blind(uint64_t* col, uint32_t commit_row, uint32_t last_row, const uint64_t* __restrict__ b2) {
    if (threadIdx.x || blockIdx.x) return;
    store(col, commit_row, load<RP>(b2, 0));
    store(col, last_row, load<RP>(b2, 1));
}

// ---- key creation: qcp is 1 on its rows (flag) and has no other non-zero entry (count) ----
__global__ __launch_bounds__(256) void k_qcp_rows(const uint64_t* __restrict__ qcp, const uint32_t* __restrict__ rows, uint32_t count,
                                                  uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count && !equal(load<RP>(qcp, rows[t]), one<RP>())) atomicOr(flag, 1u);
}
__global__ __launch_bounds__(256) void k_qcp_count(const uint64_t* __restrict__ qcp, size_t n, uint32_t* __restrict__ counter) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool nz = i < n && !is_zero(load<RP>(qcp, i));
    const unsigned long long m = __ballot(nz);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (uint32_t)__popcll(m));
}

// the host side - field helpers, bytes, fr.Hash, the transcript - is bn254_gnark_bytes.hpp

}  // namespace ppr
}  // namespace nlx

using namespace nlx;
using ppr::Fr;

// struct nlx_bn254_plonk_key: bn254_plonk_key.hpp
using namespace nlx::ppk;

// ---- the host helpers the witness checker shares (bn254_plonk_key.hpp) ----
namespace nlx {
namespace ppk {

const uint8_t BSB22_DST[] = "BSB22-Plonk";

int32_t commit(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const MsmScratch& ms, const uint64_t* d_scalars, size_t count, uint64_t out[8]) {
    using namespace nlx::msm;
    SortedDigits sd;
    int32_t rc = sort_digits(ctx, d_scalars, count, 1, &sd);
    if (rc) return rc;
    bucket_reduce(ctx, sd, key->srs, 0, ms.buckets, ms.wsum);
    std::vector<unsigned char> words(window_sum_bytes(0));
    rc = fetch(ctx, words.data(), ms.wsum, words.size());
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    release_digits(ctx, &sd);
    if (!rc) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = ctx->hip_fail(e, "kernel launch");
    }
    if (rc) return rc;
    hstore_affine<H1>(window_tail_g1(words.data()), out);
    return NLX_OK;
}
int32_t msm_scratch(nlx_ctx* ctx, Scratch& scratch, MsmScratch* ms) {
    ms->buckets = scratch.alloc(msm::bucket_bytes(0));
    ms->wsum = scratch.alloc(msm::window_sum_bytes(0));
    return ms->buckets && ms->wsum ? NLX_OK : ctx->fail(NLX_E_NOMEM, "PLONK: device memory for the MSM's buckets");
}

// pi2_j on H from the L wire into d_col (n elements), its coefficients in place
int32_t build_pi2(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, uint32_t j, const uint64_t* d_l, const uint64_t* d_b2, uint64_t* d_col) {
    const size_t n = (size_t)1 << key->log_n;
    const uint32_t count = key->seg[j + 1] - key->seg[j];
    NLX_HIP(ctx, hipMemsetAsync(d_col, 0, n * 32, ctx->stream));
    if (count) hipLaunchKernelGGL(ppr::k_pi2_gather, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, d_l, key->rows + key->seg[j], count, d_col);
    hipLaunchKernelGGL(ppr::k_pi2_blind, dim3(1), dim3(1), 0, ctx->stream, d_col, key->commit_rows[j], key->last_row, d_b2);
    return NLX_OK;
}

int32_t check_scalars(nlx_ctx* ctx, const uint64_t* w, size_t count, const char* what) {
    if (is_device_ptr(w)) return ctx->fail(NLX_E_INVAL, "%s are host values", what);
    for (size_t i = 0; i < count; i++)
        if (!bnf::below_mod<bnf::RP>(w + 4 * i)) return ctx->fail(NLX_E_RANGE, "%s: element %llu is not below r", what, (unsigned long long)i);
    return NLX_OK;
}

// round 0 for one commitment, as the prover, the solver's hint and the witness checker all take it
int32_t commit_pi2(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const MsmScratch& ms, uint32_t j, const uint64_t* d_l, const uint64_t* d_b2,
                   uint64_t* d_col, uint64_t point_out[8], uint64_t c_out[4]) {
    NLX_RC(build_pi2(ctx, key, j, d_l, d_b2, d_col));
    NLX_RC(nlx_bn254_ntt_batch(ctx, d_col, 1, key->log_n, 1, NLX_BN254_MONTGOMERY));
    NLX_RC(commit(ctx, key, ms, d_col, (size_t)1 << key->log_n, point_out));
    uint8_t bytes[64];
    ppr::g1_marshal(point_out, bytes);
    bnf::store_words(ppr::hash_to_field(bytes, 64, BSB22_DST, sizeof BSB22_DST - 1), c_out);
    return NLX_OK;
}

}  // namespace ppk
}  // namespace nlx

namespace {

// a round's device time under the library's kernel timing: the rounds are made of calls that take samples of their own, so the
// round's sample is pushed when it ends
struct RoundTimer {
    nlx_ctx* ctx;
    const char* name;
    hipEvent_t e0 = nullptr;
    RoundTimer(nlx_ctx* c, const char* n) : ctx(c), name(n) {
        if (!ctx->kernel_timing) return;
        e0 = ctx->get_event();
        (void)hipEventRecord(e0, ctx->stream);
    }
    ~RoundTimer() {
        if (!e0) return;
        hipEvent_t e1 = ctx->get_event();
        (void)hipEventRecord(e1, ctx->stream);
        ctx->samples.push_back(nlx_ctx::KernelSample{name, 0.0, 0.0, e0, e1});
    }
};

void key_free(nlx_bn254_plonk_key* key) {
    if (!key) return;
    if (key->ctx) {
        (void)hipStreamSynchronize(key->ctx->stream);
        for (void* p : key->blocks) key->ctx->release(p);
        if (key->sigma_cells) key->ctx->release(key->sigma_cells);
    }
    delete key;
}
void* key_alloc(nlx_bn254_plonk_key* key, size_t bytes) {
    void* d = key->ctx->alloc(bytes + 32);
    if (d) {
        key->blocks.push_back(d);
        key->info[0] += bytes;
    }
    return d;
}

// values of up to EVAL_MAX device polynomials at one host point -> out (host, Montgomery words)
int32_t eval_many(nlx_ctx* ctx, uint32_t n_polys, const uint64_t* const* d_polys, const uint64_t* lens, const Fr& z, uint64_t* out, Scratch& scratch) {
    ppr::EvalParams p1{}, p2{};
    const uint64_t chunk = (uint64_t)ppr::EVAL_LANES * ppr::EVAL_RUN;
    uint64_t total = 0, most = 0;
    for (uint32_t i = 0; i < n_polys; i++) {
        const uint64_t nb = (lens[i] + chunk - 1) / chunk;
        total += nb;
        most = nb > most ? nb : most;
    }
    uint64_t* d_part = scratch.alloc_as<uint64_t>((total + n_polys) * 32);
    if (!d_part) return NLX_E_NOMEM;
    uint64_t* d_vals = d_part + total * 4;
    uint64_t at = 0;
    for (uint32_t i = 0; i < ppr::EVAL_MAX; i++) {
        p1.block0[i] = (uint32_t)(i < n_polys ? at : total);
        p2.block0[i] = i < n_polys ? i : n_polys;
        if (i >= n_polys) continue;
        const uint64_t nb = (lens[i] + chunk - 1) / chunk;
        p1.poly[i] = d_polys[i], p1.len[i] = lens[i], p1.out[i] = d_part + at * 4;
        p2.poly[i] = d_part + at * 4, p2.len[i] = nb, p2.out[i] = d_vals + 4 * i;
        at += nb;
    }
    p1.run = ppr::EVAL_RUN, p1.z = z;
    p2.run = (most + ppr::EVAL_LANES - 1) / ppr::EVAL_LANES, p2.z = bnf::pow_host(z, chunk);
    ctx->begin_kernel("bn254_fr_eval_many", 0.0);
    hipLaunchKernelGGL(ppr::k_fr_eval_many, dim3((unsigned)total), dim3(ppr::EVAL_LANES), 0, ctx->stream, p1);
    hipLaunchKernelGGL(ppr::k_fr_eval_many, dim3(n_polys), dim3(ppr::EVAL_LANES), 0, ctx->stream, p2);
    ctx->end_kernel();
    return fetch(ctx, out, d_vals, (size_t)n_polys * 32);
}

template <class T>
int32_t to_host(nlx_ctx* ctx, const T* p, size_t count, std::vector<T>& out) {
    out.resize(count);
    if (!count) return NLX_OK;
    NLX_HIP(ctx, hipMemcpy(out.data(), p, count * sizeof(T), hipMemcpyDefault));
    return NLX_OK;
}

int32_t copy_in(nlx_ctx* ctx, uint64_t* d_dst, const uint64_t* src, size_t bytes) {
    NLX_HIP(ctx, hipMemcpyAsync(d_dst, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return NLX_OK;
}

int32_t key_build(nlx_ctx* ctx, const nlx_bn254_plonk_key_desc* d, nlx_bn254_plonk_key* key) {
    using namespace nlx::ppr;
    const uint32_t log_n = d->log_n, k = d->n_commit, nF = 8 + k;
    const size_t n = (size_t)1 << log_n, m = n + 3;
    hipStream_t st = ctx->stream;
    key->ctx = ctx, key->log_n = log_n, key->n_commit = k, key->coset = (d->flags & NLX_BN254_PLONK_KEY_COSET) != 0;
    memcpy(key->k1, d->k1, 32), memcpy(key->k2, d->k2, 32), memcpy(key->shift, d->coset_shift, 32);
    // the committed rows
    std::vector<uint32_t> rows;
    if (k) {
        std::vector<uint64_t> counts;
        std::vector<uint32_t> crow;
        NLX_RC(to_host(ctx, d->n_committed, (size_t)k, counts));
        NLX_RC(to_host(ctx, d->commit_rows, (size_t)k, crow));
        uint64_t total = 0;
        for (uint32_t j = 0; j < k; j++) {
            if (counts[j] > n) return ctx->fail(NLX_E_RANGE, "commitment %u commits more rows than H has", j);
            total += counts[j];
            key->seg[j + 1] = (uint32_t)total;
            if (crow[j] >= n) return ctx->fail(NLX_E_RANGE, "commitment %u: its row %u lies outside H", j, crow[j]);
            key->commit_rows[j] = crow[j];
        }
        if (total && !d->committed_rows) return ctx->fail(NLX_E_INVAL, "NULL argument (committed_rows)");
        if (d->last_row >= n) return ctx->fail(NLX_E_RANGE, "last_row %u lies outside H", d->last_row);
        key->last_row = d->last_row;
        NLX_RC(to_host(ctx, d->committed_rows, (size_t)total, rows));
        for (uint32_t j = 0; j < k; j++)
            for (uint32_t t = key->seg[j]; t < key->seg[j + 1]; t++) {
                if (rows[t] >= n) return ctx->fail(NLX_E_RANGE, "commitment %u: row %u lies outside H", j, rows[t]);
                if (t > key->seg[j] && rows[t] <= rows[t - 1]) return ctx->fail(NLX_E_RANGE, "commitment %u: the committed rows do not ascend at %u", j, rows[t]);
            }
        key->rows = (uint32_t*)key_alloc(key, rows.size() * 4 + 4);
        if (!key->rows) return NLX_E_NOMEM;
        if (!rows.empty()) NLX_HIP(ctx, hipMemcpy(key->rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        key->info[3] = total;
    }
    key->coeffs = (uint64_t*)key_alloc(key, (size_t)nF * m * 32);
    key->sigma = (uint64_t*)key_alloc(key, 3 * n * 32);
    key->srs = key_alloc(key, m * msm::converted_point_bytes(0));
    if (key->coset) key->coset_ev = (uint64_t*)key_alloc(key, (size_t)nF * 4 * n * 32);
    if (!key->coeffs || !key->sigma || !key->srs || (key->coset && !key->coset_ev)) return ctx->fail(NLX_E_NOMEM, "PLONK key: device memory");
    Scratch scratch(ctx);
    uint64_t* d_vals = scratch.alloc_as<uint64_t>((size_t)nF * n * 32);
    uint32_t* d_check = scratch.alloc_as<uint32_t>(64);
    MsmScratch ms;
    if (!d_vals || !d_check) return NLX_E_NOMEM;
    NLX_RC(msm_scratch(ctx, scratch, &ms));
    const uint64_t* src[8 + NLX_BN254_PLONK_MAX_COMMIT] = {d->ql, d->qr, d->qm, d->qo, d->qk, d->s1, d->s2, d->s3};
    for (uint32_t j = 0; j < k; j++) src[8 + j] = d->qcp[j];
    for (uint32_t i = 0; i < nF; i++) NLX_RC(copy_in(ctx, d_vals + (size_t)i * n * 4, src[i], n * 32));
    NLX_HIP(ctx, hipMemcpyAsync(key->sigma, d_vals + (size_t)S1 * n * 4, 3 * n * 32, hipMemcpyDeviceToDevice, st));
    // each selector of a commitment: 1 on its rows, and as many non-zero entries as it has rows
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t count = key->seg[j + 1] - key->seg[j];
        NLX_HIP(ctx, hipMemsetAsync(d_check, 0, 8, st));
        const uint64_t* qcp = d_vals + (size_t)(8 + j) * n * 4;
        if (count) hipLaunchKernelGGL(k_qcp_rows, dim3((count + 255) / 256), dim3(256), 0, st, qcp, key->rows + key->seg[j], count, d_check);
        hipLaunchKernelGGL(k_qcp_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, qcp, n, d_check + 1);
        uint32_t got[2];
        NLX_RC(fetch(ctx, got, d_check, 8));
        if (got[0] || got[1] != count) return ctx->fail(NLX_E_INVAL, "qcp[%u] is not 1 on the committed rows and 0 elsewhere", j);
    }
    // coefficients, padded to n + 3
    NLX_RC(nlx_bn254_ntt_batch(ctx, d_vals, nF, log_n, 1, NLX_BN254_MONTGOMERY));
    NLX_HIP(ctx, hipMemsetAsync(key->coeffs, 0, (size_t)nF * m * 32, st));
    NLX_HIP(ctx, hipMemcpy2DAsync(key->coeffs, m * 32, d_vals, n * 32, n * 32, nF, hipMemcpyDeviceToDevice, st));
    // the SRS in the bucket kernels' form
    {
        Staged sp(ctx, d->srs, m * 64, true, false);
        if (sp.status) return sp.status;
        msm::convert_points(ctx, sp.as<uint64_t>(), nullptr, m, 0, key->srs);
        NLX_HIP(ctx, hipStreamSynchronize(st));
    }
    // the commitments, in the order the transcript binds them
    const int order[8] = {S1, S2, S3, QL, QR, QM, QO, QK};
    for (uint32_t i = 0; i < nF; i++) {
        const uint32_t at = i < 8 ? (uint32_t)order[i] : i;
        NLX_RC(commit(ctx, key, ms, key->coeffs + (size_t)at * m * 4, n, key->commitments + 8 * i));
    }
    if (key->coset) {
        bnp::PolyIn polys[8 + NLX_BN254_PLONK_MAX_COMMIT];
        for (uint32_t i = 0; i < nF; i++) polys[i] = bnp::PolyIn{key->coeffs + (size_t)i * m * 4, bnp::POLY_COEFFS, n};
        NLX_RC(bnp::to_coset(ctx, log_n, polys, nF, key->shift, key->coset_ev));
    }
    key->info[1] = n, key->info[2] = k, key->info[4] = key->coset ? 1 : 0;
    return scratch.finish(NLX_OK);
}

int32_t prove_body(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o, const uint64_t* pubs,
                   uint64_t n_public, const uint64_t* blinding, const uint64_t* commit_blinding, uint8_t* proof_out, size_t* proof_len) {
    using namespace nlx::ppr;
    using namespace bnf;
    const uint32_t log_n = key->log_n, k = key->n_commit, nF = 8 + k;
    const size_t n = (size_t)1 << log_n, m = n + 3;
    const bool has_pi = n_public || k;
    hipStream_t st = ctx->stream;
    (void)hipSetDevice(ctx->device);
    Staged sl(ctx, l, n * 32, true, false), sr(ctx, r, n * 32, true, false), so(ctx, o, n * 32, true, false);
    for (const Staged* s : {&sl, &sr, &so})
        if (s->status) return s->status;
    const uint64_t* d_wire[3] = {sl.as<uint64_t>(), sr.as<uint64_t>(), so.as<uint64_t>()};
    Scratch scratch(ctx);
    MsmScratch ms;
    NLX_RC(msm_scratch(ctx, scratch, &ms));
    uint64_t* d_bl = scratch.alloc_as<uint64_t>(4 * m * 32);            // l r o z: blinded coefficients, padded to n + 3
    uint64_t* d_zv = scratch.alloc_as<uint64_t>(n * 32);                // z on H
    uint64_t* d_pi = scratch.alloc_as<uint64_t>((size_t)(1 + k) * m * 32);   // pi, pi2_j: coefficients, padded
    uint64_t* d_h = scratch.alloc_as<uint64_t>(4 * n * 32);             // the quotient's coefficients
    uint64_t* d_lin = scratch.alloc_as<uint64_t>(3 * m * 32);           // foldedH | linearised | folded batch
    uint64_t* d_q = scratch.alloc_as<uint64_t>(m * 32);                 // an opening's quotient
    uint64_t* d_small = scratch.alloc_as<uint64_t>((9 + 2 * NLX_BN254_PLONK_MAX_COMMIT) * 32);
    if (!d_bl || !d_zv || !d_pi || !d_h || !d_lin || !d_q || !d_small) return ctx->fail(NLX_E_NOMEM, "PLONK proof: device memory");
    uint64_t* d_pi2 = d_pi + m * 4;
    uint64_t* d_cb = d_small + 9 * 4;
    NLX_HIP(ctx, hipMemcpyAsync(d_small, blinding, 9 * 32, hipMemcpyHostToDevice, st));
    if (k) NLX_HIP(ctx, hipMemcpyAsync(d_cb, commit_blinding, (size_t)2 * k * 32, hipMemcpyHostToDevice, st));
    auto key_coeff = [&](uint32_t i) { return key->coeffs + (size_t)i * m * 4; };

    // round 0: the Bsb22 commitments from the finished wires, and what the circuit must hold on their rows
    uint64_t pi2c[NLX_BN254_PLONK_MAX_COMMIT][8];
    Fr cs[NLX_BN254_PLONK_MAX_COMMIT];
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_commit");
        NLX_HIP(ctx, hipMemsetAsync(d_pi, 0, (size_t)(1 + k) * m * 32, st));
        for (uint32_t j = 0; j < k; j++) {
            uint64_t* col = d_pi2 + (size_t)j * m * 4;
            uint64_t want[4], have[4];
            NLX_RC(commit_pi2(ctx, key, ms, j, d_wire[0], d_cb + 8 * j, col, pi2c[j], want));
            cs[j] = fr_words(want);
            NLX_RC(fetch(ctx, have, d_wire[0] + 4 * (size_t)key->commit_rows[j], 32));
            if (memcmp(have, want, 32))
                return ctx->fail(NLX_E_INVAL, "Bsb22 commitment %u: the L wire of its commitment row is not the hash of the commitment (or a committed value changed after the hint)", j);
        }
    }
    Challenge gamma_c("gamma", nullptr);
    for (uint32_t i = 0; i < nF; i++) gamma_c.bind_point(key->commitments + 8 * i);
    for (uint64_t i = 0; i < n_public; i++) gamma_c.bind_fr(fr_words(pubs + 4 * i));
    // round 1: the blinded wires
    uint64_t lro[3][8];
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_wires");
        NLX_HIP(ctx, hipMemsetAsync(d_bl, 0, 4 * m * 32, st));
        for (int i = 0; i < 3; i++) NLX_HIP(ctx, hipMemcpyAsync(d_bl + (size_t)i * m * 4, d_wire[i], n * 32, hipMemcpyDeviceToDevice, st));
        for (int i = 0; i < 3; i++) NLX_RC(nlx_bn254_ntt_batch(ctx, d_bl + (size_t)i * m * 4, 1, log_n, 1, NLX_BN254_MONTGOMERY));
        hipLaunchKernelGGL(k_blind_coeffs, dim3(1), dim3(64), 0, st, d_bl, d_bl + m * 4, d_bl + 2 * m * 4, (uint64_t*)nullptr, n, d_small);
        for (int i = 0; i < 3; i++) {
            NLX_RC(commit(ctx, key, ms, d_bl + (size_t)i * m * 4, n + 2, lro[i]));
            gamma_c.bind_point(lro[i]);
        }
    }
    const Fr gamma = gamma_c.value();
    Challenge beta_c("beta", &gamma_c);
    const Fr beta = beta_c.value();
    uint64_t gamma_w[4], beta_w[4], alpha_w[4];
    store_words(gamma, gamma_w), store_words(beta, beta_w);
    // round 2: the grand product, blinded
    uint64_t zc[8];
    uint64_t* d_blz = d_bl + 3 * m * 4;
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_z");
        int32_t closes = 0;
        NLX_RC(nlx_bn254_plonk_grand_product(ctx, log_n, d_wire[0], d_wire[1], d_wire[2], key->sigma, key->sigma + n * 4, key->sigma + 2 * n * 4, beta_w,
                                             gamma_w, key->k1, key->k2, d_zv, &closes));
        if (!closes) return ctx->fail(NLX_E_INVAL, "the wires do not respect the circuit's copy constraints (the grand product does not close)");
        NLX_HIP(ctx, hipMemcpyAsync(d_blz, d_zv, n * 32, hipMemcpyDeviceToDevice, st));
        NLX_RC(nlx_bn254_ntt_batch(ctx, d_blz, 1, log_n, 1, NLX_BN254_MONTGOMERY));
        hipLaunchKernelGGL(k_blind_coeffs, dim3(1), dim3(64), 0, st, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, d_blz, n, d_small);
        NLX_RC(commit(ctx, key, ms, d_blz, m, zc));
    }
    Challenge alpha_c("alpha", &beta_c);
    for (uint32_t j = 0; j < k; j++) alpha_c.bind_point(pi2c[j]);
    alpha_c.bind_point(zc);
    const Fr alpha = alpha_c.value();
    store_words(alpha, alpha_w);
    // round 3: the quotient of the blinded polynomials, cut into h1 h2 h3 of n + 2 coefficients
    uint64_t hc[3][8];
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_quotient");
        if (has_pi) {   // PI on H: the public inputs on the first rows, c_j on the commitment rows; then its coefficients
            if (n_public) NLX_HIP(ctx, hipMemcpyAsync(d_pi, pubs, n_public * 32, hipMemcpyHostToDevice, st));
            uint64_t cw[NLX_BN254_PLONK_MAX_COMMIT][4];
            for (uint32_t j = 0; j < k; j++) {
                store_words(cs[j], cw[j]);
                NLX_HIP(ctx, hipMemcpyAsync(d_pi + 4 * (size_t)key->commit_rows[j], cw[j], 32, hipMemcpyHostToDevice, st));
            }
            NLX_HIP(ctx, hipStreamSynchronize(st));   // cw leaves scope
            NLX_RC(nlx_bn254_ntt_batch(ctx, d_pi, 1, log_n, 1, NLX_BN254_MONTGOMERY));
        }
        bnp::PolyIn fixed[8 + NLX_BN254_PLONK_MAX_COMMIT], proof[5 + NLX_BN254_PLONK_MAX_COMMIT];
        for (uint32_t i = 0; i < nF; i++)
            fixed[i] = key->coset ? bnp::PolyIn{key->coset_ev + (size_t)i * 4 * n * 4, bnp::POLY_COSET, 4 * n} : bnp::PolyIn{key_coeff(i), bnp::POLY_COEFFS, n};
        uint32_t np = 0;
        for (int i = 0; i < 3; i++) proof[np++] = bnp::PolyIn{d_bl + (size_t)i * m * 4, bnp::POLY_COEFFS, n + 2};
        proof[np++] = bnp::PolyIn{d_blz, bnp::POLY_COEFFS, m};
        if (has_pi) proof[np++] = bnp::PolyIn{d_pi, bnp::POLY_COEFFS, n};
        for (uint32_t j = 0; j < k; j++) proof[np++] = bnp::PolyIn{d_pi2 + (size_t)j * m * 4, bnp::POLY_COEFFS, n};
        bnp::QuotientIn qin{log_n, has_pi ? 1u : 0u, k, fixed, proof, {key->shift, key->k1, key->k2, alpha_w, beta_w, gamma_w}, nullptr};
        int32_t high_zero = 0;
        NLX_RC(bnp::quotient_chain(ctx, qin, d_h, 3 * n + 6, 3 * n + 6, &high_zero));
        if (!high_zero) return ctx->fail(NLX_E_INVAL, "the witness does not satisfy the circuit (the quotient has more than 3 n + 6 coefficients)");
        for (int i = 0; i < 3; i++) NLX_RC(commit(ctx, key, ms, d_h + (size_t)i * (n + 2) * 4, n + 2, hc[i]));
    }
    Challenge zeta_c("zeta", &alpha_c);
    for (int i = 0; i < 3; i++) zeta_c.bind_point(hc[i]);
    const Fr zeta = zeta_c.value();
    uint64_t zeta_w[4];
    store_words(zeta, zeta_w);
    // round 4: every opened polynomial at zeta in one pass; z at w zeta with its opening
    uint64_t ev[(5 + NLX_BN254_PLONK_MAX_COMMIT) * 4], zw_w[4], zshift[8];
    Fr w_n = root28();
    for (uint32_t i = log_n; i < 28; i++) w_n = sqr(w_n);
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_evals");
        const uint64_t* polys[5 + NLX_BN254_PLONK_MAX_COMMIT] = {d_bl, d_bl + m * 4, d_bl + 2 * m * 4, key_coeff(S1), key_coeff(S2)};
        uint64_t lens[5 + NLX_BN254_PLONK_MAX_COMMIT] = {n + 2, n + 2, n + 2, n, n};
        for (uint32_t j = 0; j < k; j++) polys[5 + j] = key_coeff(8 + j), lens[5 + j] = n;
        NLX_RC(eval_many(ctx, 5 + k, polys, lens, zeta, ev, scratch));
        uint64_t zeta_shift_w[4];
        store_words(mul(zeta, w_n), zeta_shift_w);
        NLX_RC(nlx_bn254_kzg_open(ctx, d_blz, m, zeta_shift_w, nullptr, zw_w, d_q, nullptr));
        NLX_RC(commit(ctx, key, ms, d_q, m - 1, zshift));
    }
    const Fr lz = fr_words(ev), rz = fr_words(ev + 4), oz = fr_words(ev + 8), s1z = fr_words(ev + 12), s2z = fr_words(ev + 16), zw = fr_words(zw_w);
    // round 5: the linearised polynomial, foldedH, one batched opening at zeta
    const Fr k1 = fr_words(key->k1), k2 = fr_words(key->k2), one_m = one<RP>();
    const Fr zeta_n = pow_host(zeta, n), zh = sub(zeta_n, one_m);
    const Fr l1 = mul(zh, inv_host(mul(fr_small(n), sub(zeta, one_m))));
    const Fr bz = mul(beta, zeta);
    const Fr a_ = mul(mul(add(add(lz, bz), gamma), add(add(rz, mul(bz, k1)), gamma)), add(add(oz, mul(bz, k2)), gamma));
    const Fr b_ = mul(add(add(lz, mul(beta, s1z)), gamma), add(add(rz, mul(beta, s2z)), gamma));
    uint64_t* d_fh = d_lin;
    uint64_t* d_lp = d_lin + m * 4;
    uint64_t* d_fold = d_lin + 2 * m * 4;
    uint64_t claimed[(7 + NLX_BN254_PLONK_MAX_COMMIT) * 4], bh[8];
    {
        RoundTimer timer(ctx, "bn254_plonk_prove_open");
        const uint64_t* terms[7 + NLX_BN254_PLONK_MAX_COMMIT] = {key_coeff(QM), key_coeff(QL), key_coeff(QR), key_coeff(QO), key_coeff(QK), d_blz, key_coeff(S3)};
        uint64_t sc[(7 + NLX_BN254_PLONK_MAX_COMMIT) * 4];
        const Fr lin_sc[7] = {mul(lz, rz), lz, rz, oz, one_m, add(mul(alpha, a_), mul(mul(alpha, alpha), l1)), neg(mul(mul(mul(alpha, b_), beta), zw))};
        for (int i = 0; i < 7; i++) store_words(lin_sc[i], sc + 4 * i);
        for (uint32_t j = 0; j < k; j++) {
            terms[7 + j] = d_pi2 + (size_t)j * m * 4;
            memcpy(sc + 4 * (7 + j), ev + 4 * (5 + j), 32);   // qcp_j(zeta)
        }
        NLX_RC(nlx_bn254_fr_lincomb(ctx, m, 7 + k, terms, sc, d_lp));
        const Fr zn2 = mul(mul(zeta_n, zeta), zeta);
        const uint64_t* hs[3] = {d_h, d_h + (n + 2) * 4, d_h + 2 * (n + 2) * 4};
        store_words(one_m, sc), store_words(zn2, sc + 4), store_words(sqr(zn2), sc + 8);
        NLX_HIP(ctx, hipMemsetAsync(d_fh, 0, m * 32, st));
        NLX_RC(nlx_bn254_fr_lincomb(ctx, n + 2, 3, hs, sc, d_fh));
        uint64_t digests[2][8];
        NLX_RC(commit(ctx, key, ms, d_fh, n + 2, digests[0]));
        NLX_RC(commit(ctx, key, ms, d_lp, m, digests[1]));
        const uint64_t* two[2] = {d_fh, d_lp};
        const uint64_t two_len[2] = {n + 2, m};
        NLX_RC(eval_many(ctx, 2, two, two_len, zeta, claimed, scratch));
        memcpy(claimed + 8, ev, (size_t)(5 + k) * 32);
        Challenge fold_c("gamma", nullptr);
        fold_c.bind_fr(zeta);
        fold_c.bind_point(digests[0]), fold_c.bind_point(digests[1]);
        for (int i = 0; i < 3; i++) fold_c.bind_point(lro[i]);
        fold_c.bind_point(key->commitments), fold_c.bind_point(key->commitments + 8);   // [s1] [s2]
        for (uint32_t j = 0; j < k; j++) fold_c.bind_point(key->commitments + 8 * (8 + j));
        for (uint32_t i = 0; i < 7 + k; i++) fold_c.bind_fr(fr_words(claimed + 4 * i));
        const Fr gp = fold_c.value();
        const uint64_t* batch[7 + NLX_BN254_PLONK_MAX_COMMIT] = {d_fh, d_lp, d_bl, d_bl + m * 4, d_bl + 2 * m * 4, key_coeff(S1), key_coeff(S2)};
        for (uint32_t j = 0; j < k; j++) batch[7 + j] = key_coeff(8 + j);
        Fr power = one_m;
        for (uint32_t i = 0; i < 7 + k; i++, power = mul(power, gp)) store_words(power, sc + 4 * i);
        NLX_RC(nlx_bn254_fr_lincomb(ctx, m, 7 + k, batch, sc, d_fold));
        uint64_t y[4];
        NLX_RC(nlx_bn254_kzg_open(ctx, d_fold, m, zeta_w, nullptr, y, d_q, nullptr));
        NLX_RC(commit(ctx, key, ms, d_q, m - 1, bh));
    }
    NLX_RC(scratch.finish(NLX_OK));
    // Proof.WriteTo
    uint8_t* p = proof_out;
    auto point = [&](const uint64_t* w) { g1_compress(w, p), p += 32; };
    auto u32 = [&](uint32_t x) { p[0] = (uint8_t)(x >> 24), p[1] = (uint8_t)(x >> 16), p[2] = (uint8_t)(x >> 8), p[3] = (uint8_t)x, p += 4; };
    for (int i = 0; i < 3; i++) point(lro[i]);
    point(zc);
    for (int i = 0; i < 3; i++) point(hc[i]);
    u32(k);
    for (uint32_t j = 0; j < k; j++) point(pi2c[j]);
    point(bh);
    u32(7 + k);
    for (uint32_t i = 0; i < 7 + k; i++) be32(fr_words(claimed + 4 * i), p), p += 32;
    point(zshift);
    be32(zw, p), p += 32;
    *proof_len = (size_t)(p - proof_out);
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_plonk_key_create(nlx_ctx* ctx, const nlx_bn254_plonk_key_desc* d, nlx_bn254_plonk_key** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!d || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    if ((d->flags & ~NLX_BN254_PLONK_KEY_COSET) != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "flags: NLX_BN254_MONTGOMERY, optionally NLX_BN254_PLONK_KEY_COSET");
    if (d->log_n < 3 || d->log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n must be in [3, 26]");
    if (d->n_commit > NLX_BN254_PLONK_MAX_COMMIT) return ctx->fail(NLX_E_RANGE, "n_commit must be in [0, 4]");
    if (!d->ql || !d->qr || !d->qm || !d->qo || !d->qk || !d->s1 || !d->s2 || !d->s3 || !d->k1 || !d->k2 || !d->coset_shift || !d->srs)
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (d->n_commit) {
        if (!d->qcp || !d->n_committed || !d->commit_rows || is_device_ptr(d->qcp)) return ctx->fail(NLX_E_INVAL, "NULL argument (qcp is a host array of n_commit pointers)");
        for (uint32_t j = 0; j < d->n_commit; j++)
            if (!d->qcp[j]) return ctx->fail(NLX_E_INVAL, "NULL polynomial (qcp)");
    }
    if (d->n_srs < ((uint64_t)1 << d->log_n) + 3) return ctx->fail(NLX_E_RANGE, "the SRS must hold n + 3 points (blinded polynomials have up to n + 3 coefficients)");
    for (const uint64_t* sc : {d->k1, d->k2, d->coset_shift}) {
        if (is_device_ptr(sc)) return ctx->fail(NLX_E_INVAL, "k1, k2 and the coset shift are host values");
        if (!bnf::below_mod<bnf::RP>(sc)) return ctx->fail(NLX_E_RANGE, "k1, k2 or the coset shift is not below r");
    }
    (void)hipSetDevice(ctx->device);
    nlx_bn254_plonk_key* key = new nlx_bn254_plonk_key;
    key->ctx = ctx;
    int32_t rc = key_build(ctx, d, key);
    if (rc) {
        key_free(key);
        return rc;
    }
    *out = key;
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_plonk_key_destroy(nlx_bn254_plonk_key* key) NLX_TRY {
    key_free(key);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_plonk_key_info(const nlx_bn254_plonk_key* key, uint64_t out[NLX_BN254_PLONK_KEY_INFO_WORDS]) NLX_TRY {
    if (!key || !out) return NLX_E_INVAL;
    memcpy(out, key->info, sizeof key->info);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" int32_t nlx_bn254_plonk_key_commitments(const nlx_bn254_plonk_key* key, uint64_t* out) NLX_TRY {
    if (!key || !out) return NLX_E_INVAL;
    memcpy(out, key->commitments, (size_t)(8 + key->n_commit) * 64);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" size_t nlx_bn254_plonk_proof_bytes(const nlx_bn254_plonk_key* key) NLX_TRY {
    return key ? 552 + 64 * (size_t)key->n_commit : 0;
} NLX_CATCH_VALUE(nullptr, 0)

extern "C" int32_t nlx_bn254_plonk_commit(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, uint32_t j, const uint64_t* l, const uint64_t* blinding,
                                          uint64_t point_out[8], uint64_t c_out[4]) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!key || !l || !blinding || !point_out || !c_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (!key->n_commit) return ctx->fail(NLX_E_INVAL, "the key carries no commitment");
    if (j >= key->n_commit) return ctx->fail(NLX_E_RANGE, "commitment %u of %u", j, key->n_commit);
    NLX_RC(check_scalars(ctx, blinding, 2, "the commitment's blinding scalars"));
    (void)hipSetDevice(ctx->device);
    const size_t n = (size_t)1 << key->log_n;
    Staged sl(ctx, l, n * 32, true, false);
    if (sl.status) return sl.status;
    Scratch scratch(ctx);
    MsmScratch ms;
    NLX_RC(msm_scratch(ctx, scratch, &ms));
    uint64_t* d_col = scratch.alloc_as<uint64_t>(n * 32);
    uint64_t* d_b2 = scratch.alloc_as<uint64_t>(64);
    if (!d_col || !d_b2) return NLX_E_NOMEM;
    NLX_HIP(ctx, hipMemcpyAsync(d_b2, blinding, 64, hipMemcpyHostToDevice, ctx->stream));
    RoundTimer timer(ctx, "bn254_plonk_prove_commit");
    uint64_t pt[8], c[4];
    NLX_RC(commit_pi2(ctx, key, ms, j, sl.as<uint64_t>(), d_b2, d_col, pt, c));
    NLX_RC(scratch.finish(NLX_OK));
    memcpy(point_out, pt, 64);
    memcpy(c_out, c, 32);
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_plonk_prove(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                                         const uint64_t* public_inputs, uint64_t n_public, const uint64_t* blinding, const uint64_t* commit_blinding,
                                         uint8_t* proof_out, size_t proof_cap, size_t* proof_len) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!key || !l || !r || !o || !blinding || !proof_out || !proof_len || (n_public && !public_inputs)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (key->n_commit && !commit_blinding) return ctx->fail(NLX_E_INVAL, "the key carries commitments: two blinding scalars for each");
    if (!key->n_commit && commit_blinding) return ctx->fail(NLX_E_INVAL, "the key carries no commitment: commit_blinding must be NULL");
    if (n_public > ((uint64_t)1 << key->log_n)) return ctx->fail(NLX_E_RANGE, "more public inputs than rows");
    const size_t need = 552 + 64 * (size_t)key->n_commit;
    if (proof_cap < need) return ctx->fail(NLX_E_RANGE, "the proof takes %llu bytes", (unsigned long long)need);
    NLX_RC(check_scalars(ctx, blinding, 9, "the blinding scalars"));
    if (key->n_commit) NLX_RC(check_scalars(ctx, commit_blinding, 2 * (size_t)key->n_commit, "the commitments' blinding scalars"));
    if (n_public) NLX_RC(check_scalars(ctx, public_inputs, (size_t)n_public, "the public inputs"));
    std::vector<uint8_t> bytes(need);   // nothing reaches the caller's buffer before the proof is whole
    size_t len = 0;
    NLX_RC(prove_body(ctx, key, l, r, o, public_inputs, n_public, blinding, commit_blinding, bytes.data(), &len));
    memcpy(proof_out, bytes.data(), len);
    *proof_len = len;
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_fr_eval_many(nlx_ctx* ctx, uint32_t n_polys, const uint64_t* const* polys, const uint64_t* lens, const uint64_t point[4],
                                          uint64_t* out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!polys || !lens || !point || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (n_polys < 1 || n_polys > ppr::EVAL_MAX) return ctx->fail(NLX_E_RANGE, "1 .. 16 polynomials");
    if (is_device_ptr(polys) || is_device_ptr(lens) || is_device_ptr(point) || is_device_ptr(out))
        return ctx->fail(NLX_E_INVAL, "the pointer array, the lengths, the point and the values are host arrays");
    if (!bnf::below_mod<bnf::RP>(point)) return ctx->fail(NLX_E_RANGE, "the point is not below r");
    for (uint32_t i = 0; i < n_polys; i++) {
        if (!polys[i]) return ctx->fail(NLX_E_INVAL, "NULL polynomial");
        if (lens[i] < 1 || lens[i] > ((uint64_t)1 << 28)) return ctx->fail(NLX_E_RANGE, "1 .. 2^28 coefficients per polynomial");
    }
    (void)hipSetDevice(ctx->device);
    std::deque<Staged> sp;   // the polynomials are read in place
    const uint64_t* d_polys[ppr::EVAL_MAX];
    for (uint32_t i = 0; i < n_polys; i++) {
        sp.emplace_back(ctx, polys[i], (size_t)lens[i] * 32, true, false);
        if (sp[i].status) return sp[i].status;
        d_polys[i] = sp[i].as<uint64_t>();
    }
    Scratch scratch(ctx);
    std::vector<uint64_t> vals((size_t)n_polys * 4);
    NLX_RC(scratch.finish(eval_many(ctx, n_polys, d_polys, lens, bnf::load_words<bnf::RP>(point), vals.data(), scratch)));
    memcpy(out, vals.data(), vals.size() * 8);
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint64_t out[4]) NLX_TRY {
    if ((len && !msg) || (dst_len && !dst) || !out) return NLX_E_INVAL;
    if (dst_len > 255) return NLX_E_RANGE;   // RFC 9380: DST_prime carries the length in one byte
    bnf::store_words(ppr::hash_to_field(msg, len, dst, dst_len), out);
    return NLX_OK;
} NLX_CATCH(nullptr)
