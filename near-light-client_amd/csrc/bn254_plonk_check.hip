// The witness checker of the resident PLONK prover over BN254 (nlx_bn254_plonk_check_witness): which row,
// which copy or which Bsb22 commitment a witness breaks, exact on the rows of H - the counterpart over Fr of the plonky2
// checker of section 25 (prover_kernels.hip).  Nothing here is kept except the decoded sigma cells (12 n bytes on the key): the
// five selectors' values on H are made per check in the call's scratch from the key's coefficients.
//
// Fr is bn254_fp.hpp's eight 32-bit limbs in Montgomery form, as in bn254_plonk_prove.hip; the report's values are canonical.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "bn254_fp.hpp"
#include "bn254_plonk_key.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace pck {

using namespace bnf;
typedef Fp<RP> Fr;

constexpr unsigned long long NONE = ~0ull;
struct CheckBlock {
    unsigned long long gate_rows_bad, gate_first, copy_cells_bad, copy_first, sigma_bad;
    uint64_t gate_value[4];   // canonical words, written by the second launch
};

__global__ void k_plonk_check_reset(CheckBlock* __restrict__ b) {
    b->gate_rows_bad = b->copy_cells_bad = 0;
    b->gate_first = b->copy_first = b->sigma_bad = NONE;
    for (int i = 0; i < 4; i++) b->gate_value[i] = 0;
}

// a wave's count of set lanes onto a counter (one atomic per wave), the smallest key of its set lanes into a minimum
__device__ __forceinline__ void report(bool bad, unsigned long long key, unsigned long long* count, unsigned long long* first) {
    const unsigned long long m = __ballot(bad);
    if (m == 0) return;
    if ((threadIdx.x & 63) == (uint32_t)__ffsll((long long)m) - 1) atomicAdd(count, (unsigned long long)__popcll(m));
    if (bad) atomicMin(first, key);
}

// m_i: how many commitment sets hold row i.  One launch per set (the rows of a set ascend, so its lanes write distinct bytes;
// the launches of the sets follow one another on the stream).
__global__ __launch_bounds__(256) void k_plonk_check_mult(const uint32_t* __restrict__ rows, uint32_t count, uint8_t* __restrict__ mult) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) mult[rows[t]] += 1;
}

struct GateParams {
    const uint64_t *l, *r, *o;
    const uint64_t* sel;          // [5][n] ql qr qm qo qk on H
    const uint8_t* mult;          // [n] m_i, or NULL for a key without committed rows
    const uint64_t* pubs;         // n_public elements
    const uint64_t* cvals;        // k elements c_j; NULL: the commitment rows are skipped
    uint64_t n_public;
    uint32_t log_n, k;
    uint32_t crow[NLX_BN254_PLONK_MAX_COMMIT];
    CheckBlock* block;
};
// One lane per row: ql l + qr r + qm l r + qo o + qk + PI_i + m_i l on the row's own values, each polynomial read as 32-byte
// elements (a wave reads 2 KB contiguous per polynomial).  PI_i needs no column: the public inputs are the first rows, and
// the k <= 4 commitment rows are compared in registers.  No lane leaves early: rows past n redo the last row and say nothing.
// report_row == 0xFFFFFFFF: count the bad rows and find the lowest; otherwise the block holding that row runs again and its
// lane writes the value out (plain stores: one lane).
__global__ __launch_bounds__(256) void k_plonk_check_gates(GateParams p, uint32_t row0, uint32_t report_row) {
    const size_t n = (size_t)1 << p.log_n;
    const size_t raw = (size_t)row0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = raw < n;
    const size_t row = live ? raw : n - 1;
    const Fr l = load<RP>(p.l, row), r = load<RP>(p.r, row), o = load<RP>(p.o, row);
    Fr ql = load<RP>(p.sel, row);
    const uint32_t m = p.mult ? p.mult[row] : 0u;
    for (uint32_t t = 0; t < m; t++) ql = add(ql, one<RP>());   // (ql + m_i) l
    Fr pi = zero<RP>();
    if (row < p.n_public) pi = load<RP>(p.pubs, row);
    bool skip = false;
    for (uint32_t j = 0; j < p.k; j++)
        if (row == p.crow[j]) {
            if (p.cvals) pi = load<RP>(p.cvals, j);
            else skip = true;
        }
    Fr v = mul(ql, l);
    v = add(v, mul(load<RP>(p.sel, n + row), r));
    v = add(v, mul(load<RP>(p.sel, 2 * n + row), mul(l, r)));
    v = add(v, mul(load<RP>(p.sel, 3 * n + row), o));
    v = add(v, add(load<RP>(p.sel, 4 * n + row), pi));
    const bool bad = live && !skip && !is_zero(v);
    if (report_row == 0xFFFFFFFFu) {
        report(bad, (unsigned long long)row, &p.block->gate_rows_bad, &p.block->gate_first);
    } else if (live && row == report_row) {
        store_words(from_mont(v), p.block->gate_value);
    }
}

// Sigma values back to cells, one lane per cell (wire c, row i): sigma(c, i) = k_c' w^i' as a field element (section 25's four
// steps over Fr).
//   1. the identity k_c w^i first (a wave whose cells are all routed to themselves stops here);
//   2. else the coset: v^n against 1, k1^n, k2^n picks c';
//   3. then the logarithm of u = v / k_c' in the subgroup of order n = 2^log_n, bit by bit from the low end: with the low i bits
//      of the exponent cleared, u^(2^(log_n-1-i)) is 1 or -1 as bit i is 0 or 1 (log_n (log_n + 1) / 2 squarings with step 2);
//   4. and k_c' w^i' == v once more, so that what is stored is exact; anything else is undecodable.
// Steps 2 and 3 are selects on per-lane data, never branches: every loop's trip count depends on log_n alone.
// tab (Montgomery): [0..2] 1 k1 k2 | [3..5] their n-th powers | [6..8] their inverses | [9 ..] w^(2^i), i < log_n |
// [9 + log_n ..] w^(-2^i), i < log_n.
__device__ __forceinline__ Fr select(bool c, const Fr& a, const Fr& b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
__device__ __forceinline__ Fr root_pow(const uint64_t* __restrict__ tab, uint32_t log_n, uint32_t e) {
    Fr x = one<RP>();
#pragma unroll 1
    for (uint32_t i = 0; i < log_n; i++) x = select((e >> i) & 1, mul(x, load<RP>(tab, 9 + i)), x);
    return x;
}
__global__ __launch_bounds__(256) void k_plonk_sigma_decode(const uint64_t* __restrict__ sigma, const uint64_t* __restrict__ tab, uint32_t log_n,
                                                            uint32_t* __restrict__ cells, CheckBlock* __restrict__ block) {
    const size_t n = (size_t)1 << log_n;
    const size_t raw = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = raw < n;
    const uint32_t row = (uint32_t)(live ? raw : n - 1), c = blockIdx.y;
    const size_t idx = (size_t)c * n + row;
    const Fr v = load<RP>(sigma, idx);
    const bool ident = equal(v, mul(load<RP>(tab, c), root_pow(tab, log_n, row)));
    uint32_t tc = c, tr = row;
    if (__ballot(!ident) != 0) {   // wave-uniform
        Fr vn = v;
#pragma unroll 1
        for (uint32_t i = 0; i < log_n; i++) vn = sqr(vn);
        uint32_t dc = 3;
#pragma unroll
        for (int j = 2; j >= 0; j--) dc = equal(vn, load<RP>(tab, 3 + j)) ? (uint32_t)j : dc;
        const uint32_t kc = dc < 3 ? dc : 0;
        Fr cur = mul(v, select(kc == 2, load<RP>(tab, 8), select(kc == 1, load<RP>(tab, 7), load<RP>(tab, 6))));
        uint32_t dr = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < log_n; i++) {
            Fr t = cur;
#pragma unroll 1
            for (uint32_t s = 0; s + 1 + i < log_n; s++) t = sqr(t);
            const bool bit = !equal(t, one<RP>());
            dr |= (uint32_t)bit << i;
            cur = select(bit, mul(cur, load<RP>(tab, 9 + log_n + i)), cur);
        }
        const Fr back = mul(select(kc == 2, load<RP>(tab, 2), select(kc == 1, load<RP>(tab, 1), load<RP>(tab, 0))), root_pow(tab, log_n, dr));
        if (!equal(back, v)) dc = 3;
        tc = ident ? c : dc;
        tr = ident ? row : dr;
    }
    if (!live) return;
    if (tc > 2) {
        atomicMin(&block->sigma_bad, (unsigned long long)idx);
        tc = 3, tr = 0;
    }
    cells[idx] = tc << 30 | tr;
}

// One lane per cell: its value against the value at the decoded partner.  Both ends of a broken copy are bad cells.
__global__ __launch_bounds__(256) void k_plonk_check_copies(const uint64_t* l, const uint64_t* r, const uint64_t* o, uint32_t log_n,
                                                            const uint32_t* __restrict__ cells, CheckBlock* __restrict__ block) {
    const size_t n = (size_t)1 << log_n;
    const size_t raw = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = raw < n;
    const size_t row = live ? raw : n - 1;
    const uint32_t c = blockIdx.y;
    const uint32_t cell = cells[(size_t)c * n + row];
    const uint32_t tc = cell >> 30, tr = cell & 0x3FFFFFFFu;
    const uint64_t* from = c == 0 ? l : c == 1 ? r : o;
    const uint64_t* to = tc == 0 ? l : tc == 1 ? r : o;
    const bool bad = live && tc < 3 && tr < n && !equal(load<RP>(from, row), load<RP>(to, tr));
    report(bad, (unsigned long long)row << 2 | c, &block->copy_cells_bad, &block->copy_first);
}

}  // namespace pck
}  // namespace nlx

using namespace nlx;
using namespace nlx::ppk;
using nlx::pck::CheckBlock;
using nlx::pck::Fr;

namespace {

const char* const WIRE_NAMES[3] = {"L", "R", "O"};

// the canonical words of a Montgomery element on the host / in device memory
void canon(const uint64_t mont[4], uint64_t out[4]) { bnf::store_words(bnf::from_mont(bnf::load_words<bnf::RP>(mont)), out); }
int32_t fetch_canon(nlx_ctx* ctx, const uint64_t* d_elem, uint64_t out[4]) {
    uint64_t w[4];
    NLX_RC(fetch(ctx, w, d_elem, 32));
    canon(w, out);
    return NLX_OK;
}
std::string hex(const uint64_t w[4]) {
    char buf[80];
    snprintf(buf, sizeof buf, "0x%016llx%016llx%016llx%016llx", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1],
             (unsigned long long)w[0]);
    return buf;
}

// s1 s2 s3 as cells, once per key: kept only when every value decoded
int32_t ensure_sigma_cells(nlx_ctx* ctx, nlx_bn254_plonk_key* key, CheckBlock* d_block, Scratch& scratch) {
    using namespace bnf;
    if (key->sigma_cells) return NLX_OK;
    const uint32_t log_n = key->log_n;
    const size_t n = (size_t)1 << log_n;
    const Fr ks[3] = {one<RP>(), load_words<RP>(key->k1), load_words<RP>(key->k2)};
    Fr kn[3], w = root28();
    for (int i = 0; i < 3; i++) kn[i] = pow_host(ks[i], n);
    if (equal(kn[0], kn[1]) || equal(kn[0], kn[2]) || equal(kn[1], kn[2]))
        return ctx->fail(NLX_E_INVAL, "the key's cosets H, k1 H, k2 H are not disjoint (1, k1^n, k2^n are not pairwise distinct): sigma cannot be decoded");
    for (uint32_t i = log_n; i < 28; i++) w = sqr(w);
    std::vector<uint64_t> tab((size_t)(9 + 2 * log_n) * 4);
    Fr wp = w, wi = inv_host(w);
    for (int i = 0; i < 3; i++) {
        store_words(ks[i], &tab[4 * i]);
        store_words(kn[i], &tab[4 * (3 + i)]);
        store_words(inv_host(ks[i]), &tab[4 * (6 + i)]);
    }
    for (uint32_t i = 0; i < log_n; i++, wp = sqr(wp), wi = sqr(wi)) {
        store_words(wp, &tab[4 * (9 + i)]);
        store_words(wi, &tab[4 * (9 + log_n + i)]);
    }
    uint64_t* d_tab = scratch.alloc_as<uint64_t>(tab.size() * 8);
    uint32_t* d_cells = (uint32_t*)ctx->alloc(3 * n * 4);
    auto give_back = [&](int32_t rc) {
        (void)hipStreamSynchronize(ctx->stream);
        ctx->release(d_cells);
        return rc;
    };
    if (!d_tab || !d_cells) return give_back(ctx->fail(NLX_E_NOMEM, "out of device memory (sigma cells)"));
    hipError_t e = hipMemcpy(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return give_back(ctx->hip_fail(e, "hipMemcpy(coset tables)"));
    ctx->begin_kernel("bn254_plonk_sigma_decode", 3.0 * n * 36);
    hipLaunchKernelGGL(pck::k_plonk_sigma_decode, dim3((unsigned)((n + 255) / 256), 3), dim3(256), 0, ctx->stream, key->sigma, d_tab, log_n, d_cells,
                       d_block);
    ctx->end_kernel();
    CheckBlock b;
    int32_t rc = fetch(ctx, &b, d_block, sizeof b);
    if (rc) return give_back(rc);
    if (b.sigma_bad != pck::NONE)
        return give_back(ctx->fail(NLX_E_INVAL, "sigma value s%llu at row %llu lies in no coset {1, k1, k2} H of the key", b.sigma_bad / n + 1,
                                   b.sigma_bad % n));
    key->sigma_cells = d_cells;
    return NLX_OK;
}

int32_t check_body(nlx_ctx* ctx, nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o, const uint64_t* pubs,
                   uint64_t n_public, const uint64_t* commit_blinding, uint32_t what, nlx_bn254_plonk_witness_report* rep, Scratch& scratch) {
    const uint32_t log_n = key->log_n, k = key->n_commit;
    const size_t n = (size_t)1 << log_n, m = n + 3;
    hipStream_t st = ctx->stream;
    if (!k) what &= ~NLX_BN254_PLONK_CHECK_COMMITS;
    rep->checked = what;
    rep->satisfied = 1;
    rep->cache_bytes = key->sigma_cells ? 12 * (uint64_t)n : 0;
    if (!what) return NLX_OK;
    Staged sl(ctx, l, n * 32, true, false), sr(ctx, r, n * 32, true, false), so(ctx, o, n * 32, true, false);
    for (const Staged* s : {&sl, &sr, &so})
        if (s->status) return s->status;
    const uint64_t *d_l = sl.as<uint64_t>(), *d_r = sr.as<uint64_t>(), *d_o = so.as<uint64_t>();
    CheckBlock* d_block = scratch.alloc_as<CheckBlock>(sizeof(CheckBlock));
    uint64_t* d_small = scratch.alloc_as<uint64_t>((size_t)3 * NLX_BN254_PLONK_MAX_COMMIT * 32);   // commit_blinding (2 k) | c_j (k)
    if (!d_block || !d_small) return ctx->fail(NLX_E_NOMEM, "PLONK check: device memory");
    uint64_t* d_c = d_small + 2 * NLX_BN254_PLONK_MAX_COMMIT * 4;
    hipLaunchKernelGGL(pck::k_plonk_check_reset, dim3(1), dim3(1), 0, st, d_block);
    const bool with_c = (what & NLX_BN254_PLONK_CHECK_COMMITS) != 0;
    char line[3][400] = {"", "", ""};

    // commits first: the gate pass reads the c_j
    if (with_c) {
        MsmScratch ms;
        NLX_RC(msm_scratch(ctx, scratch, &ms));
        uint64_t* d_col = scratch.alloc_as<uint64_t>(n * 32);
        if (!d_col) return ctx->fail(NLX_E_NOMEM, "PLONK check: device memory");
        NLX_HIP(ctx, hipMemcpy(d_small, commit_blinding, (size_t)2 * k * 32, hipMemcpyHostToDevice));
        uint64_t cw[NLX_BN254_PLONK_MAX_COMMIT][4];
        for (uint32_t j = 0; j < k; j++) {
            uint64_t point[8], have[4];
            NLX_RC(commit_pi2(ctx, key, ms, j, d_l, d_small + 8 * j, d_col, point, cw[j]));
            NLX_RC(fetch(ctx, have, d_l + 4 * (size_t)key->commit_rows[j], 32));
            if (memcmp(have, cw[j], 32)) {
                if (!rep->commits_bad++) {
                    rep->commit_index = j;
                    rep->commit_row = key->commit_rows[j];
                    canon(have, rep->commit_have);
                    canon(cw[j], rep->commit_want);
                }
            }
        }
        NLX_HIP(ctx, hipMemcpy(d_c, cw, (size_t)k * 32, hipMemcpyHostToDevice));
        if (rep->commits_bad)
            snprintf(line[2], sizeof line[2], "Bsb22 commitment %u: the L wire of its commitment row %u holds %s, the hash of the commitment is %s, %u commitment(s) wrong",
                     rep->commit_index, rep->commit_row, hex(rep->commit_have).c_str(), hex(rep->commit_want).c_str(), rep->commits_bad);
    }

    pck::GateParams gp{};
    if (what & NLX_BN254_PLONK_CHECK_GATES) {
        // ql qr qm qo qk on H: five forward transforms of the key's coefficients, in the call's scratch
        uint64_t* d_sel = scratch.alloc_as<uint64_t>(5 * n * 32);
        if (!d_sel) return ctx->fail(NLX_E_NOMEM, "PLONK check: device memory for the selectors on H");
        NLX_HIP(ctx, hipMemcpy2DAsync(d_sel, n * 32, key->coeffs, m * 32, n * 32, 5, hipMemcpyDeviceToDevice, st));
        NLX_RC(nlx_bn254_ntt_batch(ctx, d_sel, 5, log_n, 0, NLX_BN254_MONTGOMERY));
        gp.l = d_l, gp.r = d_r, gp.o = d_o, gp.sel = d_sel, gp.block = d_block;
        gp.log_n = log_n, gp.k = k, gp.n_public = n_public;
        if (k && key->seg[k]) {
            uint8_t* d_mult = scratch.alloc_as<uint8_t>(n);
            if (!d_mult) return ctx->fail(NLX_E_NOMEM, "PLONK check: device memory");
            NLX_HIP(ctx, hipMemsetAsync(d_mult, 0, n, st));
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t count = key->seg[j + 1] - key->seg[j];
                if (count) hipLaunchKernelGGL(pck::k_plonk_check_mult, dim3((count + 255) / 256), dim3(256), 0, st, key->rows + key->seg[j], count, d_mult);
            }
            gp.mult = d_mult;
        }
        if (n_public) {
            uint64_t* d_pubs = scratch.alloc_as<uint64_t>(n_public * 32);
            if (!d_pubs) return ctx->fail(NLX_E_NOMEM, "PLONK check: device memory");
            NLX_HIP(ctx, hipMemcpy(d_pubs, pubs, n_public * 32, hipMemcpyHostToDevice));
            gp.pubs = d_pubs;
        }
        for (uint32_t j = 0; j < k; j++) {
            gp.crow[j] = key->commit_rows[j];
            bool seen = false;
            for (uint32_t t = 0; t < j; t++) seen |= key->commit_rows[t] == key->commit_rows[j];
            if (!with_c && !seen) rep->gate_rows_skipped++;
        }
        gp.cvals = with_c ? d_c : nullptr;
        ctx->begin_kernel("bn254_plonk_check_gates", 8.0 * n * 32);
        hipLaunchKernelGGL(pck::k_plonk_check_gates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gp, 0u, 0xFFFFFFFFu);
        ctx->end_kernel();
    }
    if (what & NLX_BN254_PLONK_CHECK_COPIES) {
        NLX_RC(ensure_sigma_cells(ctx, key, d_block, scratch));
        rep->cache_bytes = 12 * (uint64_t)n;
        ctx->begin_kernel("bn254_plonk_check_copies", 3.0 * n * 68);
        hipLaunchKernelGGL(pck::k_plonk_check_copies, dim3((unsigned)((n + 255) / 256), 3), dim3(256), 0, st, d_l, d_r, d_o, log_n, key->sigma_cells, d_block);
        ctx->end_kernel();
    }
    CheckBlock b;
    NLX_RC(fetch(ctx, &b, d_block, sizeof b));
    rep->gate_rows_bad = b.gate_rows_bad;
    rep->copy_cells_bad = b.copy_cells_bad;
    rep->satisfied = !(b.gate_rows_bad || b.copy_cells_bad || rep->commits_bad);
    if (rep->satisfied) return NLX_OK;
    // the details of each first finding: a handful of words from the device, on the failing path only
    if (b.gate_rows_bad) {
        rep->gate_row = (uint32_t)b.gate_first;
        hipLaunchKernelGGL(pck::k_plonk_check_gates, dim3(1), dim3(256), 0, st, gp, rep->gate_row & ~255u, rep->gate_row);
        NLX_RC(fetch(ctx, &b, d_block, sizeof b));
        memcpy(rep->gate_value, b.gate_value, 32);
        snprintf(line[0], sizeof line[0], "row %u: ql l + qr r + qm l r + qo o + qk + PI + m l = %s, %llu row(s) with a non-zero constraint", rep->gate_row,
                 hex(rep->gate_value).c_str(), (unsigned long long)rep->gate_rows_bad);
    }
    if (b.copy_cells_bad) {
        rep->copy_row = (uint32_t)(b.copy_first >> 2);
        rep->copy_wire = (uint32_t)(b.copy_first & 3);
        uint32_t cell = 0;
        NLX_RC(fetch(ctx, &cell, key->sigma_cells + (size_t)rep->copy_wire * n + rep->copy_row, 4));
        rep->copy_to_wire = cell >> 30;
        rep->copy_to_row = cell & 0x3FFFFFFFu;
        const uint64_t* d_wire[3] = {d_l, d_r, d_o};
        NLX_RC(fetch_canon(ctx, d_wire[rep->copy_wire] + 4 * (size_t)rep->copy_row, rep->copy_value));
        NLX_RC(fetch_canon(ctx, d_wire[rep->copy_to_wire] + 4 * (size_t)rep->copy_to_row, rep->copy_to_value));
        snprintf(line[1], sizeof line[1], "copy: wire %s of row %u = %s but sigma sends it to wire %s of row %u = %s, %llu cell(s) differ from their copy",
                 WIRE_NAMES[rep->copy_wire], rep->copy_row, hex(rep->copy_value).c_str(), WIRE_NAMES[rep->copy_to_wire], rep->copy_to_row,
                 hex(rep->copy_to_value).c_str(), (unsigned long long)rep->copy_cells_bad);
    }
    std::string msg = "the witness does not satisfy the circuit: ";
    bool any = false;
    for (const auto& t : line)
        if (t[0]) {
            if (any) msg += "; ";
            msg += t;
            any = true;
        }
    ctx->err = msg;
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_plonk_check_witness(nlx_ctx* ctx, nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                                                 const uint64_t* public_inputs, uint64_t n_public, const uint64_t* commit_blinding, uint32_t what,
                                                 nlx_bn254_plonk_witness_report* report) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (report) memset(report, 0, sizeof *report);
    if (!key || !l || !r || !o || !report || (n_public && !public_inputs)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (what < 1 || what > NLX_BN254_PLONK_CHECK_ALL)
        return ctx->fail(NLX_E_INVAL, "what = %u: a non-empty set of NLX_BN254_PLONK_CHECK_* bits (1 .. 7)", what);
    const bool commits = key->n_commit && (what & NLX_BN254_PLONK_CHECK_COMMITS);
    if (commits && !commit_blinding) return ctx->fail(NLX_E_INVAL, "NLX_BN254_PLONK_CHECK_COMMITS: the key carries commitments, two blinding scalars for each");
    if (n_public > ((uint64_t)1 << key->log_n)) return ctx->fail(NLX_E_RANGE, "more public inputs than rows");
    if (commits) NLX_RC(check_scalars(ctx, commit_blinding, 2 * (size_t)key->n_commit, "the commitments' blinding scalars"));
    if (n_public) NLX_RC(check_scalars(ctx, public_inputs, (size_t)n_public, "the public inputs"));
    (void)hipSetDevice(ctx->device);
    int32_t rc;
    {
        Scratch scratch(ctx);
        rc = scratch.finish(check_body(ctx, key, l, r, o, public_inputs, n_public, commit_blinding, what, report, scratch));
    }
    if (rc) memset(report, 0, sizeof *report);
    return rc;
} NLX_CATCH(ctx)
