// Row f.4, the PLONK half: gnark's plonk.Setup(spr, srs) on the device, from the constraints - a
// SparseR1CS in, the trace on H (ql qr qm qo qk s1 s2 s3 qcp_j by values), the 3 n cells and the copy permutation out, resident;
// nlx_bn254_plonk_setup_key builds the resident proving key from them through nlx_bn254_plonk_key_create and hands it the decoded
// permutation; nlx_bn254_plonk_setup_wires is the solver's last step (variables -> l r o); nlx_bn254_kzg_srs makes a test SRS.
//
// The rules are those of tools/gnark_plonk_setup_model.py, the place of record: RECALLED from gnark v0.9 (backend/plonk/bn254
// setup.go), UNPINNED - there is no Go source and no gnark-produced key to compare with; parity with gnark's keys is not claimed.
//
// Fr in Montgomery form on bn254_fp.hpp's eight 32-bit limbs:
//   k_pls_rows          a lane per row: the five selectors gathered from the coefficient table (-1 on public rows, 0 on
//                       padding), the qcp_j (a binary search of the row in each ascending set), the three cell ids, and the
//                       positions 0 .. 3 n - 1 the sort carries;
//   hipcub radix sort   (variable id, position) by variable id over the bits n_variables needs: stable, so a class keeps its
//                       positions ascending - rule 3 depends on that order;
//   k_pls_class_ends    the slot that closes a class (its right neighbour holds another key) writes its index per variable;
//   k_pls_perm          per sorted slot (a fixed grid strides): perm[sorted[j]] = sorted[j - 1] inside a class, the first slot takes the
//                       last.  No lane walks a class: variable 0 alone holds about 2 n positions of a padded circuit;
//   k_pls_root_tables   w^lo for lo < 2^half and w^(hi << half): two tables of at most 2^13 entries (256 KiB each at 2^26);
//   k_pls_sigma         a lane per position: (1, k1, k2)[c'] * w^row' = two loads and two products, and the checker's cell word;
//   k_pls_wires         a lane per cell: l[row] = values[cell];
//   k_pls_tau_powers    lane i: tau^i from tau^(2^b), selects, at most 27 steps; a step whose bit no lane of the wave has is skipped.
#include <hipcub/hipcub.hpp>
#include <cstring>
#include <memory>
#include <vector>
#include "bn254_fixed_base.hpp"
#include "bn254_fp.hpp"
#include "bn254_plonk_key.hpp"
#include "bn254_plonk_setup.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace pls {

using namespace bnf;
typedef Fp<RP> Fr;

constexpr uint32_t MAX_K = NLX_BN254_PLONK_MAX_COMMIT;

__device__ __forceinline__ Fr select(bool c, const Fr& a, const Fr& b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}

struct RowsParams {
    const uint32_t *xa, *xb, *xc;           // [n_constraints] variable ids
    const uint32_t* sel[5];                 // [n_constraints] coefficient ids: ql qr qm qo qk
    const uint64_t* coeffs;                 // [n_coeffs][4]
    const uint32_t* committed_rows;         // the k sets concatenated, rows of H, ascending in a set
    uint32_t seg[MAX_K + 1];
    uint64_t n_public, n_used;              // n_used = N = n_public + n_constraints
    uint32_t log_n, k;
    uint64_t* vals;                         // [8 + k][n][4]
    uint32_t *cells, *iota;                 // [3 n]
};
__global__ __launch_bounds__(256) void k_pls_rows(RowsParams p) {
    const size_t n = (size_t)1 << p.log_n;
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const bool is_public = row < p.n_public, is_constraint = !is_public && row < p.n_used;
    const size_t c = is_constraint ? row - p.n_public : 0;
    uint32_t cell[3] = {is_public ? (uint32_t)row : 0u, 0u, 0u};
    if (is_constraint) cell[0] = p.xa[c], cell[1] = p.xb[c], cell[2] = p.xc[c];
#pragma unroll
    for (int col = 0; col < 3; col++) {
        p.cells[col * n + row] = cell[col];
        p.iota[col * n + row] = (uint32_t)(col * n + row);
    }
    const Fr minus_one = neg(one<RP>());
#pragma unroll
    for (int s = 0; s < 5; s++) {
        Fr v = zero<RP>();
        if (is_constraint) v = load<RP>(p.coeffs, p.sel[s][c]);
        else if (is_public && s == 0) v = minus_one;
        store(p.vals, (size_t)s * n + row, v);
    }
    for (uint32_t j = 0; j < p.k; j++) {
        uint32_t lo = p.seg[j], hi = p.seg[j + 1];   // the first entry >= row lies in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (p.committed_rows[mid] < row) lo = mid + 1;
            else hi = mid;
        }
        const bool in = lo < p.seg[j + 1] && p.committed_rows[lo] == row;
        store(p.vals, (size_t)(8 + j) * n + row, in ? one<RP>() : zero<RP>());
    }
}

struct ClassStats {
    unsigned long long occurring;   // variables that hold at least one cell
    unsigned int longest;           // the cells of the one that holds most
};
__global__ __launch_bounds__(256) void k_pls_class_ends(const uint32_t* __restrict__ keys, size_t total, uint32_t* __restrict__ last_slot) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const uint32_t key = keys[j];
    if (j + 1 == total || keys[j + 1] != key) last_slot[key] = (uint32_t)j;
}
// A fixed grid strides over the slots, so that the two counters take one atomic per wave of the grid, not per wave of slots
// (at 3 * 2^20 slots the per-slot-wave form spent most of its time on them).  Every lane reaches the wave's joins.
constexpr unsigned PERM_MAX_BLOCKS = 2048;
__global__ __launch_bounds__(256) void k_pls_perm(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pos, size_t total,
                                                  const uint32_t* __restrict__ last_slot, uint32_t* __restrict__ perm, ClassStats* __restrict__ stats) {
    uint32_t classes = 0, longest = 0;
#pragma unroll 1
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x) {
        const uint32_t key = keys[j];
        uint32_t from;
        if (j == 0 || keys[j - 1] != key) {   // the class's first slot takes its last
            const uint32_t last = last_slot[key], len = last - (uint32_t)j + 1;
            from = pos[last];
            classes++;
            longest = len > longest ? len : longest;
        } else {
            from = pos[j - 1];
        }
        perm[pos[j]] = from;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        classes += (uint32_t)__shfl_xor((int)classes, d, 64);
        const uint32_t o = (uint32_t)__shfl_xor((int)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63) == 0 && classes) {
        atomicAdd(&stats->occurring, (unsigned long long)classes);
        atomicMax(&stats->longest, longest);
    }
}

// lo[i] = w^i for i < 2^half, hi[i] = w^(i << half) for i < 2^(log_n - half): w and w^(2^half) raised by square-and-multiply
__global__ __launch_bounds__(256) void k_pls_root_tables(Fr w, Fr w_hi, uint32_t n_lo, uint32_t n_hi, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_lo + n_hi) return;
    const bool low = t < n_lo;
    Fr b = low ? w : w_hi, r = one<RP>();
#pragma unroll 1
    for (uint32_t e = low ? t : t - n_lo; e; e >>= 1) {
        if (e & 1) r = mul(r, b);
        b = sqr(b);
    }
    store(low ? lo : hi, low ? t : t - n_lo, r);
}
struct SigmaParams {
    Fr k[3];                        // 1, k1, k2
    const uint32_t* perm;           // [3 n]
    const uint64_t *lo, *hi;        // the two tables
    uint32_t log_n, half;
    uint64_t* sigma;                // [3][n][4]
    uint32_t* sigma_cells;          // [3 n]
};
__global__ __launch_bounds__(256) void k_pls_sigma(SigmaParams p) {
    const size_t n = (size_t)1 << p.log_n;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= 3 * n) return;
    const uint32_t q = p.perm[pos];
    const uint32_t c = q >> p.log_n, row = q & (uint32_t)(n - 1);
    const Fr wr = mul(load<RP>(p.lo, row & ((1u << p.half) - 1)), load<RP>(p.hi, row >> p.half));
    store(p.sigma, pos, mul(select(c == 2, p.k[2], select(c == 1, p.k[1], p.k[0])), wr));
    p.sigma_cells[pos] = c << 30 | row;
}

__global__ __launch_bounds__(256) void k_pls_wires(const uint32_t* __restrict__ cells, uint32_t log_n, const uint64_t* __restrict__ values,
                                                   uint64_t* __restrict__ l, uint64_t* __restrict__ r, uint64_t* __restrict__ o) {
    const size_t n = (size_t)1 << log_n;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= 3 * n) return;
    const size_t col = pos >> log_n, row = pos & (n - 1);
    store(col == 0 ? l : col == 1 ? r : o, row, load<RP>(values, cells[pos]));
}

// out[i] = tau^i, i < n: the product of tab[b] = tau^(2^b) over the set bits of i
__global__ __launch_bounds__(256) void k_pls_tau_powers(const uint64_t* __restrict__ tab, uint32_t n_bits, size_t n, uint64_t* __restrict__ out) {
    const size_t raw = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = raw < n;
    const size_t i = live ? raw : n - 1;
    Fr r = one<RP>();
#pragma unroll 1
    for (uint32_t b = 0; b < n_bits; b++) {
        const bool bit = (i >> b) & 1;
        if (__ballot(bit) == 0) continue;   // wave-uniform
        r = select(bit, mul(r, load<RP>(tab, b)), r);
    }
    if (live) store(out, i, r);
}

}  // namespace pls
}  // namespace nlx

using namespace nlx;
using pls::Fr;

typedef struct nlx_bn254_plonk_setup PSetup;   // the plain name is the entry point's

namespace {

// the caller's arrays on the host for the checks; dropped when the call returns
struct Checked {
    std::vector<uint32_t> x[3], sel[5];
    std::vector<uint64_t> coeffs;
};

template <class T>
int32_t to_host(nlx_ctx* ctx, const T* p, size_t count, std::vector<T>& out) {
    out.resize(count);
    if (!count) return NLX_OK;
    NLX_HIP(ctx, hipMemcpy(out.data(), p, count * sizeof(T), hipMemcpyDefault));
    return NLX_OK;
}

void setup_free(PSetup* s) {
    if (!s) return;
    if (s->ctx && s->vals) {
        (void)hipStreamSynchronize(s->ctx->stream);
        s->ctx->release(s->vals);
    }
    delete s;
}

const char* const X_NAMES[3] = {"xa", "xb", "xc"};
const char* const SEL_NAMES[5] = {"ql", "qr", "qm", "qo", "qk"};

// every refusal, on the host, before anything is allocated on the device; fills the result's host side
int32_t load_and_check(nlx_ctx* ctx, const nlx_bn254_plonk_setup_desc* d, PSetup& s, Checked& c) {
    if (d->flags != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "flags must be NLX_BN254_MONTGOMERY");
    if (d->n_public > ((uint64_t)1 << 26) || d->n_constraints > ((uint64_t)1 << 26))
        return ctx->fail(NLX_E_RANGE, "log_n: n_public + n_constraints = %llu + %llu rows exceed 2^26", (unsigned long long)d->n_public, (unsigned long long)d->n_constraints);
    const uint64_t used = d->n_public + d->n_constraints;
    uint32_t log_n = d->log_n;
    if (log_n == 0) {
        log_n = 3;
        while (log_n < 26 && ((uint64_t)1 << log_n) < used) log_n++;
    }
    if (log_n < 3 || log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n must be 0 or in [3, 26]");
    if (((uint64_t)1 << log_n) < used)
        return ctx->fail(NLX_E_RANGE, "log_n = %u is too small: n_public + n_constraints = %llu rows", log_n, (unsigned long long)used);
    if (d->n_variables == 0 || d->n_variables < d->n_public || d->n_variables > 0xFFFFFFFFull)
        return ctx->fail(NLX_E_RANGE, "n_variables = %llu: at least 1 (variable 0 pads), at least n_public = %llu, below 2^32", (unsigned long long)d->n_variables,
                         (unsigned long long)d->n_public);
    if (d->n_commit > pls::MAX_K) return ctx->fail(NLX_E_RANGE, "n_commit must be in [0, %u]", pls::MAX_K);
    if (!d->k1 || !d->k2 || !d->coset_shift) return ctx->fail(NLX_E_INVAL, "NULL argument (k1, k2, coset_shift)");
    const uint64_t* sc[3] = {d->k1, d->k2, d->coset_shift};
    const char* const sc_names[3] = {"k1", "k2", "coset_shift"};
    for (int i = 0; i < 3; i++) {
        if (is_device_ptr(sc[i])) return ctx->fail(NLX_E_INVAL, "%s is a host value", sc_names[i]);
        if (!bnf::below_mod<bnf::RP>(sc[i])) return ctx->fail(NLX_E_RANGE, "%s is not below r", sc_names[i]);
    }
    s.ctx = ctx;
    s.log_n = log_n, s.k = d->n_commit;
    s.n_variables = d->n_variables, s.n_public = d->n_public, s.n_constraints = d->n_constraints;
    memcpy(s.k1, d->k1, 32), memcpy(s.k2, d->k2, 32), memcpy(s.shift, d->coset_shift, 32);
    const uint64_t nc = d->n_constraints;
    if (nc) {
        const uint32_t* x[3] = {d->xa, d->xb, d->xc};
        const uint32_t* q[5] = {d->ql, d->qr, d->qm, d->qo, d->qk};
        for (int i = 0; i < 3; i++)
            if (!x[i]) return ctx->fail(NLX_E_INVAL, "NULL argument (%s)", X_NAMES[i]);
        for (int i = 0; i < 5; i++)
            if (!q[i]) return ctx->fail(NLX_E_INVAL, "NULL argument (%s)", SEL_NAMES[i]);
        if (!d->coeffs) return ctx->fail(NLX_E_INVAL, "NULL argument (coeffs)");
        if (d->n_coeffs > 0xFFFFFFFFull) return ctx->fail(NLX_E_RANGE, "the coefficient table holds at most 2^32 - 1 entries");
        NLX_RC(to_host(ctx, d->coeffs, (size_t)d->n_coeffs * 4, c.coeffs));
        for (uint64_t i = 0; i < d->n_coeffs; i++)
            if (!bnf::below_mod<bnf::RP>(&c.coeffs[4 * i])) return ctx->fail(NLX_E_RANGE, "coefficient %llu is not below r", (unsigned long long)i);
        for (int i = 0; i < 3; i++) {
            NLX_RC(to_host(ctx, x[i], (size_t)nc, c.x[i]));
            for (uint64_t t = 0; t < nc; t++)
                if (c.x[i][t] >= d->n_variables)
                    return ctx->fail(NLX_E_RANGE, "constraint %llu, %s: variable %u of %llu", (unsigned long long)t, X_NAMES[i], c.x[i][t], (unsigned long long)d->n_variables);
        }
        for (int i = 0; i < 5; i++) {
            NLX_RC(to_host(ctx, q[i], (size_t)nc, c.sel[i]));
            for (uint64_t t = 0; t < nc; t++)
                if (c.sel[i][t] >= d->n_coeffs)
                    return ctx->fail(NLX_E_RANGE, "constraint %llu, %s: coefficient %u of %llu", (unsigned long long)t, SEL_NAMES[i], c.sel[i][t], (unsigned long long)d->n_coeffs);
        }
    }
    const uint32_t k = s.k;
    if (k) {
        if (!d->n_committed || !d->commit_constraint) return ctx->fail(NLX_E_INVAL, "NULL argument (n_committed, commit_constraint)");
        NLX_RC(to_host(ctx, d->n_committed, (size_t)k, s.counts));
        NLX_RC(to_host(ctx, d->commit_constraint, (size_t)k, s.commit_rows));
        uint64_t total = 0;
        for (uint32_t j = 0; j < k; j++) {
            if (s.counts[j] > nc) return ctx->fail(NLX_E_RANGE, "commitment %u commits %llu constraints of %llu", j, (unsigned long long)s.counts[j], (unsigned long long)nc);
            total += s.counts[j];
        }
        if (total && !d->committed) return ctx->fail(NLX_E_INVAL, "NULL argument (committed)");
        NLX_RC(to_host(ctx, d->committed, (size_t)total, s.committed_rows));
        size_t t = 0;
        for (uint32_t j = 0; j < k; j++)
            for (uint64_t i = 0; i < s.counts[j]; i++, t++) {
                const uint32_t id = s.committed_rows[t];
                if (id >= nc) return ctx->fail(NLX_E_RANGE, "commitment %u: committed constraint %u of %llu", j, id, (unsigned long long)nc);
                if (i && id <= s.committed_rows[t - 1]) return ctx->fail(NLX_E_RANGE, "commitment %u: the committed constraints do not ascend at %u", j, id);
            }
        for (uint32_t j = 0; j < k; j++) {
            if (s.commit_rows[j] >= nc) return ctx->fail(NLX_E_RANGE, "commitment %u: its constraint %u of %llu", j, s.commit_rows[j], (unsigned long long)nc);
            s.commit_rows[j] += (uint32_t)d->n_public;
        }
        for (uint32_t& r : s.committed_rows) r += (uint32_t)d->n_public;   // constraint index -> row of H
    }
    return NLX_OK;
}

// a caller's array where the kernels can read it: device pointers in place, host data (already copied for the checks) uploaded
template <class T>
int32_t on_device(nlx_ctx* ctx, Scratch& scratch, const T* user, const std::vector<T>& host, const T** out) {
    if (user && is_device_ptr(user)) {
        *out = user;
        return NLX_OK;
    }
    T* d = scratch.alloc_as<T>(host.size() * sizeof(T) + 16);
    if (!d) return ctx->fail(NLX_E_NOMEM, "PLONK setup: device memory");
    if (!host.empty()) NLX_HIP(ctx, hipMemcpyAsync(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));   // `host` outlives the call's last synchronise
    *out = d;
    return NLX_OK;
}
inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

int32_t setup_body(nlx_ctx* ctx, Scratch& scratch, const nlx_bn254_plonk_setup_desc* d, const Checked& c, PSetup& s) {
    using namespace nlx::pls;
    hipStream_t st = ctx->stream;
    const uint32_t log_n = s.log_n, k = s.k;
    const size_t n = (size_t)1 << log_n, total = 3 * n;
    const size_t val_bytes = (size_t)(8 + k) * n * 32;
    s.vals = (uint64_t*)ctx->alloc(val_bytes + 3 * total * 4);
    if (!s.vals) return ctx->fail(NLX_E_NOMEM, "PLONK setup: device memory for the trace of 2^%u rows", log_n);
    s.cells = (uint32_t*)((uint8_t*)s.vals + val_bytes);
    s.perm = s.cells + total;
    s.sigma_cells = s.perm + total;
    int end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) < s.n_variables) end_bit++;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)total, 0, end_bit, (hipStream_t)nullptr);
    if (!tmp_bytes) tmp_bytes = 16;
    const uint32_t half = (log_n + 1) / 2, n_lo = 1u << half, n_hi = 1u << (log_n - half);
    void* d_tmp = scratch.alloc(tmp_bytes);
    uint32_t* d_iota = scratch.alloc_as<uint32_t>(total * 4);
    uint32_t* d_keys = scratch.alloc_as<uint32_t>(total * 4);
    uint32_t* d_pos = scratch.alloc_as<uint32_t>(total * 4);
    uint32_t* d_last = scratch.alloc_as<uint32_t>((size_t)s.n_variables * 4);
    ClassStats* d_stats = scratch.alloc_as<ClassStats>(sizeof(ClassStats));
    uint64_t* d_tab = scratch.alloc_as<uint64_t>((size_t)(n_lo + n_hi) * 32);
    if (!d_tmp || !d_iota || !d_keys || !d_pos || !d_last || !d_stats || !d_tab) return ctx->fail(NLX_E_NOMEM, "PLONK setup: device memory");

    RowsParams rp{};
    NLX_RC(on_device(ctx, scratch, d->xa, c.x[0], &rp.xa));
    NLX_RC(on_device(ctx, scratch, d->xb, c.x[1], &rp.xb));
    NLX_RC(on_device(ctx, scratch, d->xc, c.x[2], &rp.xc));
    const uint32_t* q[5] = {d->ql, d->qr, d->qm, d->qo, d->qk};
    for (int i = 0; i < 5; i++) NLX_RC(on_device(ctx, scratch, q[i], c.sel[i], &rp.sel[i]));
    NLX_RC(on_device(ctx, scratch, d->coeffs, c.coeffs, &rp.coeffs));
    NLX_RC(on_device(ctx, scratch, (const uint32_t*)nullptr, s.committed_rows, &rp.committed_rows));
    for (uint32_t j = 0; j < k; j++) rp.seg[j + 1] = rp.seg[j] + (uint32_t)s.counts[j];
    rp.n_public = s.n_public, rp.n_used = s.n_public + s.n_constraints;
    rp.log_n = log_n, rp.k = k;
    rp.vals = s.vals, rp.cells = s.cells, rp.iota = d_iota;
    ctx->begin_kernel("bn254_plonk_setup_rows", (double)(5 + k) * n * 32 + 24.0 * n);
    hipLaunchKernelGGL(k_pls_rows, dim3(blocks_of(n)), dim3(256), 0, st, rp);
    ctx->end_kernel();

    ctx->begin_kernel("bn254_plonk_setup_sort", 16.0 * total);
    const hipError_t se = hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, (const uint32_t*)s.cells, d_keys, (const uint32_t*)d_iota, d_pos, (int)total, 0, end_bit, st);
    ctx->end_kernel();
    if (se != hipSuccess) return ctx->hip_fail(se, "hipcub::DeviceRadixSort::SortPairs");

    NLX_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(ClassStats), st));
    ctx->begin_kernel("bn254_plonk_setup_perm", 24.0 * total);
    hipLaunchKernelGGL(k_pls_class_ends, dim3(blocks_of(total)), dim3(256), 0, st, d_keys, total, d_last);
    hipLaunchKernelGGL(k_pls_perm, dim3(blocks_of(total) < PERM_MAX_BLOCKS ? blocks_of(total) : PERM_MAX_BLOCKS), dim3(256), 0, st, d_keys, d_pos, total, d_last, s.perm, d_stats);
    ctx->end_kernel();

    SigmaParams sp{};
    sp.k[0] = bnf::one<bnf::RP>(), sp.k[1] = bnf::load_words<bnf::RP>(s.k1), sp.k[2] = bnf::load_words<bnf::RP>(s.k2);
    sp.perm = s.perm, sp.lo = d_tab, sp.hi = d_tab + (size_t)n_lo * 4;
    sp.log_n = log_n, sp.half = half;
    sp.sigma = s.vals + (size_t)5 * n * 4, sp.sigma_cells = s.sigma_cells;
    const Fr w = bnf::pow_host(bnf::root28(), (uint64_t)1 << (28 - log_n));
    ctx->begin_kernel("bn254_plonk_setup_sigma", 40.0 * total);
    hipLaunchKernelGGL(k_pls_root_tables, dim3(blocks_of(n_lo + n_hi)), dim3(256), 0, st, w, bnf::pow_host(w, (uint64_t)1 << half), n_lo, n_hi, d_tab,
                       d_tab + (size_t)n_lo * 4);
    hipLaunchKernelGGL(k_pls_sigma, dim3(blocks_of(total)), dim3(256), 0, st, sp);
    ctx->end_kernel();

    ClassStats stats;
    NLX_RC(fetch(ctx, &stats, d_stats, sizeof stats));
    s.occurring = stats.occurring, s.longest = stats.longest;
    return NLX_OK;
}

int32_t wires_body(nlx_ctx* ctx, const PSetup& s, const uint64_t* values, uint64_t* l, uint64_t* r, uint64_t* o) {
    const size_t n = (size_t)1 << s.log_n;
    Staged sv(ctx, values, (size_t)s.n_variables * 32, true, false);
    Staged sl(ctx, l, n * 32, false, true), sr(ctx, r, n * 32, false, true), so(ctx, o, n * 32, false, true);
    for (const Staged* t : {&sv, &sl, &sr, &so})
        if (t->status) return t->status;
    ctx->begin_kernel("bn254_plonk_setup_wires", 3.0 * n * 68);
    hipLaunchKernelGGL(pls::k_pls_wires, dim3(blocks_of(3 * n)), dim3(256), 0, ctx->stream, s.cells, s.log_n, sv.as<uint64_t>(), sl.as<uint64_t>(),
                       sr.as<uint64_t>(), so.as<uint64_t>());
    ctx->end_kernel();
    NLX_RC(sl.finish());
    NLX_RC(sr.finish());
    NLX_RC(so.finish());
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the copies out are done before the staged blocks go back
    NLX_HIP(ctx, hipGetLastError());
    return NLX_OK;
}

int32_t srs_body(nlx_ctx* ctx, Scratch& scratch, const Fr& tau, uint64_t n, uint64_t* g1_out, uint64_t* g2_out) {
    Staged so(ctx, g1_out, (size_t)n * 64, false, true);
    if (so.status) return so.status;
    uint32_t n_bits = 0;
    while (n_bits < 27 && ((uint64_t)1 << n_bits) < n) n_bits++;
    std::vector<uint64_t> tab((size_t)(n_bits + 2) * 4);   // tau^(2^b), b < n_bits | the G2 pair's scalars: 1, tau
    Fr t = tau;
    for (uint32_t b = 0; b < n_bits; b++, t = bnf::sqr(t)) bnf::store_words(t, &tab[4 * b]);
    bnf::store_words(bnf::one<bnf::RP>(), &tab[4 * n_bits]);
    bnf::store_words(tau, &tab[4 * (n_bits + 1)]);
    uint64_t* d_tab = scratch.alloc_as<uint64_t>(tab.size() * 8);
    uint64_t* d_scalars = scratch.alloc_as<uint64_t>((size_t)n * 32);
    uint64_t* d_g2 = scratch.alloc_as<uint64_t>(2 * 128);
    void* d_table1 = scratch.alloc(fixed_base::table_bytes(0));
    void* d_table2 = g2_out ? scratch.alloc(fixed_base::table_bytes(1)) : nullptr;
    if (!d_tab || !d_scalars || !d_g2 || !d_table1 || (g2_out && !d_table2)) return ctx->fail(NLX_E_NOMEM, "KZG SRS of %llu points: device memory", (unsigned long long)n);
    NLX_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));   // the scratch drains before `tab` goes
    ctx->begin_kernel("bn254_kzg_srs_powers", 32.0 * (double)n, (double)n);
    hipLaunchKernelGGL(pls::k_pls_tau_powers, dim3(blocks_of((size_t)n)), dim3(256), 0, ctx->stream, d_tab, n_bits, (size_t)n, d_scalars);
    ctx->end_kernel();
    NLX_RC(fixed_base::build_table(ctx, scratch, fixed_base::G1_GEN, 0, d_table1));
    NLX_RC(fixed_base::run(ctx, scratch, d_table1, d_scalars, (size_t)n, 1, 0, so.as<uint64_t>()));
    if (g2_out) {
        NLX_RC(fixed_base::build_table(ctx, scratch, fixed_base::G2_GEN, 1, d_table2));
        NLX_RC(fixed_base::run(ctx, scratch, d_table2, d_tab + 4 * (size_t)n_bits, 2, 1, 1, d_g2));
    }
    NLX_RC(so.finish());
    if (g2_out) NLX_RC(fetch(ctx, g2_out, d_g2, 2 * 128));
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the copy-out is done before `so` gives its block back
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_plonk_setup(nlx_ctx* ctx, const nlx_bn254_plonk_setup_desc* desc, struct nlx_bn254_plonk_setup** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<PSetup, void (*)(PSetup*)> s(new PSetup, setup_free);
    Checked checked;
    NLX_RC(load_and_check(ctx, desc, *s, checked));   // nothing of the device is held yet
    int32_t rc;
    {
        Scratch scratch(ctx);
        rc = scratch.finish(setup_body(ctx, scratch, desc, checked, *s));
    }
    if (rc) return rc;   // setup_free gives the block back
    s->nonzero.assign((size_t)s->n_constraints, 0);
    for (int i = 0; i < 5; i++)
        for (size_t t = 0; t < s->nonzero.size(); t++)
            s->nonzero[t] |= (uint8_t)((bnf::is_zero(bnf::load_words<bnf::RP>(&checked.coeffs[4 * (size_t)checked.sel[i][t]])) ? 0 : 1) << i);
    for (int i = 0; i < 3; i++) s->x[i] = std::move(checked.x[i]);
    *out = s.release();
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_plonk_setup_destroy(struct nlx_bn254_plonk_setup* setup) NLX_TRY {
    setup_free(setup);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_plonk_setup_info(const struct nlx_bn254_plonk_setup* setup, uint64_t out[NLX_BN254_PLONK_SETUP_INFO_WORDS]) NLX_TRY {
    if (!setup || !out) return NLX_E_INVAL;
    const uint64_t v[NLX_BN254_PLONK_SETUP_INFO_WORDS] = {(uint64_t)1 << setup->log_n, setup->log_n, setup->k, setup->n_public + setup->n_constraints,
                                                          setup->occurring, setup->longest};
    memcpy(out, v, sizeof v);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" int32_t nlx_bn254_plonk_setup_read(const struct nlx_bn254_plonk_setup* setup, uint32_t which, void* out) NLX_TRY {
    if (!setup) return NLX_E_INVAL;
    nlx_ctx* ctx = setup->ctx;
    const PSetup& s = *setup;
    const size_t n = (size_t)1 << s.log_n;
    const void* src = nullptr;
    size_t bytes = 3 * n * 4;
    if (which < NLX_PLONK_SETUP_QCP0 + s.k) src = s.vals + (size_t)which * n * 4, bytes = n * 32;
    else if (which == NLX_PLONK_SETUP_CELLS) src = s.cells;
    else if (which == NLX_PLONK_SETUP_PERMUTATION) src = s.perm;
    else if (which == NLX_PLONK_SETUP_SIGMA_CELLS) src = s.sigma_cells;
    else return ctx->fail(NLX_E_RANGE, "unknown array %u (the setup carries %u commitments)", which, s.k);
    if (!out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    (void)hipSetDevice(ctx->device);
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    NLX_HIP(ctx, hipMemcpy(out, src, bytes, hipMemcpyDefault));
    return NLX_OK;
} NLX_CATCH(setup ? setup->ctx : nullptr)

extern "C" int32_t nlx_bn254_plonk_setup_key(const struct nlx_bn254_plonk_setup* setup, const uint64_t* srs, uint64_t n_srs, uint32_t key_flags,
                                             nlx_bn254_plonk_key** out) NLX_TRY {
    if (!setup) return NLX_E_INVAL;
    nlx_ctx* ctx = setup->ctx;
    if (!out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    if (key_flags & ~(uint32_t)NLX_BN254_PLONK_KEY_COSET) return ctx->fail(NLX_E_RANGE, "key_flags: 0 or NLX_BN254_PLONK_KEY_COSET");
    const PSetup& s = *setup;
    const size_t n = (size_t)1 << s.log_n;
    nlx_bn254_plonk_key_desc d{};
    d.log_n = s.log_n, d.flags = NLX_BN254_MONTGOMERY | key_flags;
    const uint64_t** fixed[8] = {&d.ql, &d.qr, &d.qm, &d.qo, &d.qk, &d.s1, &d.s2, &d.s3};
    for (int i = 0; i < 8; i++) *fixed[i] = s.vals + (size_t)i * n * 4;
    d.k1 = s.k1, d.k2 = s.k2, d.coset_shift = s.shift;
    d.srs = srs, d.n_srs = n_srs;
    d.n_commit = s.k;
    const uint64_t* qcp[NLX_BN254_PLONK_MAX_COMMIT] = {};
    for (uint32_t j = 0; j < s.k; j++) qcp[j] = s.vals + (size_t)(8 + j) * n * 4;
    if (s.k) {
        d.qcp = qcp;
        d.n_committed = s.counts.data(), d.committed_rows = s.committed_rows.data(), d.commit_rows = s.commit_rows.data();
        d.last_row = (uint32_t)(s.n_public + s.n_constraints - 1);
    }
    nlx_bn254_plonk_key* key = nullptr;
    NLX_RC(nlx_bn254_plonk_key_create(ctx, &d, &key));
    // the permutation, already decoded: the key's first copy check finds its cells
    uint32_t* cells = (uint32_t*)ctx->alloc(3 * n * 4);
    hipError_t e = cells ? hipMemcpy(cells, s.sigma_cells, 3 * n * 4, hipMemcpyDeviceToDevice) : hipErrorOutOfMemory;
    if (e != hipSuccess) {
        if (cells) ctx->release(cells);
        nlx_bn254_plonk_key_destroy(key);
        return ctx->hip_fail(e, "the key's sigma cells");
    }
    key->sigma_cells = cells;
    *out = key;
    return NLX_OK;
} NLX_CATCH(setup ? setup->ctx : nullptr)

extern "C" int32_t nlx_bn254_plonk_setup_wires(nlx_ctx* ctx, const struct nlx_bn254_plonk_setup* setup, const uint64_t* values, uint64_t* l, uint64_t* r,
                                               uint64_t* o) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!setup || !values || !l || !r || !o) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (setup->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the setup belongs to another context");
    (void)hipSetDevice(ctx->device);
    return wires_body(ctx, *setup, values, l, r, o);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_kzg_srs(nlx_ctx* ctx, const uint64_t* tau, uint64_t n, uint64_t* g1_out, uint64_t* g2_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!tau) return ctx->fail(NLX_E_INVAL, "NULL argument");
    (void)hipSetDevice(ctx->device);
    if (is_device_ptr(tau) || (g2_out && is_device_ptr(g2_out))) return ctx->fail(NLX_E_INVAL, "tau and g2_out are host values");
    if (!bnf::below_mod<bnf::RP>(tau)) return ctx->fail(NLX_E_RANGE, "tau is not below r");
    const Fr t = bnf::load_words<bnf::RP>(tau);
    if (bnf::is_zero(t)) return ctx->fail(NLX_E_RANGE, "tau is zero");
    if (n == 0 || n > fixed_base::MAX_SCALARS) return ctx->fail(NLX_E_RANGE, "n = %llu: an SRS holds 1 .. 2^27 points", (unsigned long long)n);
    if (!g1_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    Scratch scratch(ctx);
    return scratch.finish(srs_body(ctx, scratch, t, n, g1_out, g2_out));
} NLX_CATCH(ctx)
