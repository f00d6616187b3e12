// Row f.4, the Groth16 half: whole proofs from a proving key resident in HBM.
//
// What gnark's backend/groth16/bn254 `Prove` does after its solver (Go, not in the reference; restated from the published
// protocol - Groth, "On the Size of Pairing-based Non-interactive Arguments" - and gnark's ProvingKey layout as recalled, parity
// with gnark-produced bytes UNPINNED):
//   a, b, c = A w, B w, C w on H              k_r1cs_rows / k_r1cs_long_rows below (or the solver's values, handed in)
//   h = (a b - c) / Z_H                       nlx_bn254_groth16_quotient (bn254_plonk.hip), device-resident
//   Ar  = sum_i w_i A_i + alpha + r delta                                   G1.A  } the four queries over the wire vector:
//   Bs1 = sum_i w_i B_i + beta + s delta (G1), Bs the same sum in G2        G1.B, G2.B  } ONE digit decomposition and ONE set
//   Krs = sum_private w_i K_i + sum_(i < n-1) h_i Z_i + s Ar + r Bs1 - r s delta    G1.K } of sorted indices (bn254_msm.hpp)
// The key's queries are converted to the bucket kernels' form once, at creation, and - filtered of their points at infinity
// in gnark's layout - expanded to the wires' index space ((0, 0) at masked and public positions), which is what lets them
// share the sorted indices: the bucket kernels skip the point at infinity.
//
// The SpMV: one lane per row for rows of at most R1CS_LONG_ROW terms, one wave per row above that (partial sums joined by
// shuffles); coefficients equal to 1 or -1 are marked when the key is built and cost an addition or a subtraction.  Fr in
// Montgomery form on bn254_fp.hpp's eight 32-bit limbs; the witness gather (32 bytes per term) is the random-access stream.
//
// Keys with Bsb22 / Pedersen commitments (rules: tools/groth16_commit_model.py): the committed wires and
// the commitment wires hold the point at infinity in the expanded G1.K, so Krs needs nothing new; the two Pedersen bases stay
// compact (M points each, concatenated over the k commitments) next to the committed wire ids.  k_g16_gather_scale gathers the
// M committed values once per proof into a plain and a rho^j-scaled compact vector: C_j is an MSM over a slice of the first
// and Basis, Pok ONE MSM over the second and BasisExpSigma.
#include <cstring>
#include <vector>
#include "bn254_fp.hpp"
#include "bn254_msm.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace g16 {

using namespace bnf;
typedef Fp<RP> Fr;

constexpr uint32_t R1CS_LONG_ROW = 64;     // rows with more terms than this go one per wave
// Decompositions of the wire vector per proof: 1 - the four wire queries share one set of sorted digits.  A tuning build with
// -DNLX_GROTH16_INDEPENDENT_SORT (build.py: NLX_BUILD_VARIANT / NLX_EXTRA_FLAGS) sorts once per query: the A/B of DESIGN.md section 19.
#ifdef NLX_GROTH16_INDEPENDENT_SORT
constexpr int G16_WIRE_SORTS = 4;
#else
constexpr int G16_WIRE_SORTS = 1;
#endif
constexpr uint32_t TERM_ID_BITS = 30, TERM_ID_MASK = (1u << TERM_ID_BITS) - 1;
constexpr uint32_t TERM_GENERAL = 0, TERM_PLUS = 1, TERM_MINUS = 2;   // bits 30..31 of a term's code

struct R1csDev {
    const uint32_t* row_ptr[3];   // [n_constraints + 1]
    const uint32_t* wire[3];      // [nnz]
    const uint32_t* code[3];      // [nnz] kind << 30 | coefficient id
    const uint64_t* coeffs;       // [n_coeffs][4] Montgomery
    uint32_t log_n, n_constraints;
};

__device__ __forceinline__ Fr term(const R1csDev& p, int m, uint32_t k, const uint64_t* __restrict__ witness, const Fr& acc) {
    const uint32_t code = p.code[m][k];
    const Fr w = load<RP>(witness, p.wire[m][k]);
    const uint32_t kind = code >> TERM_ID_BITS;
    if (kind == TERM_PLUS) return add(acc, w);
    if (kind == TERM_MINUS) return sub(acc, w);
    return add(acc, mul(w, load<RP>(p.coeffs, code & TERM_ID_MASK)));
}

// lane t = matrix (t >> log_n), row (t & (N - 1)); rows past n_constraints are zero; long rows are the other kernel's
__global__ __launch_bounds__(256) void k_r1cs_rows(R1csDev p, const uint64_t* __restrict__ witness, uint64_t* __restrict__ out /* [3][N][4] */) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)1 << p.log_n;
    if (t >= 3 * n) return;
    const int m = (int)(t >> p.log_n);
    const uint32_t row = (uint32_t)(t & (n - 1));
    Fr acc = zero<RP>();
    if (row < p.n_constraints) {
        const uint32_t lo = p.row_ptr[m][row], hi = p.row_ptr[m][row + 1];
        if (hi - lo > R1CS_LONG_ROW) return;
#pragma unroll 1
        for (uint32_t k = lo; k < hi; k++) acc = term(p, m, k, witness, acc);
    }
    store(out, t, acc);
}
// one wave per long row: long_rows[j] = matrix << 30 | row
__global__ __launch_bounds__(256) void k_r1cs_long_rows(R1csDev p, const uint32_t* __restrict__ long_rows, uint32_t n_long,
                                                        const uint64_t* __restrict__ witness, uint64_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (j >= n_long) return;   // whole waves leave together
    const int m = (int)(long_rows[j] >> 30);
    const uint32_t row = long_rows[j] & ((1u << 30) - 1);
    const uint32_t lo = p.row_ptr[m][row], hi = p.row_ptr[m][row + 1];
    Fr acc = zero<RP>();
#pragma unroll 1
    for (uint32_t k = lo + lane; k < hi; k += 64) acc = term(p, m, k, witness, acc);
#pragma unroll 1
    for (int d = 32; d > 0; d >>= 1) {
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.v[i] = (uint32_t)__shfl_down((int)acc.v[i], d, 64);
        acc = add(acc, o);
    }
    if (lane == 0) store(out, ((size_t)m << p.log_n) + row, acc);
}

// a_i b_i = c_i on H: the first failing row (atomicMin over the waves that saw one)
__global__ __launch_bounds__(256) void k_g16_check(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                                                   size_t n, uint32_t* __restrict__ first_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = i < n && !equal(mul(load<RP>(a, i), load<RP>(b, i)), load<RP>(c, i));
    if (bad) atomicMin(first_bad, (uint32_t)i);
}

// The committed values, compact: lane t < m loads its wire id, then w[id] (the random 32-byte stream: two 16-byte loads), and
// stores it to plain[t] and, times rho^j, to scaled[t] (NULL: not wanted).  j = the number of segment ends at or below t - an
// empty set repeats an end; ends past the last commitment equal m.  rho^0 = 1: a plain copy.
struct CommitSegments {
    uint32_t end[NLX_BN254_GROTH16_MAX_COMMITMENTS];
    Fr rho_pow[NLX_BN254_GROTH16_MAX_COMMITMENTS];   // Montgomery; [0] is not read
};
__global__ __launch_bounds__(256) void k_g16_gather_scale(const uint32_t* __restrict__ ids, uint32_t m, const uint64_t* __restrict__ witness,
                                                          CommitSegments seg, uint64_t* __restrict__ plain, uint64_t* __restrict__ scaled) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    Fr w = load<RP>(witness, ids[t]);
    store(plain, t, w);
    if (!scaled) return;
    int j = 0;
#pragma unroll
    for (int i = 0; i < NLX_BN254_GROTH16_MAX_COMMITMENTS - 1; i++) j += t >= seg.end[i];
    if (j) {
        Fr p = seg.rho_pow[1];
#pragma unroll
        for (int i = 2; i < NLX_BN254_GROTH16_MAX_COMMITMENTS; i++)   // static indices: the table stays in scalar registers
            if (j == i) p = seg.rho_pow[i];
        w = mul(w, p);
    }
    store(scaled, t, w);
}

}  // namespace g16
}  // namespace nlx

using namespace nlx;

struct nlx_bn254_groth16_key {
    nlx_ctx* ctx = nullptr;
    uint32_t log_n = 0;
    uint64_t n_wires = 0, n_public = 0, n_constraints = 0;
    // the queries in the bucket kernels' form; a, b1, b2, k over the wires' index space, z over i < n - 1
    void *a = nullptr, *b1 = nullptr, *b2 = nullptr, *k = nullptr, *z = nullptr;
    uint64_t alpha1[8], beta1[8], delta1[8], beta2[16], delta2[16];
    // the R1CS (optional)
    bool has_r1cs = false;
    g16::R1csDev r1cs{};
    uint32_t* long_rows = nullptr;
    // Bsb22 / Pedersen commitments (n_commit = 0: none): set j's entries are [seg[j], seg[j + 1]) of the compact arrays
    uint32_t n_commit = 0;
    uint64_t n_committed = 0;                                    // M
    uint32_t seg[NLX_BN254_GROTH16_MAX_COMMITMENTS + 1] = {};
    const uint32_t* committed_ids = nullptr;                     // [M] wire ids, device
    void *basis = nullptr, *basis_sigma = nullptr;               // [M] each, the bucket kernels' form
    std::vector<void*> blocks;     // every device block the key owns
    uint64_t info[NLX_BN254_GROTH16_KEY_INFO_WORDS] = {};
};

namespace {

// the caller's array on the host, wherever it lies
template <class T>
int32_t to_host(nlx_ctx* ctx, const T* p, size_t count, std::vector<T>& out) {
    out.resize(count);
    if (!count) return NLX_OK;
    if (!is_device_ptr(p)) {
        memcpy(out.data(), p, count * sizeof(T));
        return NLX_OK;
    }
    NLX_HIP(ctx, hipMemcpy(out.data(), p, count * sizeof(T), hipMemcpyDeviceToHost));
    return NLX_OK;
}

void key_free(nlx_bn254_groth16_key* key) {
    if (!key) return;
    if (key->ctx) {
        (void)hipStreamSynchronize(key->ctx->stream);
        for (void* p : key->blocks) key->ctx->release(p);
    }
    delete key;
}

// a device block owned by the key, filled from a host vector
template <class T>
int32_t key_upload(nlx_bn254_groth16_key* key, const std::vector<T>& v, const T** out) {
    nlx_ctx* ctx = key->ctx;
    void* d = ctx->alloc(v.size() * sizeof(T) + 16);
    if (!d) return NLX_E_NOMEM;
    key->blocks.push_back(d);
    if (!v.empty()) NLX_HIP(ctx, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)d;
    return NLX_OK;
}

// one query: the caller's filtered points -> converted, expanded through `index` (n_out entries) when there is one
int32_t key_query(nlx_bn254_groth16_key* key, const uint64_t* points, uint64_t count, const std::vector<uint32_t>* index, size_t n_out, int g2,
                  void** out) {
    nlx_ctx* ctx = key->ctx;
    const size_t in_bytes = (size_t)count * (g2 ? 128 : 64);
    void* d = ctx->alloc(n_out * msm::converted_point_bytes(g2) + 16);
    if (!d) return NLX_E_NOMEM;
    key->blocks.push_back(d);
    *out = d;
    key->info[0] += n_out * msm::converted_point_bytes(g2);
    if (!n_out) return NLX_OK;
    if (!count) {   // every position masked: the point at infinity is all-zero words in the kernels' form too
        NLX_HIP(ctx, hipMemset(d, 0, n_out * msm::converted_point_bytes(g2)));
        return NLX_OK;
    }
    Staged sp(ctx, points, in_bytes, true, false);
    if (sp.status) return sp.status;
    uint32_t* d_index = nullptr;
    if (index) {
        d_index = (uint32_t*)ctx->alloc(n_out * 4);
        if (!d_index) return NLX_E_NOMEM;
        hipError_t e = hipMemcpy(d_index, index->data(), n_out * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            ctx->release(d_index);
            return ctx->hip_fail(e, "hipMemcpy");
        }
    }
    msm::convert_points(ctx, sp.as<uint64_t>(), d_index, n_out, g2, d);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (d_index) ctx->release(d_index);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipStreamSynchronize");
    return NLX_OK;
}

int32_t key_r1cs(nlx_bn254_groth16_key* key, const nlx_bn254_groth16_key_desc* d) {
    nlx_ctx* ctx = key->ctx;
    const uint64_t nc = d->n_constraints;
    if (d->n_coeffs == 0 || d->n_coeffs > g16::TERM_ID_MASK) return ctx->fail(NLX_E_RANGE, "the coefficient table holds 1 .. 2^30 - 1 entries");
    std::vector<uint64_t> coeffs;
    int32_t rc = to_host(ctx, d->coeffs, (size_t)d->n_coeffs * 4, coeffs);
    if (rc) return rc;
    uint64_t ONE[4], MINUS_ONE[4];   // fr.Element words of 1 and -1
    store_words(bnf::one<bnf::RP>(), ONE);
    store_words(bnf::neg(bnf::one<bnf::RP>()), MINUS_ONE);
    std::vector<uint8_t> kind((size_t)d->n_coeffs);
    for (uint64_t i = 0; i < d->n_coeffs; i++) {
        if (!bnf::below_mod<bnf::RP>(&coeffs[4 * i])) return ctx->fail(NLX_E_RANGE, "coefficient %llu is not below r", (unsigned long long)i);
        kind[i] = !memcmp(&coeffs[4 * i], ONE, 32) ? g16::TERM_PLUS : !memcmp(&coeffs[4 * i], MINUS_ONE, 32) ? g16::TERM_MINUS : g16::TERM_GENERAL;
    }
    rc = key_upload(key, coeffs, &key->r1cs.coeffs);
    if (rc) return rc;
    key->info[0] += coeffs.size() * 8;
    std::vector<uint32_t> long_rows;
    uint64_t n_short = 0, n_unit = 0, nnz_all = 0;
    const uint64_t* rp[3] = {d->a_row_ptr, d->b_row_ptr, d->c_row_ptr};
    const uint32_t* wi[3] = {d->a_wire, d->b_wire, d->c_wire};
    const uint32_t* ci[3] = {d->a_coeff_id, d->b_coeff_id, d->c_coeff_id};
    for (int m = 0; m < 3; m++) {
        if (!rp[m] || !wi[m] || !ci[m]) return ctx->fail(NLX_E_INVAL, "NULL argument (the three matrices come together)");
        std::vector<uint64_t> row_ptr;
        rc = to_host(ctx, rp[m], (size_t)nc + 1, row_ptr);
        if (rc) return rc;
        if (row_ptr[0] != 0) return ctx->fail(NLX_E_RANGE, "matrix %d: row pointers do not start at 0", m);
        for (uint64_t r = 0; r < nc; r++)
            if (row_ptr[r + 1] < row_ptr[r]) return ctx->fail(NLX_E_RANGE, "matrix %d: row pointers decrease at row %llu", m, (unsigned long long)r);
        const uint64_t nnz = row_ptr[nc];
        if (nnz >= ((uint64_t)1 << 32)) return ctx->fail(NLX_E_RANGE, "matrix %d: at most 2^32 - 1 terms", m);
        std::vector<uint32_t> wire, cid, rp32((size_t)nc + 1);
        rc = to_host(ctx, wi[m], (size_t)nnz, wire);
        if (!rc) rc = to_host(ctx, ci[m], (size_t)nnz, cid);
        if (rc) return rc;
        for (uint64_t k = 0; k < nnz; k++) {
            if (wire[k] >= d->n_wires) return ctx->fail(NLX_E_RANGE, "matrix %d, term %llu: wire %u of %llu", m, (unsigned long long)k, wire[k], (unsigned long long)d->n_wires);
            if (cid[k] >= d->n_coeffs) return ctx->fail(NLX_E_RANGE, "matrix %d, term %llu: coefficient %u of %llu", m, (unsigned long long)k, cid[k], (unsigned long long)d->n_coeffs);
            n_unit += kind[cid[k]] != g16::TERM_GENERAL;
            cid[k] |= (uint32_t)kind[cid[k]] << g16::TERM_ID_BITS;
        }
        for (uint64_t r = 0; r <= nc; r++) rp32[r] = (uint32_t)row_ptr[r];
        for (uint64_t r = 0; r < nc; r++) {
            if (rp32[r + 1] - rp32[r] > g16::R1CS_LONG_ROW) long_rows.push_back((uint32_t)m << 30 | (uint32_t)r);
            else n_short++;
        }
        nnz_all += nnz;
        rc = key_upload(key, rp32, &key->r1cs.row_ptr[m]);
        if (!rc) rc = key_upload(key, wire, &key->r1cs.wire[m]);
        if (!rc) rc = key_upload(key, cid, &key->r1cs.code[m]);
        if (rc) return rc;
        key->info[0] += (nc + 1) * 4 + nnz * 8;
    }
    const uint32_t* d_long = nullptr;
    rc = key_upload(key, long_rows, &d_long);
    if (rc) return rc;
    key->long_rows = const_cast<uint32_t*>(d_long);
    key->info[0] += long_rows.size() * 4;
    key->r1cs.log_n = key->log_n;
    key->r1cs.n_constraints = (uint32_t)nc;
    key->info[1] = n_short, key->info[2] = long_rows.size(), key->info[3] = nnz_all, key->info[4] = n_unit;
    key->has_r1cs = true;
    return NLX_OK;
}

// enqueue the SpMV: d_out = [3][N][4]
void launch_r1cs(const nlx_bn254_groth16_key* key, const uint64_t* d_witness, uint64_t* d_out) {
    hipStream_t st = key->ctx->stream;
    const size_t n = (size_t)1 << key->log_n;
    hipLaunchKernelGGL(g16::k_r1cs_rows, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, key->r1cs, d_witness, d_out);
    const uint32_t n_long = (uint32_t)key->info[2];
    if (n_long) hipLaunchKernelGGL(g16::k_r1cs_long_rows, dim3((n_long + 3) / 4), dim3(256), 0, st, key->r1cs, key->long_rows, n_long, d_witness, d_out);
}

}  // namespace

// The committed sets of a key on the host, validated: ids within the private wires, ascending inside a set, the sets disjoint,
// the commitment wires private, not committed and distinct.  committed[i] != 0: wire i has left G1.K.
struct CommitHost {
    std::vector<uint64_t> counts;
    std::vector<uint32_t> ids, wires;
    std::vector<uint8_t> committed;
    uint64_t m = 0;
};
static int32_t commit_host(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* d, const nlx_bn254_groth16_commit_desc* cd, CommitHost& h) {
    const uint32_t k = cd->n_commitments;
    if (!cd->n_private || !cd->commitment_wires) return ctx->fail(NLX_E_INVAL, "NULL argument");
    (void)hipSetDevice(ctx->device);
    int32_t rc = to_host(ctx, cd->n_private, (size_t)k, h.counts);
    if (!rc) rc = to_host(ctx, cd->commitment_wires, (size_t)k, h.wires);
    if (rc) return rc;
    for (uint32_t j = 0; j < k; j++) {
        if (h.counts[j] > d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u commits more wires than the key has", j);
        h.m += h.counts[j];
    }
    if (h.m + k > d->n_wires - d->n_public) return ctx->fail(NLX_E_RANGE, "more committed and commitment wires than private wires");
    if (h.m && (!cd->private_wires || !cd->basis || !cd->basis_exp_sigma)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    rc = to_host(ctx, cd->private_wires, (size_t)h.m, h.ids);
    if (rc) return rc;
    h.committed.assign((size_t)d->n_wires, 0);
    size_t t = 0;
    for (uint32_t j = 0; j < k; j++)
        for (uint64_t i = 0; i < h.counts[j]; i++, t++) {
            const uint32_t id = h.ids[t];
            if (id < d->n_public || id >= d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u: wire %u is not a private wire", j, id);
            if (i && id <= h.ids[t - 1]) return ctx->fail(NLX_E_RANGE, "commitment %u: the committed wire ids do not ascend at %u", j, id);
            if (h.committed[id]) return ctx->fail(NLX_E_RANGE, "commitment %u: wire %u is committed twice", j, id);
            h.committed[id] = 1;
        }
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t id = h.wires[j];
        if (id < d->n_public || id >= d->n_wires) return ctx->fail(NLX_E_RANGE, "commitment %u: its wire %u is not a private wire", j, id);
        if (h.committed[id]) return ctx->fail(NLX_E_RANGE, "commitment %u: its wire %u is committed or listed twice", j, id);
        h.committed[id] = 2;
    }
    return NLX_OK;
}

// both creation entries, past their own first checks; cd = NULL: a key without commitments
static int32_t key_build(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* d, const nlx_bn254_groth16_commit_desc* cd, nlx_bn254_groth16_key** out) {
    if (d->log_n < 1 || d->log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n must be in [1, 26]");
    const uint64_t n = (uint64_t)1 << d->log_n;
    if (d->n_constraints > n) return ctx->fail(NLX_E_RANGE, "n_constraints exceeds 2^log_n");
    if (d->n_wires < 1 || d->n_wires > ((uint64_t)1 << 27) || d->n_public < 1 || d->n_public > d->n_wires)
        return ctx->fail(NLX_E_RANGE, "1 <= n_public <= n_wires <= 2^27");
    if (!d->infinity_a || !d->infinity_b || !d->g1_alpha || !d->g1_beta || !d->g1_delta || !d->g2_beta || !d->g2_delta ||
        (d->n_g1_a && !d->g1_a) || (d->n_g1_b && !d->g1_b) || (d->n_g2_b && !d->g2_b) || (d->n_g1_k && !d->g1_k) || !d->g1_z)
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    CommitHost ch;
    if (cd) NLX_RC(commit_host(ctx, d, cd, ch));
    if (d->n_g1_k != d->n_wires - d->n_public - ch.m - (cd ? cd->n_commitments : 0))
        return ctx->fail(NLX_E_RANGE, cd ? "G1.K holds one point per private wire that is neither committed nor a commitment's" : "G1.K holds one point per private wire");
    if (d->n_g1_z != n - 1) return ctx->fail(NLX_E_RANGE, "G1.Z holds 2^log_n - 1 points");
    if (d->n_g2_b != d->n_g1_b) return ctx->fail(NLX_E_RANGE, "G1.B and G2.B are filtered by the same mask");
    (void)hipSetDevice(ctx->device);
    std::vector<uint8_t> mask_a, mask_b;
    int32_t rc = to_host(ctx, d->infinity_a, (size_t)d->n_wires, mask_a);
    if (!rc) rc = to_host(ctx, d->infinity_b, (size_t)d->n_wires, mask_b);
    if (rc) return rc;
    std::vector<uint32_t> idx_a((size_t)d->n_wires), idx_b((size_t)d->n_wires), idx_k((size_t)d->n_wires);
    uint64_t clear_a = 0, clear_b = 0, clear_k = 0;
    for (uint64_t i = 0; i < d->n_wires; i++) {
        idx_a[i] = mask_a[i] ? 0xFFFFFFFFu : (uint32_t)clear_a++;
        idx_b[i] = mask_b[i] ? 0xFFFFFFFFu : (uint32_t)clear_b++;
        idx_k[i] = (i < d->n_public || (cd && ch.committed[i])) ? 0xFFFFFFFFu : (uint32_t)clear_k++;
    }
    if (clear_a != d->n_g1_a) return ctx->fail(NLX_E_RANGE, "InfinityA leaves %llu wires, G1.A holds %llu points", (unsigned long long)clear_a, (unsigned long long)d->n_g1_a);
    if (clear_b != d->n_g1_b) return ctx->fail(NLX_E_RANGE, "InfinityB leaves %llu wires, G1.B holds %llu points", (unsigned long long)clear_b, (unsigned long long)d->n_g1_b);
    const bool any_matrix = d->a_row_ptr || d->b_row_ptr || d->c_row_ptr || d->coeffs;
    nlx_bn254_groth16_key* key = new nlx_bn254_groth16_key;
    key->ctx = ctx;
    key->log_n = d->log_n;
    key->n_wires = d->n_wires, key->n_public = d->n_public, key->n_constraints = d->n_constraints;
    const struct { const uint64_t* src; uint64_t* dst; size_t words; } singles[5] = {
        {d->g1_alpha, key->alpha1, 8}, {d->g1_beta, key->beta1, 8}, {d->g1_delta, key->delta1, 8}, {d->g2_beta, key->beta2, 16}, {d->g2_delta, key->delta2, 16}};
    for (const auto& s : singles) {
        hipError_t e = hipMemcpy(s.dst, s.src, s.words * 8, hipMemcpyDefault);
        if (e != hipSuccess && !rc) rc = ctx->hip_fail(e, "hipMemcpy");
    }
    if (!rc) rc = key_query(key, d->g1_a, d->n_g1_a, &idx_a, (size_t)d->n_wires, 0, &key->a);
    if (!rc) rc = key_query(key, d->g1_b, d->n_g1_b, &idx_b, (size_t)d->n_wires, 0, &key->b1);
    if (!rc) rc = key_query(key, d->g2_b, d->n_g2_b, &idx_b, (size_t)d->n_wires, 1, &key->b2);
    if (!rc) rc = key_query(key, d->g1_k, d->n_g1_k, &idx_k, (size_t)d->n_wires, 0, &key->k);
    if (!rc) rc = key_query(key, d->g1_z, d->n_g1_z, nullptr, (size_t)d->n_g1_z, 0, &key->z);
    if (!rc && cd) {   // the Pedersen bases, compact, and the committed wire ids next to them
        key->n_commit = cd->n_commitments;
        key->n_committed = ch.m;
        for (uint32_t j = 0; j < cd->n_commitments; j++) key->seg[j + 1] = key->seg[j] + (uint32_t)ch.counts[j];
        rc = key_query(key, cd->basis, ch.m, nullptr, (size_t)ch.m, 0, &key->basis);
        if (!rc) rc = key_query(key, cd->basis_exp_sigma, ch.m, nullptr, (size_t)ch.m, 0, &key->basis_sigma);
        if (!rc) rc = key_upload(key, ch.ids, &key->committed_ids);
        key->info[0] += ch.m * 4;
        key->info[6] = ch.m, key->info[7] = cd->n_commitments;
    }
    if (!rc && any_matrix) {
        if (!d->coeffs) rc = ctx->fail(NLX_E_INVAL, "NULL argument (the matrices come with their coefficient table)");
        else rc = key_r1cs(key, d);
    }
    if (!rc) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = ctx->hip_fail(e, "kernel launch");
    }
    if (rc) {
        key_free(key);
        return rc;
    }
    key->info[5] = g16::R1CS_LONG_ROW;
    *out = key;
    return NLX_OK;
}

extern "C" int32_t nlx_bn254_groth16_key_create(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* d, nlx_bn254_groth16_key** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!d || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    if (d->flags != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "flags must be NLX_BN254_MONTGOMERY");
    if (d->n_commitments)
        return ctx->fail(NLX_E_UNSUPPORTED, "a key with Bsb22 / Pedersen commitments brings its bases: nlx_bn254_groth16_key_create_committed");
    return key_build(ctx, d, nullptr, out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_groth16_key_create_committed(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* d, const nlx_bn254_groth16_commit_desc* cd,
                                                          nlx_bn254_groth16_key** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!d || !cd || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    if (d->flags != NLX_BN254_MONTGOMERY) return ctx->fail(NLX_E_RANGE, "flags must be NLX_BN254_MONTGOMERY");
    if (cd->n_commitments < 1 || cd->n_commitments > NLX_BN254_GROTH16_MAX_COMMITMENTS)
        return ctx->fail(NLX_E_RANGE, "1 .. %d commitments", NLX_BN254_GROTH16_MAX_COMMITMENTS);
    if (d->n_commitments != cd->n_commitments)
        return ctx->fail(NLX_E_RANGE, "the key descriptor counts %u commitments, the commitment descriptor %u", d->n_commitments, cd->n_commitments);
    return key_build(ctx, d, cd, out);
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_groth16_key_destroy(nlx_bn254_groth16_key* key) NLX_TRY {
    key_free(key);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_groth16_key_info(const nlx_bn254_groth16_key* key, uint64_t out[NLX_BN254_GROTH16_KEY_INFO_WORDS]) NLX_TRY {
    if (!key || !out) return NLX_E_INVAL;
    memcpy(out, key->info, sizeof key->info);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" int32_t nlx_bn254_r1cs_eval(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, uint64_t* a_out, uint64_t* b_out,
                                       uint64_t* c_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!key || !witness || !a_out || !b_out || !c_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (!key->has_r1cs) return ctx->fail(NLX_E_INVAL, "the key was built without its R1CS matrices");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << key->log_n;
    Staged sw(ctx, witness, (size_t)key->n_wires * 32, true, false);
    if (sw.status) return sw.status;
    uint64_t* d_abc = (uint64_t*)ctx->alloc(3 * n * 32);
    if (!d_abc) return NLX_E_NOMEM;
    ctx->begin_kernel("bn254_r1cs_eval", 40.0 * (double)key->info[3] + 96.0 * (double)n, (double)key->info[3]);
    launch_r1cs(key, sw.as<uint64_t>(), d_abc);
    ctx->end_kernel();
    uint64_t* outs[3] = {a_out, b_out, c_out};
    hipError_t e = hipSuccess;
    for (int m = 0; m < 3 && e == hipSuccess; m++)
        e = hipMemcpyAsync(outs[m], d_abc + (size_t)m * n * 4, n * 32, is_device_ptr(outs[m]) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    ctx->release(d_abc);
    if (e != hipSuccess) return ctx->hip_fail(e, "nlx_bn254_r1cs_eval");
    return NLX_OK;
} NLX_CATCH(ctx)

// The committed values gathered (and scaled by rho^j when `scaled` is wanted): entries [first, first + m) of the key's sets
static void launch_gather(const nlx_bn254_groth16_key* key, uint32_t first, uint32_t m, const uint64_t* d_witness, const g16::CommitSegments& seg,
                          uint64_t* d_plain, uint64_t* d_scaled) {
    hipLaunchKernelGGL(g16::k_g16_gather_scale, dim3((m + 255) / 256), dim3(256), 0, key->ctx->stream, key->committed_ids + first, m, d_witness, seg,
                       d_plain, d_scaled);
}

// One proof on either kind of key (the entries below have checked their own arguments).  rho = NULL: a key without
// commitments; otherwise the k commitments and Pok are computed as well (commitments_out: k x 8 words).
static int32_t prove_body(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, const uint64_t* a, const uint64_t* b,
                          const uint64_t* c, const uint64_t r[4], const uint64_t s[4], const uint64_t* rho, uint64_t ar_out[8], uint64_t bs_out[16],
                          uint64_t krs_out[8], uint64_t* commitments_out, uint64_t* pok_out) {
    using namespace nlx::msm;
    const bool given = a && b && c;
    if (!given && (a || b || c)) return ctx->fail(NLX_E_INVAL, "a, b, c come together or not at all");
    if (!given && !key->has_r1cs) return ctx->fail(NLX_E_INVAL, "a, b, c are NULL and the key was built without its R1CS matrices");
    if (is_device_ptr(r) || is_device_ptr(s)) return ctx->fail(NLX_E_INVAL, "r and s are host values");
    if (!bnf::below_mod<bnf::RP>(r) || !bnf::below_mod<bnf::RP>(s)) return ctx->fail(NLX_E_RANGE, "r or s is not below the group order");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << key->log_n, nw = (size_t)key->n_wires;
    Staged sw(ctx, witness, nw * 32, true, false);
    if (sw.status) return sw.status;
    const uint64_t* d_w = sw.as<uint64_t>();
    const uint32_t k = rho ? key->n_commit : 0, m = (uint32_t)key->n_committed;
    SortedDigits wires_sorted[g16::G16_WIRE_SORTS], h_sorted, commit_sorted[NLX_BN254_GROTH16_MAX_COMMITMENTS + 1];   // the last one: Pok
    struct ReleaseSorted {   // runs after `scratch` below (declared later, destroyed first) has synchronised the stream
        nlx_ctx* ctx;
        SortedDigits *wires, *h, *commit;
        ~ReleaseSorted() {
            for (int i = 0; i < g16::G16_WIRE_SORTS; i++) release_digits(ctx, wires + i);
            release_digits(ctx, h);
            for (int i = 0; i <= NLX_BN254_GROTH16_MAX_COMMITMENTS; i++) release_digits(ctx, commit + i);
        }
    } release_sorted{ctx, wires_sorted, &h_sorted, commit_sorted};
    Scratch scratch(ctx);
    auto dev = [&](size_t bytes) { return scratch.alloc(bytes); };
    uint64_t* d_abc = (uint64_t*)dev(3 * n * 32);
    uint64_t* d_h = (uint64_t*)dev(n * 32);
    uint32_t* d_bad = (uint32_t*)dev(64);
    void* d_buckets = dev(bucket_bytes(1));   // one block serves all five bucket passes (the stream runs them in order)
    const size_t wsum_bytes = (4 + (k ? k + 1 : 0)) * window_sum_bytes(0) + window_sum_bytes(1);   // then the k commitments' and Pok's
    unsigned char* d_wsum = (unsigned char*)dev(wsum_bytes);
    uint64_t* d_committed = k && m ? (uint64_t*)dev(2 * (size_t)m * 32) : nullptr;   // plain | scaled by rho^j
    if (!d_abc || !d_h || !d_bad || !d_buckets || !d_wsum || (k && m && !d_committed)) return ctx->fail(NLX_E_NOMEM, "Groth16 proof: device memory");
    // the solver's a, b, c, or the key's matrices times the witness
    hipError_t e = hipSuccess;
    if (given) {
        const uint64_t* in[3] = {a, b, c};
        for (int m = 0; m < 3 && e == hipSuccess; m++)
            e = hipMemcpyAsync(d_abc + (size_t)m * n * 4, in[m], n * 32, is_device_ptr(in[m]) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    } else {
        launch_r1cs(key, d_w, d_abc);
    }
    // w[0] = 1 and a o b = c before anything is committed: h has no spare coefficient that would betray a bad witness
    uint64_t w0[4];
    uint32_t first_bad = 0xFFFFFFFFu;
    if (e == hipSuccess) e = hipMemcpyAsync(d_bad, &first_bad, 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g16::k_g16_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_abc, d_abc + n * 4, d_abc + 2 * n * 4, n, d_bad);
        e = hipMemcpyAsync(&first_bad, d_bad, 4, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(w0, d_w, 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return ctx->hip_fail(e, "Groth16 proof: a, b, c");
    uint64_t ONE[4];
    store_words(bnf::one<RP>(), ONE);
    if (memcmp(w0, ONE, 32)) return ctx->fail(NLX_E_INVAL, "the witness does not start with the constant wire 1");
    if (first_bad != 0xFFFFFFFFu) return ctx->fail(NLX_E_INVAL, "the witness does not satisfy the circuit: a b != c at row %u", first_bad);
    // h, device-resident (gnark's domain generator 5 as the coset shift)
    Fr five = bnf::zero<RP>();
    five.v[0] = 5;
    uint64_t shift[4];
    store_words(to_mont(five), shift);
    int32_t rc = nlx_bn254_groth16_quotient(ctx, key->log_n, d_abc, d_abc + n * 4, d_abc + 2 * n * 4, shift, d_h);
    if (rc) return rc;
    // the MSMs: four queries over the wire vector on one set of sorted indices, G1.Z over h on its own
    const void* query[4] = {key->a, key->b1, key->b2, key->k};
    const int query_g2[4] = {0, 0, 1, 0};
    unsigned char* wsum_at[5 + NLX_BN254_GROTH16_MAX_COMMITMENTS + 1];
    {
        unsigned char* p = d_wsum;
        for (int q = 0; q < 4; q++) {
            wsum_at[q] = p;
            p += window_sum_bytes(query_g2[q]);
        }
        for (uint32_t q = 4; q < 5 + (k ? k + 1 : 0); q++, p += window_sum_bytes(0)) wsum_at[q] = p;
    }
    ctx->begin_kernel("bn254_groth16_msms", 32.0 * (double)(nw + n) + 320.0 * (double)nw + 64.0 * (double)n, (double)(4 * nw + n));
    for (int q = 0; q < 4 && !rc; q++) {
        if (q < g16::G16_WIRE_SORTS) rc = sort_digits(ctx, d_w, nw, 1, &wires_sorted[q]);
        if (!rc) bucket_reduce(ctx, wires_sorted[q < g16::G16_WIRE_SORTS ? q : 0], query[q], query_g2[q], d_buckets, wsum_at[q]);
    }
    if (!rc && n > 1) {
        rc = sort_digits(ctx, d_h, n - 1, 1, &h_sorted);
        if (!rc) bucket_reduce(ctx, h_sorted, key->z, 0, d_buckets, wsum_at[4]);
    }
    if (!rc && k && m) {
        // the committed values once, plain and scaled; then C_j over the slices of the plain vector and Basis, Pok over the
        // scaled vector and BasisExpSigma.  An empty set reaches no kernel: its C_j is the point at infinity.
        g16::CommitSegments seg;
        Fr power = bnf::one<RP>();
        const Fr rho_m = load_words<RP>(rho);
        for (uint32_t j = 0; j < NLX_BN254_GROTH16_MAX_COMMITMENTS; j++) {
            seg.end[j] = j < k ? key->seg[j + 1] : m;
            seg.rho_pow[j] = power;
            power = bnf::mul(power, rho_m);
        }
        launch_gather(key, 0, m, d_w, seg, d_committed, d_committed + (size_t)m * 4);
        for (uint32_t j = 0; j < k && !rc; j++) {
            const uint32_t lo = key->seg[j], count = key->seg[j + 1] - lo;
            if (!count) continue;
            rc = sort_digits(ctx, d_committed + (size_t)lo * 4, count, 1, &commit_sorted[j]);
            if (!rc) bucket_reduce(ctx, commit_sorted[j], (const unsigned char*)key->basis + (size_t)lo * converted_point_bytes(0), 0, d_buckets, wsum_at[5 + j]);
        }
        if (!rc) rc = sort_digits(ctx, d_committed + (size_t)m * 4, m, 1, &commit_sorted[k]);
        if (!rc) bucket_reduce(ctx, commit_sorted[k], key->basis_sigma, 0, d_buckets, wsum_at[5 + k]);
    }
    ctx->end_kernel();
    if (rc) return rc;
    std::vector<unsigned char> words(wsum_bytes);
    rc = fetch(ctx, words.data(), d_wsum, words.size());
    if (!rc) {
        e = hipGetLastError();
        if (e != hipSuccess) rc = ctx->hip_fail(e, "kernel launch");
    }
    if (rc) return rc;
    // the tail, on the host
    const size_t off1 = window_sum_bytes(0), off2 = 2 * off1, off3 = off2 + window_sum_bytes(1), off4 = off3 + off1;
    const JacH<H1> msm_a = window_tail_g1(words.data()), msm_b1 = window_tail_g1(words.data() + off1), msm_k = window_tail_g1(words.data() + off3);
    const JacH<H1> msm_z = n > 1 ? window_tail_g1(words.data() + off4) : hinf<H1>();
    const JacH<H2> msm_b2 = window_tail_g2(words.data() + off2);
    const Fr rk = from_mont(load_words<RP>(r)), sk = from_mont(load_words<RP>(s));
    const JacH<H1> delta1 = hload_affine<H1>(key->delta1), s_delta1 = hjmul<H1>(delta1, sk);
    const JacH<H1> ar = hjadd<H1>(hjadd<H1>(msm_a, hload_affine<H1>(key->alpha1)), hjmul<H1>(delta1, rk));
    const JacH<H1> bs1 = hjadd<H1>(hjadd<H1>(msm_b1, hload_affine<H1>(key->beta1)), s_delta1);
    const JacH<H2> bs = hjadd<H2>(hjadd<H2>(msm_b2, hload_affine<H2>(key->beta2)), hjmul<H2>(hload_affine<H2>(key->delta2), sk));
    JacH<H1> krs = hjadd<H1>(msm_k, msm_z);
    krs = hjadd<H1>(krs, hjmul<H1>(ar, sk));
    krs = hjadd<H1>(krs, hjmul<H1>(bs1, rk));
    krs = hjadd<H1>(krs, hjneg<H1>(hjmul<H1>(s_delta1, rk)));
    JacH<H1> commitment[NLX_BN254_GROTH16_MAX_COMMITMENTS], pok = hinf<H1>();
    for (uint32_t j = 0; j < k; j++)
        commitment[j] = key->seg[j + 1] > key->seg[j] ? window_tail_g1(words.data() + off4 + (1 + j) * off1) : hinf<H1>();
    if (k && m) pok = window_tail_g1(words.data() + off4 + (1 + k) * off1);
    hstore_affine<H1>(ar, ar_out);
    hstore_affine<H2>(bs, bs_out);
    hstore_affine<H1>(krs, krs_out);
    for (uint32_t j = 0; j < k; j++) hstore_affine<H1>(commitment[j], commitments_out + 8 * j);
    if (k) hstore_affine<H1>(pok, pok_out);
    return NLX_OK;
}

extern "C" int32_t nlx_bn254_groth16_prove(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, const uint64_t* a,
                                           const uint64_t* b, const uint64_t* c, const uint64_t r[4], const uint64_t s[4], uint64_t ar_out[8],
                                           uint64_t bs_out[16], uint64_t krs_out[8]) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!key || !witness || !r || !s || !ar_out || !bs_out || !krs_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (key->n_commit) return ctx->fail(NLX_E_INVAL, "the key carries commitments: its proofs come from nlx_bn254_groth16_prove_committed");
    return prove_body(ctx, key, witness, a, b, c, r, s, nullptr, ar_out, bs_out, krs_out, nullptr, nullptr);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_groth16_prove_committed(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, const uint64_t* a,
                                                     const uint64_t* b, const uint64_t* c, const uint64_t r[4], const uint64_t s[4],
                                                     const uint64_t rho[4], uint64_t ar_out[8], uint64_t bs_out[16], uint64_t krs_out[8],
                                                     uint64_t* commitments_out, uint64_t pok_out[8]) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!key || !witness || !r || !s || !rho || !ar_out || !bs_out || !krs_out || !commitments_out || !pok_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (!key->n_commit) return ctx->fail(NLX_E_INVAL, "the key carries no commitment: its proofs come from nlx_bn254_groth16_prove");
    if (is_device_ptr(rho)) return ctx->fail(NLX_E_INVAL, "rho is a host value");
    if (!bnf::below_mod<bnf::RP>(rho)) return ctx->fail(NLX_E_RANGE, "rho is not below the group order");
    return prove_body(ctx, key, witness, a, b, c, r, s, rho, ar_out, bs_out, krs_out, commitments_out, pok_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_bn254_groth16_commit(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, uint32_t j, const uint64_t* witness, uint64_t out[8]) NLX_TRY {
    using namespace nlx::msm;
    if (!ctx) return NLX_E_INVAL;
    if (!key || !witness || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
    if (!key->n_commit) return ctx->fail(NLX_E_INVAL, "the key carries no commitment");
    if (j >= key->n_commit) return ctx->fail(NLX_E_RANGE, "commitment %u of %u", j, key->n_commit);
    const uint32_t lo = key->seg[j], count = key->seg[j + 1] - lo;
    if (!count) {   // the empty sum
        memset(out, 0, 64);
        return NLX_OK;
    }
    (void)hipSetDevice(ctx->device);
    Staged sw(ctx, witness, (size_t)key->n_wires * 32, true, false);
    if (sw.status) return sw.status;
    SortedDigits sorted;
    struct ReleaseSorted {   // after `scratch` (declared later, destroyed first) has synchronised the stream
        nlx_ctx* ctx;
        SortedDigits* s;
        ~ReleaseSorted() { release_digits(ctx, s); }
    } release_sorted{ctx, &sorted};
    Scratch scratch(ctx);
    uint64_t* d_plain = (uint64_t*)scratch.alloc((size_t)count * 32);
    void* d_buckets = scratch.alloc(bucket_bytes(0));
    void* d_wsum = scratch.alloc(window_sum_bytes(0));
    if (!d_plain || !d_buckets || !d_wsum) return ctx->fail(NLX_E_NOMEM, "Groth16 commitment: device memory");
    g16::CommitSegments seg{};
    ctx->begin_kernel("bn254_groth16_commit", 100.0 * (double)count, (double)count);
    launch_gather(key, lo, count, sw.as<uint64_t>(), seg, d_plain, nullptr);
    int32_t rc = sort_digits(ctx, d_plain, count, 1, &sorted);
    if (!rc) bucket_reduce(ctx, sorted, (const unsigned char*)key->basis + (size_t)lo * converted_point_bytes(0), 0, d_buckets, d_wsum);
    ctx->end_kernel();
    if (rc) return rc;
    std::vector<unsigned char> words(window_sum_bytes(0));
    rc = fetch(ctx, words.data(), d_wsum, words.size());
    if (!rc) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = ctx->hip_fail(e, "kernel launch");
    }
    if (rc) return rc;
    hstore_affine<H1>(window_tail_g1(words.data()), out);
    return NLX_OK;
} NLX_CATCH(ctx)
