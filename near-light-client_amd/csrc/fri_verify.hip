// The part of a device verifier that every proof format with a FRI proof in it shares (fri_verify.hpp):
// the two kernels over the queries and the host driver of a batch call.
// The device reads the aligned staging copy of the proof only; every address and loop bound comes from the descriptor or from a
// transcript output reduced mod the LDE size, none from a byte of the proof.
#include <algorithm>
#include "fri_verify.hpp"
#include "poseidon_bn128_path.hpp"
#include "poseidon_quad.hpp"

namespace nlx {
namespace fv {

constexpr uint32_t MAX_TREES = fpl::MAX_TREES + fpl::MAX_LAYERS;
enum : uint32_t { FRI_FAIL_FOLD = 1, FRI_FAIL_FINAL = 2 };   // k_fri_queries' code: kind << 8 | layer

// one Merkle tree of the proof: an initial tree or a FRI layer
struct VTree {
    uint32_t w_row, width;      // the opened row (or coset): word offset within the query, words
    uint32_t w_path, path_len;  // siblings
    uint32_t w_cap;             // word offset of the cap within the proof, or within the cap outside it
    uint32_t shift;             // leaf index = x_index >> shift
    uint32_t group;             // leaf_group_cols (0 for a FRI layer)
    uint32_t ext_cap;           // 1: the cap is PathParams::ext_cap, not in the proof
};

struct PathParams {
    const uint64_t* stage;      // [proof][w_total]
    const uint64_t* ext_cap;    // a cap the proofs do not carry (plonky2's constants_sigmas_cap), or null
    const uint32_t* qidx;       // [proof][query]
    uint8_t* fail;              // [proof][query][tree]: 0 the path holds, 1 it does not (preset to 0xFF: not run)
    size_t w_total, w_queries, w_query_words;
    uint32_t n_items, n_queries, n_trees;
    VTree trees[MAX_TREES];
};

// hash_no_pad of n >= 1 words onto the state (overwrite-mode absorb, eight words a permutation); n is quad-uniform
__device__ __forceinline__ void quad_absorb(gl32::F (&x)[3], const uint64_t* __restrict__ v, uint32_t n, uint32_t q, const pquad::Mds& mds) {
#pragma unroll 1
    for (uint32_t c = 0; c < n; c += 8) {
        if (c + q < n) x[0] = gl32::from_u64(v[c + q]);
        if (c + 4 + q < n) x[1] = gl32::from_u64(v[c + 4 + q]);
        pquad::permute(x, q, mds);
    }
}

// blockIdx.y = tree, so width, grouping, path length and where the cap lies are block-uniform; spare quads redo the last item and
// store nothing.  Lane q of a quad holds word q of the running digest.  GROUPED: the format has grouped leaves
// (Verifier::grouped_leaves) - one without them runs the instantiation that carries neither that code nor its registers.
template <bool GROUPED>
__global__ __launch_bounds__(64) void k_fri_paths(PathParams p) {
    const VTree t = p.trees[blockIdx.y];
    const uint32_t q = threadIdx.x & 3;
    const uint32_t raw = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool live = raw < p.n_items;
    const uint32_t item = live ? raw : p.n_items - 1;
    const uint32_t proof = item / p.n_queries, query = item - proof * p.n_queries;
    const uint64_t* base = p.stage + (size_t)proof * p.w_total;
    const uint64_t* qs = base + p.w_queries + (size_t)query * p.w_query_words;
    const uint64_t* row = qs + t.w_row;
    const uint32_t idx = p.qidx[item] >> t.shift;
    const pquad::Mds mds = pquad::mds_table(q);
    gl32::F x[3] = {gl32::from_u64(0), gl32::from_u64(0), gl32::from_u64(0)};
    if (t.width <= 4) {   // hash_or_noop: the row is its own digest, zero-padded
        if (q < t.width) x[0] = gl32::from_u64(row[q]);
    } else if (!GROUPED || t.group == 0 || t.width <= t.group) {
        quad_absorb(x, row, t.width, q, mds);
    } else {
        // grouped leaves: hash_no_pad of every run of `group` columns, then hash_no_pad of the run digests - two digests a
        // permutation, and lane q's word of a run digest is exactly the word it owns of the outer state
        gl32::F y[3] = {gl32::from_u64(0), gl32::from_u64(0), gl32::from_u64(0)};
        const uint32_t K = (t.width + t.group - 1) / t.group;
#pragma unroll 1
        for (uint32_t g = 0; g < K; g++) {
            const uint32_t c0 = g * t.group, len = t.width - c0 < t.group ? t.width - c0 : t.group;
            x[0] = x[1] = x[2] = gl32::from_u64(0);
            quad_absorb(x, row + c0, len, q, mds);
            y[g & 1] = gl32::from_u64(gl::canon(gl32::to_u64(x[0])));
            if ((g & 1) || g + 1 == K) pquad::permute(y, q, mds);
        }
        x[0] = y[0];
    }
    uint64_t cur = gl::canon(gl32::to_u64(x[0]));
    const uint64_t* path = qs + t.w_path;
#pragma unroll 1
    for (uint32_t k = 0; k < t.path_len; k++) {
        const uint64_t sib = path[4 * k + q];
        const bool right = (idx >> k) & 1;   // the same for the four lanes
        x[0] = gl32::from_u64(right ? sib : cur);
        x[1] = gl32::from_u64(right ? cur : sib);
        x[2] = gl32::from_u64(0);
        pquad::permute(x, q, mds);
        cur = gl::canon(gl32::to_u64(x[0]));
    }
    const uint64_t* cap = (t.ext_cap ? p.ext_cap : base) + t.w_cap;
    const bool ok = cur == cap[(size_t)(idx >> t.path_len) * 4 + q];   // idx < 2^(path_len + cap_height)
    const unsigned long long m = __ballot(ok);
    const bool quad_ok = ((m >> (threadIdx.x & 60u)) & 0xFull) == 0xFull;
    if (live && q == 0) p.fail[(size_t)item * p.n_trees + blockIdx.y] = quad_ok ? 0 : 1;
}

// The same grid and items for trees hashed with PoseidonBN128 (Verifier::hasher): one quad per (proof, query, tree) on the
// lane-split permutation, lane q holding element q of the state as nine 29-bit limbs in Montgomery form; the work of the quad is
// pbn::quad_merkle_path (poseidon_bn128_path.hpp).  A digest is one integer below r, four words: lane 0 brings the last one out
// of Montgomery form and compares the four words with the cap's.  The siblings were checked below r by the parser
// (fpl::first_bad_word_bn128).  There is no hash_or_noop branch: validate_circuit_desc (prover.hip) refuses a BN128 circuit
// with an oracle of <= 4 columns, and a commit-phase leaf has 2 arity >= 8 words - every row here is hashed.
__global__ __launch_bounds__(64) void k_fri_paths_bn128(PathParams p) {
    const VTree t = p.trees[blockIdx.y];
    const uint32_t q = threadIdx.x & 3;
    const uint32_t raw = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool live = raw < p.n_items;
    const uint32_t item = live ? raw : p.n_items - 1;   // spare quads redo the last item and store nothing: a quad stays whole
    const uint32_t proof = item / p.n_queries, query = item - proof * p.n_queries;
    const uint64_t* base = p.stage + (size_t)proof * p.w_total;
    const uint64_t* qs = base + p.w_queries + (size_t)query * p.w_query_words;
    const uint32_t idx = p.qidx[item] >> t.shift;
    const pbn::QuadRow qrow = pbn::quad_row(q);
    const pbn::Fe s = pbn::quad_merkle_path(f29::zero(), qs + t.w_row, t.width, idx, qs + t.w_path, t.path_len, q, qrow);
    uint64_t d[4];
    pbn::to_words(s, d);
    const uint64_t* cap = (t.ext_cap ? p.ext_cap : base) + t.w_cap + (size_t)(idx >> t.path_len) * 4;   // idx < 2^(path_len + cap_height)
    const bool ok = d[0] == cap[0] && d[1] == cap[1] && d[2] == cap[2] && d[3] == cap[3];
    if (live && q == 0) p.fail[(size_t)item * p.n_trees + blockIdx.y] = ok ? 0 : 1;
}

struct FriParams {
    const uint64_t* stage;
    const uint64_t* pp;         // [proof][pp_stride]
    const uint32_t* qidx;
    uint32_t* fail;             // [proof][query]: 0, or kind << 8 | layer
    size_t w_total, w_queries, w_query_words, w_final_poly;
    uint32_t pp_stride, n_queries, log_L, arity_bits, n_layers, final_len, n_runs, batch_shift;
    FriRun runs[fpl::MAX_TREES];
    uint32_t w_layer_evals[fpl::MAX_LAYERS];
    // the blocks past n_items: one per (proof, periodic column)
    const uint64_t* per_coeffs; // device: [column][period] coefficients of the periodic columns' interpolations
    uint64_t* per;              // [proof][column]: P_a(zeta^(n / period)), an extension element
    uint32_t n_items, n_periodic, period_bits, log_n;
};

__device__ __forceinline__ gl::Ext wave_sum(gl::Ext v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint64_t a = __shfl_xor((unsigned long long)v.a, off), b = __shfl_xor((unsigned long long)v.b, off);
        v = gl::add(v, gl::Ext{a, b});
    }
    return v;   // every lane has the sum
}
__device__ __forceinline__ gl::Ext base_minus(uint64_t x, gl::Ext y) { return gl::Ext{gl::sub(x, y.a), gl::neg(y.b)}; }

// One wave per (proof, query).  The lanes stride over each run of opened columns for sum_j alpha^j row[j] (lane l starts at
// alpha^(pow0 + l) and steps by alpha^64) and add it to the batches the run enters, one wave reduction a batch gives the two
// sums; the fold chain runs on values every lane holds, with the arity terms of each interpolation on lanes 0 .. arity - 1.
// The same launch carries what a constraint kernel needs once per proof and not once per load: blocks past the queries evaluate
// one periodic column each at y = zeta^(n / period), P_a(y) = sum_m c_m y^m with the lanes striding over m as above.
__global__ __launch_bounds__(64) void k_fri_queries(FriParams p) {
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= p.n_items) {   // block-uniform
        const uint32_t w = blockIdx.x - p.n_items, proof = w / p.n_periodic, a = w - proof * p.n_periodic;
        const uint64_t* pp = p.pp + (size_t)proof * p.pp_stride;
        gl::Ext y{pp[PP_ZETA], pp[PP_ZETA + 1]};
        for (uint32_t i = p.period_bits; i < p.log_n; i++) y = gl::mul(y, y);
        const uint64_t* co = p.per_coeffs + ((size_t)a << p.period_bits);
        const gl::Ext y64 = gl::pow(y, 64);
        gl::Ext yp = gl::pow(y, lane), acc{0, 0};
        for (uint32_t m = lane; m < (1u << p.period_bits); m += 64) {
            acc = gl::add(acc, gl::mul(yp, co[m]));
            yp = gl::mul(yp, y64);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            p.per[2 * (size_t)w] = acc.a;
            p.per[2 * (size_t)w + 1] = acc.b;
        }
        return;
    }
    const uint32_t item = blockIdx.x;
    const uint32_t proof = item / p.n_queries, query = item - proof * p.n_queries;
    const uint64_t* base = p.stage + (size_t)proof * p.w_total;
    const uint64_t* qs = base + p.w_queries + (size_t)query * p.w_query_words;
    const uint64_t* pp = p.pp + (size_t)proof * p.pp_stride;
    const gl::Ext alpha{pp[PP_FRI_ALPHA], pp[PP_FRI_ALPHA + 1]};
    const gl::Ext alpha64 = gl::pow(alpha, 64);
    gl::Ext acc0{0, 0}, acc1{0, 0};   // the batch at zeta, the batch at g zeta
    for (uint32_t r = 0; r < p.n_runs; r++) {
        const FriRun run = p.runs[r];
        const uint64_t* row = qs + run.w_off;
        gl::Ext ap = gl::pow(alpha, run.pow0 + lane), part{0, 0};
        for (uint32_t c = lane; c < run.count; c += 64) {
            part = gl::add(part, gl::mul(ap, row[c]));
            ap = gl::mul(ap, alpha64);
        }
        if (run.batches & 1) acc0 = gl::add(acc0, part);
        if (run.batches & 2) acc1 = gl::add(acc1, part);
    }
    acc0 = wave_sum(acc0);
    acc1 = wave_sum(acc1);
    uint32_t x_index = p.qidx[item];
    uint64_t sx = gl::mul(gl::GEN, gl::pow(gl::root_of_unity(p.log_L), gl::bitrev32(x_index, p.log_L)));
    // fri_combine_initial: the batch at zeta, shifted by alpha^(the g zeta batch's count), then the batch at g zeta
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]}, gzeta{pp[PP_GZETA], pp[PP_GZETA + 1]};
    const gl::Ext red0{pp[PP_RED0], pp[PP_RED0 + 1]}, red1{pp[PP_RED1], pp[PP_RED1 + 1]};
    gl::Ext old = gl::mul(gl::sub(acc0, red0), gl::inv(base_minus(sx, zeta)));
    old = gl::add(gl::mul(old, gl::pow(alpha, p.batch_shift)), gl::mul(gl::sub(acc1, red1), gl::inv(base_minus(sx, gzeta))));
    const uint32_t arity = 1u << p.arity_bits;
    const uint64_t gA = gl::root_of_unity(p.arity_bits);
    uint32_t fail = 0;
    for (uint32_t k = 0; k < p.n_layers; k++) {   // every branch below is wave-uniform
        const uint64_t* ev = qs + p.w_layer_evals[k];
        const uint32_t within = x_index & (arity - 1);
        if (!gl::eq(gl::Ext{ev[2 * within], ev[2 * within + 1]}, old)) {
            fail = FRI_FAIL_FOLD << 8 | k;
            break;
        }
        // interpolation over the coset coset_start * <gA> at beta_k, barycentric: term i on lane i
        const gl::Ext beta{pp[PP_FRI_BETAS + 2 * k], pp[PP_FRI_BETAS + 2 * k + 1]};
        const uint64_t coset_start = gl::mul(sx, gl::pow(gA, arity - gl::bitrev32(within, p.arity_bits)));
        gl::Ext term{0, 0};
        if (lane < arity) {
            const uint32_t e = gl::bitrev32(lane, p.arity_bits);
            const gl::Ext yi{ev[2 * e], ev[2 * e + 1]};
            const uint64_t pi = gl::mul(coset_start, gl::pow(gA, lane));
            gl::Ext num{1, 0};
            uint64_t den = 1, pj = coset_start;
            for (uint32_t j = 0; j < arity; j++) {
                if (j != lane) {
                    num = gl::mul(num, gl::Ext{gl::sub(beta.a, pj), beta.b});
                    den = gl::mul(den, gl::sub(pi, pj));
                }
                pj = gl::mul(pj, gA);
            }
            term = gl::mul(yi, gl::mul(num, gl::inv(den)));
        }
        old = wave_sum(term);
        sx = gl::exp_pow2(sx, p.arity_bits);
        x_index >>= p.arity_bits;
    }
    if (!fail) {
        const uint64_t* fp = base + p.w_final_poly;
        gl::Ext fe{0, 0};
        for (uint32_t i = p.final_len; i-- > 0;) fe = gl::add(gl::mul(fe, sx), gl::Ext{fp[2 * i], fp[2 * i + 1]});
        if (!gl::eq(fe, old)) fail = FRI_FAIL_FINAL << 8;
    }
    if (lane == 0) p.fail[item] = fail;
}

namespace {

const char* reason_name(uint32_t r) {
    static const char* const names[] = {"accept", "malformed", "public inputs", "constraints", "proof of work", "trace path",
                                        "FRI fold", "FRI path", "final polynomial"};
    return r <= NLX_VERIFY_FINAL_POLY ? names[r] : "?";
}

// the transcript from the FRI commit caps to the query indices; returns whether the proof of work fails.  A cap enters through
// observe_hash: under BN128 five limbs a digest, which the parser has found below r; the sponge, the proof of work and the
// reduction of the query indices are Goldilocks under both configs
bool transcript_tail(Challenger& ch, const fpl::Layout& l, uint32_t hasher, uint32_t pow_bits, const uint64_t* w, uint64_t* pp, uint32_t* qidx) {
    for (uint32_t k = 0; k < l.n_layers; k++) {
        (void)observe_hash(hasher, ch, w + l.w_fri_caps + k * l.cap_words, l.cap_words / 4);
        ch.ext_challenge(pp + PP_FRI_BETAS + 2 * k);
    }
    ch.observe(w + l.w_final_poly, 2 * (size_t)l.final_len);
    ch.observe(w[l.w_pow_witness]);
    const uint64_t pow_response = ch.challenge();
    for (uint32_t q = 0; q < l.n_queries; q++) qidx[q] = (uint32_t)(ch.challenge() & (((uint64_t)1 << l.log_L) - 1));
    return pow_bits && (pow_response >> (64 - pow_bits)) != 0;
}

// What one query fails first, in the order of a sequential verifier: the initial trees' paths, then per layer the fold before
// the layer's path, then the final polynomial.  pf: k_fri_paths' byte per tree, ff: k_fri_queries' code.  0: nothing.
uint32_t query_reason(const uint8_t* pf, uint32_t ff, uint32_t n_initial, uint32_t n_layers, uint32_t* tree, uint32_t* layer) {
    for (uint32_t o = 0; o < n_initial; o++)
        if (pf[o]) { *tree = o; return NLX_VERIFY_TRACE_PATH; }
    for (uint32_t k = 0; k < n_layers; k++) {
        *layer = k;
        if ((ff >> 8) == FRI_FAIL_FOLD && (ff & 0xFF) == k) return NLX_VERIFY_FRI_FOLD;
        if (pf[n_initial + k]) return NLX_VERIFY_FRI_PATH;
    }
    *layer = 0;
    return (ff >> 8) == FRI_FAIL_FINAL ? NLX_VERIFY_FINAL_POLY : 0;
}

// from the staging buffers to the verdicts of the proofs in `live`
int32_t verify_live(Verifier& v, VerifyCall& vc, const std::vector<size_t>& live, const std::vector<uint8_t>& pow_bad,
                    nlx_stark_verdict* verdicts) {
    nlx_ctx* ctx = v.ctx;
    const fpl::Layout& l = *v.lay;
    hipStream_t st = ctx->stream;
    const uint32_t nQ = l.n_queries, NT = l.n_trees, R = l.n_layers, n_trees = NT + R;
    const size_t np = live.size(), n_items = np * nQ, capw = l.cap_words, part_words = np * v.part_words;
    (void)hipSetDevice(ctx->device);
    if (v.prepare) NLX_RC(v.prepare());
    if (n_items + np * v.n_periodic > 0x7FFFFFFFu) return ctx->fail(NLX_E_RANGE, "too many proofs in one batch");
    Scratch& scratch = vc.scratch;
    uint64_t* d_stage = scratch.alloc_as<uint64_t>(np * l.w_total * 8);
    uint64_t* d_pp = scratch.alloc_as<uint64_t>(np * v.pp_stride * 8);
    uint32_t* d_qidx = scratch.alloc_as<uint32_t>(n_items * 4);
    uint8_t* d_path_fail = scratch.alloc_as<uint8_t>(n_items * n_trees);
    uint32_t* d_fri_fail = scratch.alloc_as<uint32_t>(n_items * 4);
    uint64_t* d_part = scratch.alloc_as<uint64_t>(part_words * 8);
    uint64_t* d_per = scratch.alloc_as<uint64_t>((np * v.n_periodic + 1) * 16);
    if (!d_stage || !d_pp || !d_qidx || !d_path_fail || !d_fri_fail || !d_part || !d_per) return ctx->fail(NLX_E_NOMEM, "out of device memory");
    NLX_HIP(ctx, hipMemcpyAsync(d_stage, vc.stage.data(), np * l.w_total * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_pp, vc.pp.data(), np * v.pp_stride * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_qidx, vc.qidx.data(), n_items * 4, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemsetAsync(d_path_fail, 0xFF, n_items * n_trees, st));   // as the two below: what no kernel writes
    NLX_HIP(ctx, hipMemsetAsync(d_fri_fail, 0xFF, n_items * 4, st));
    NLX_HIP(ctx, hipMemsetAsync(d_part, 0xFF, part_words * 8, st));   // a part that was not computed can never pass for one that was
    {
        PathParams pa{};
        pa.stage = d_stage; pa.ext_cap = v.ext_cap; pa.qidx = d_qidx; pa.fail = d_path_fail;
        pa.w_total = l.w_total; pa.w_queries = l.w_queries; pa.w_query_words = l.w_query_words;
        pa.n_items = (uint32_t)n_items; pa.n_queries = nQ; pa.n_trees = n_trees;
        const uint32_t ext = v.ext_cap ? 1 : 0;   // the proof's caps belong to the trees from this one on
        for (uint32_t o = 0; o < NT; o++)
            pa.trees[o] = VTree{(uint32_t)l.w_row[o], l.tree_cols[o], (uint32_t)l.w_path[o], l.tree_plen,
                                o < ext ? 0 : (uint32_t)(v.w_caps + (o - ext) * capw), 0, v.grouped_leaves ? v.leaf_group : 0, o < ext ? 1u : 0u};
        for (uint32_t k = 0; k < R; k++)
            pa.trees[NT + k] = VTree{(uint32_t)l.w_layer_evals[k], 2 * l.arity, (uint32_t)l.w_layer_path[k], l.layer_plen[k],
                                     (uint32_t)(l.w_fri_caps + k * capw), (k + 1) * v.arity_bits, 0, 0};
        const bool bn128 = v.hasher == NLX_HASHER_POSEIDON_BN128;
        const uint32_t chunk = bn128 ? pbn::CHUNK : 8;   // words a permutation absorbs
        size_t perms = 0;
        for (uint32_t t = 0; t < n_trees; t++) perms += (pa.trees[t].width + chunk - 1) / chunk + pa.trees[t].path_len;
        ctx->begin_kernel(v.name_paths, 8.0 * np * l.w_total, (double)perms * n_items);
        const dim3 grid((unsigned)((n_items + 15) / 16), n_trees);
        if (bn128) hipLaunchKernelGGL(k_fri_paths_bn128, grid, dim3(64), 0, st, pa);
        else hipLaunchKernelGGL(v.grouped_leaves ? k_fri_paths<true> : k_fri_paths<false>, grid, dim3(64), 0, st, pa);
        ctx->end_kernel();
    }
    {
        FriParams fp{};
        fp.stage = d_stage; fp.pp = d_pp; fp.qidx = d_qidx; fp.fail = d_fri_fail;
        fp.w_total = l.w_total; fp.w_queries = l.w_queries; fp.w_query_words = l.w_query_words; fp.w_final_poly = l.w_final_poly;
        fp.pp_stride = v.pp_stride; fp.n_queries = nQ; fp.log_L = l.log_L; fp.arity_bits = v.arity_bits; fp.n_layers = R;
        fp.final_len = l.final_len; fp.n_runs = v.n_runs; fp.batch_shift = v.batch_shift;
        std::copy(v.runs, v.runs + v.n_runs, fp.runs);
        for (uint32_t k = 0; k < R; k++) fp.w_layer_evals[k] = (uint32_t)l.w_layer_evals[k];
        fp.per_coeffs = v.per_coeffs; fp.per = d_per;
        fp.n_items = (uint32_t)n_items; fp.n_periodic = v.n_periodic; fp.period_bits = v.period_bits; fp.log_n = v.log_n;
        ctx->begin_kernel(v.name_fri, 8.0 * n_items * l.w_query_words);
        hipLaunchKernelGGL(k_fri_queries, dim3((unsigned)(n_items + np * v.n_periodic)), dim3(64), 0, st, fp);
        ctx->end_kernel();
    }
    NLX_RC(v.constraints(Device{d_stage, d_pp, d_per, d_part, np}));
    std::vector<uint8_t> path_fail(n_items * n_trees);
    std::vector<uint32_t> fri_fail(n_items);
    std::vector<uint64_t> part(part_words);
    NLX_RC(fetch(ctx, path_fail.data(), d_path_fail, path_fail.size()));
    NLX_RC(fetch(ctx, fri_fail.data(), d_fri_fail, fri_fail.size() * 4));
    NLX_RC(fetch(ctx, part.data(), d_part, part_words * 8));
    for (uint8_t f : path_fail)
        if (f > 1) return ctx->fail(NLX_E_HIP, "the path kernel left a tree unwritten");
    for (uint64_t pw : part)
        if (pw >= gl::P) return ctx->fail(NLX_E_HIP, "%s", v.part_unwritten);

    // ---- the verdicts, in the order of a sequential verifier ----
    auto reject = [&](size_t i, uint32_t reason) -> nlx_stark_verdict& {
        verdicts[i].accepted = 0;
        verdicts[i].reason = reason;
        return verdicts[i];
    };
    for (size_t at = 0; at < np; at++) {
        const size_t i = live[at];
        const uint32_t j = v.judge(vc.stage.data() + at * l.w_total, vc.pp.data() + at * v.pp_stride, part.data() + at * v.part_words);
        if (j != NO_CHALLENGE) {
            reject(i, NLX_VERIFY_CONSTRAINTS).challenge = j;
            continue;
        }
        if (pow_bad[at]) {
            reject(i, NLX_VERIFY_POW);
            continue;
        }
        bool done = false;
        for (uint32_t q = 0; q < nQ && !done; q++) {
            const size_t item = at * nQ + q;
            const uint32_t ff = fri_fail[item];
            if (ff == 0xFFFFFFFFu) return ctx->fail(NLX_E_HIP, "the FRI kernel left a query unwritten");
            uint32_t tree = 0, layer = 0;
            const uint32_t reason = query_reason(path_fail.data() + item * n_trees, ff, NT, R, &tree, &layer);
            if (reason) {
                nlx_stark_verdict& vd = reject(i, reason);
                vd.query = q; vd.tree = tree; vd.layer = layer; vd.x_index = vc.qidx[item];
                done = true;
            }
        }
        if (!done) {
            verdicts[i].accepted = 1;
            verdicts[i].reason = NLX_VERIFY_ACCEPT;
        }
    }
    return NLX_OK;
}

}  // namespace

int32_t check_batch_args(nlx_ctx* ctx, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs, const uint64_t* public_inputs,
                         uint32_t n_pis, const nlx_stark_verdict* verdicts) {
    if (n_proofs && (!proofs || !lens || !verdicts)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ctx->fail(NLX_E_INVAL, "proof %llu is NULL", (unsigned long long)i);
    if (public_inputs)
        for (size_t i = 0; i < n_proofs * n_pis; i++)
            if (public_inputs[i] >= gl::P)
                return ctx->fail(NLX_E_RANGE, "public input %llu of proof %llu is not canonical", (unsigned long long)(i % n_pis),
                                 (unsigned long long)(i / n_pis));
    return NLX_OK;
}

namespace {

int32_t verify_staged(Verifier& v, VerifyCall& vc, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                      const uint64_t* public_inputs, nlx_stark_verdict* verdicts) {
    nlx_ctx* ctx = v.ctx;
    const fpl::Layout& l = *v.lay;
    const uint32_t nQ = l.n_queries, n_pis = l.n_pis;
    // ---- host: structure, public inputs, transcript, proof of work, query indices ----
    std::vector<size_t> live;            // proofs that reach the device, by index
    std::vector<uint8_t> pow_bad;        // per live proof
    vc.stage.reserve(l.w_total);
    for (size_t i = 0; i < n_proofs; i++) {
        const size_t at = live.size();
        vc.stage.resize((at + 1) * l.w_total);
        uint64_t* w = vc.stage.data() + at * l.w_total;
        fpl::Finding f;
        if (fpl::parse(l, proofs[i], lens[i], w, &f) != fpl::SOUND) {
            nlx_stark_verdict& vd = verdicts[i];
            vd.accepted = 0;
            vd.reason = NLX_VERIFY_MALFORMED;
            if (f.what == fpl::BAD_PATH_LENGTH) {
                vd.query = f.query;
                if (f.tree < l.n_trees) vd.tree = f.tree;
                else vd.layer = f.layer;
            }
            continue;
        }
        if (public_inputs && memcmp(public_inputs + i * n_pis, w + l.w_public_inputs, 8 * (size_t)n_pis) != 0) {
            verdicts[i].accepted = 0;
            verdicts[i].reason = NLX_VERIFY_PUBLIC_INPUTS;
            continue;
        }
        vc.pp.resize((at + 1) * v.pp_stride, 0);
        vc.qidx.resize((at + 1) * nQ);
        uint64_t* pp = vc.pp.data() + at * v.pp_stride;
        Challenger ch;
        v.head(w, pp, ch);
        pow_bad.push_back(transcript_tail(ch, l, v.hasher, v.pow_bits, w, pp, vc.qidx.data() + at * nQ));
        live.push_back(i);
    }
    if (!live.empty()) NLX_RC(verify_live(v, vc, live, pow_bad, verdicts));
    for (size_t i = 0; i < n_proofs; i++)
        if (!verdicts[i].accepted) {
            const nlx_stark_verdict& vd = verdicts[i];
            // NLX_OK: the check ran.  The line is for nlx_last_error.
            ctx->fail(NLX_OK, "proof %llu does not verify: %s (reason %u), challenge %u, query %u (x_index %llu), tree %u, layer %u",
                      (unsigned long long)i, reason_name(vd.reason), vd.reason, vd.challenge, vd.query, (unsigned long long)vd.x_index, vd.tree, vd.layer);
            return NLX_OK;
        }
    ctx->err.clear();   // every proof verifies: no line of an earlier rejection stays behind
    return NLX_OK;
}

}  // namespace

int32_t verify_batch(Verifier& v, VerifyCall& vc, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                     const uint64_t* public_inputs, nlx_stark_verdict* verdicts) {
    const int32_t rc = vc.scratch.finish(verify_staged(v, vc, proofs, lens, n_proofs, public_inputs, verdicts));
    if (rc) memset(verdicts, 0, n_proofs * sizeof *verdicts);   // an error is no verdict
    return rc;
}

}  // namespace fv
}  // namespace nlx
