// plonky2 verifier (C ABI: nlx_verifier_*, nlx_verify, nlx_verify_batch): does a ProofWithPublicInputs verify, and if not, which
// check breaks.
//
// plonky2::plonk::verifier::verify + fri::verifier::verify_fri_proof for the proofs of prover.hip, one proof or a batch of proofs
// of one circuit.  On the host: the structure of the proof against its layout (plonk_proof_layout.hpp), the public-inputs hash,
// the transcript, the proof of work, the query indices, the reduced openings, get_lut_poly, L_0(zeta) - a sponge is a chain, and
// a proof has one.  On the device, in three launches whatever the number of proofs:
//   k_plonk_paths        one quad of lanes per (proof, query, tree): leaf digest of the opened row, the sibling path, the cap
//   k_plonk_fri          one wave per (proof, query): fri_combine_initial over the four rows, the fold chain, the final polynomial
//   k_plonk_constraints  one lane per proof, one block row per gate (then per challenge: the permutation argument, the lookup
//                        argument): the constraints at zeta over F_p[X]/(X^2 - 7) (gate_eval_ext.hpp)
// The device reads the aligned staging copy of the proof only (and, for the constraints, its openings transposed to [word][proof]);
// every address and loop bound comes from the descriptor or from a transcript output reduced mod the LDE size, none from a byte
// of the proof.
#include <algorithm>
#include <memory>
#include <vector>
#include "gate_eval_ext.hpp"
#include "gl.hpp"
#include "plonk_proof_layout.hpp"
#include "poseidon_quad.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace nlx;

namespace nlx {
namespace pv {

constexpr uint32_t MAX_TREES = ppl::N_TREES + ppl::MAX_LAYERS;
// per proof, what the transcript gave (64-bit words)
enum : uint32_t { PP_ZETA = 0, PP_GZETA = 2, PP_FRI_ALPHA = 4, PP_RED0 = 6, PP_RED1 = 8, PP_ALPHAS = 10, PP_BETAS = 12, PP_GAMMAS = 14,
                  PP_PIH = 16, PP_L0 = 20, PP_DELTAS = 22, PP_LUT = 30, PP_FRI_BETAS = 62, PP_STRIDE = PP_FRI_BETAS + 2 * ppl::MAX_LAYERS };
enum : uint32_t { FRI_FAIL_FOLD = 1, FRI_FAIL_FINAL = 2 };   // k_plonk_fri's code: kind << 8 | layer
constexpr uint64_t UNUSED_SELECTOR = 0xFFFFFFFFULL;          // gates::selectors::UNUSED_SELECTOR

// one Merkle tree of the proof: an initial tree or a FRI layer
struct VTree {
    uint32_t w_row, width;      // the opened row (or coset): word offset within the query, words
    uint32_t w_path, path_len;  // siblings
    uint32_t w_cap;             // word offset of the cap within the proof (own_cap) or within the circuit's cap
    uint32_t shift;             // leaf index = x_index >> shift
    uint32_t own_cap;           // 1: the cap is in the proof; 0: it is the circuit's constants_sigmas_cap
    uint32_t pad_;
};

struct PathParams {
    const uint64_t* stage;      // [proof][w_total]
    const uint64_t* cs_cap;     // the circuit's constants_sigmas_cap
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

// blockIdx.y = tree, so width and path length are block-uniform; spare quads redo the last item and store nothing.  Lane q of a
// quad holds word q of the running digest.
__global__ __launch_bounds__(64) void k_plonk_paths(PathParams p) {
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
    } else {
        quad_absorb(x, row, t.width, q, mds);
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
    const uint64_t* cap = t.own_cap ? base + t.w_cap : p.cs_cap;
    const bool ok = cur == cap[(size_t)(idx >> t.path_len) * 4 + q];   // idx < 2^(path_len + cap_height)
    const unsigned long long m = __ballot(ok);
    const bool quad_ok = ((m >> (threadIdx.x & 60u)) & 0xFull) == 0xFull;
    if (live && q == 0) p.fail[(size_t)item * p.n_trees + blockIdx.y] = quad_ok ? 0 : 1;
}

// a run of opened columns that enters one of the two FRI batches
struct FriSeg {
    uint32_t w_off;    // word offset of its first column within the query
    uint32_t count;
    uint32_t pow0;     // its first column's power of alpha
    uint32_t batch;    // 0: opened at zeta, 1: at g zeta
};

struct FriParams {
    const uint64_t* stage;
    const uint64_t* pp;         // [proof][PP_STRIDE]
    const uint32_t* qidx;
    uint32_t* fail;             // [proof][query]: 0, or kind << 8 | layer
    size_t w_total, w_queries, w_query_words, w_final_poly;
    uint32_t n_queries, log_L, arity_bits, n_layers, final_len, n_segs, n_batch1;
    FriSeg seg[8];
    uint32_t w_layer_evals[ppl::MAX_LAYERS];
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
// alpha^(pow0 + l) and steps by alpha^64), one wave reduction gives the two batches' sums; the fold chain runs on values every
// lane holds, with the arity terms of each interpolation on lanes 0 .. arity - 1.
__global__ __launch_bounds__(64) void k_plonk_fri(FriParams p) {
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    const uint32_t proof = item / p.n_queries, query = item - proof * p.n_queries;
    const uint64_t* base = p.stage + (size_t)proof * p.w_total;
    const uint64_t* qs = base + p.w_queries + (size_t)query * p.w_query_words;
    const uint64_t* pp = p.pp + (size_t)proof * PP_STRIDE;
    const gl::Ext alpha{pp[PP_FRI_ALPHA], pp[PP_FRI_ALPHA + 1]};
    const gl::Ext alpha64 = gl::pow(alpha, 64);
    gl::Ext acc[2] = {{0, 0}, {0, 0}};
    for (uint32_t s = 0; s < p.n_segs; s++) {
        const FriSeg sg = p.seg[s];
        const uint64_t* row = qs + sg.w_off;
        gl::Ext ap = gl::pow(alpha, sg.pow0 + lane), part{0, 0};
        for (uint32_t c = lane; c < sg.count; c += 64) {
            part = gl::add(part, gl::mul(ap, row[c]));
            ap = gl::mul(ap, alpha64);
        }
        if (sg.batch) acc[1] = gl::add(acc[1], part);
        else acc[0] = gl::add(acc[0], part);
    }
    acc[0] = wave_sum(acc[0]);
    acc[1] = wave_sum(acc[1]);
    uint32_t x_index = p.qidx[item];
    uint64_t sx = gl::mul(gl::GEN, gl::pow(gl::root_of_unity(p.log_L), gl::bitrev32(x_index, p.log_L)));
    // fri_combine_initial: the batch at zeta, shifted by alpha^(the g zeta batch's count), then the batch at g zeta
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]}, gzeta{pp[PP_GZETA], pp[PP_GZETA + 1]};
    const gl::Ext red0{pp[PP_RED0], pp[PP_RED0 + 1]}, red1{pp[PP_RED1], pp[PP_RED1 + 1]};
    gl::Ext old = gl::mul(gl::sub(acc[0], red0), gl::inv(base_minus(sx, zeta)));
    old = gl::add(gl::mul(old, gl::pow(alpha, p.n_batch1)), gl::mul(gl::sub(acc[1], red1), gl::inv(base_minus(sx, gzeta))));
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

struct ConsParams {
    const uint64_t* open;       // [word of the opening set][proof]: extension element e = words 2 e and 2 e + 1
    const uint64_t* pp;         // [proof][PP_STRIDE]
    const GateDev* gates;
    const uint64_t* k_is;
    uint64_t* part;             // [proof][item][challenge] extension elements
    uint32_t n_proofs, n_items, n_gates, nc, npp, routed, chunk, num_wires, num_constants, num_selectors, n_lk_sel, n_lk_terms,
        n_lk_per_round;         // 1 + S
    uint32_t e_consts, e_sigmas, e_wires, e_zs, e_zs_next, e_lk, e_lk_next, e_pp;   // element offsets of the opening classes
    LookupShape lk;
};

// What one (proof, item) leaves per challenge c.  Item g < n_gates: filter_g(selector opening) * sum_j alpha_c^j g_j(zeta) - the
// host scales the gates' total by alpha_c^(index of the first gate term).  Item n_gates + ci: the permutation argument's terms of
// challenge round ci, L_0 (Z - 1) and the num_partial_products + 1 chunk identities, each times its own power of alpha_c.  Item
// n_gates + nc + ci (circuits with tables): the lookup terms of round ci, likewise.  Host and device: the kernel below is this
// function on a lane per proof.
GL_HD void constraints_item(const ConsParams& p, uint32_t proof, uint32_t item) {
    using gl::Ext;
    const uint64_t* pp = p.pp + (size_t)proof * PP_STRIDE;
    auto opening = [&](uint32_t e) { return Ext{p.open[(size_t)(2 * e) * p.n_proofs + proof], p.open[(size_t)(2 * e + 1) * p.n_proofs + proof]}; };
    auto wire = [&](uint32_t i) { return i < p.num_wires ? opening(p.e_wires + i) : Ext{0, 0}; };
    const uint32_t nc = p.nc;
    const uint64_t alphas[2] = {pp[PP_ALPHAS], pp[PP_ALPHAS + 1]};
    Ext acc[2] = {{0, 0}, {0, 0}};
    uint64_t ap[2] = {1, 1};
    auto emit = [&](Ext c) {
        for (uint32_t j = 0; j < nc; j++) {
            acc[j] = gl::add(acc[j], gl::mul(c, ap[j]));
            ap[j] = gl::mul(ap[j], alphas[j]);
        }
    };
    if (item < p.n_gates) {
        const GateDev g = p.gates[item];
        const uint32_t c0 = p.num_selectors + p.n_lk_sel;
        auto cst = [&](uint32_t i) { return i < p.num_constants ? opening(p.e_consts + c0 + i) : Ext{0, 0}; };
        gext::eval_gate_ext(g, wire, cst, pp + PP_PIH, emit);
        // the filter: prod over the gate's selector group, but for the gate itself, of (index - s), times (UNUSED - s) when the
        // circuit has more than one selector
        const Ext s = opening(p.e_consts + g.selector_index);
        Ext f{1, 0};
        for (uint32_t i = g.group_start; i < g.group_end; i++)
            if (i != g.index) f = gl::mul(f, Ext{gl::sub((uint64_t)i, s.a), gl::neg(s.b)});
        if (p.num_selectors > 1) f = gl::mul(f, Ext{gl::sub(UNUSED_SELECTOR, s.a), gl::neg(s.b)});
        for (uint32_t j = 0; j < nc; j++) acc[j] = gl::mul(acc[j], f);
    } else if (item < p.n_gates + nc) {
        const uint32_t ci = item - p.n_gates;
        const uint64_t beta = pp[PP_BETAS + ci], gamma = pp[PP_GAMMAS + ci];
        const Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]}, l0{pp[PP_L0], pp[PP_L0 + 1]};
        const Ext z = opening(p.e_zs + ci);
        for (uint32_t j = 0; j < nc; j++) ap[j] = gl::pow(alphas[j], ci);
        emit(gl::mul(l0, gext::sub_base(z, 1)));
        for (uint32_t j = 0; j < nc; j++) ap[j] = gl::pow(alphas[j], nc + ci * (p.npp + 1));
        Ext prev = z;
        for (uint32_t q = 0; q <= p.npp; q++) {
            Ext num{1, 0}, den{1, 0};
            for (uint32_t w = q * p.chunk; w < (q + 1) * p.chunk && w < p.routed; w++) {
                const Ext x = opening(p.e_wires + w);
                const Ext s_id = gl::mul(zeta, p.k_is[w]);
                num = gl::mul(num, gext::add_base(gl::add(x, gl::mul(s_id, beta)), gamma));
                den = gl::mul(den, gext::add_base(gl::add(x, gl::mul(opening(p.e_sigmas + w), beta)), gamma));
            }
            const Ext next = q < p.npp ? opening(p.e_pp + ci * p.npp + q) : opening(p.e_zs_next + ci);
            emit(gl::sub(gl::mul(prev, num), gl::mul(next, den)));
            prev = next;
        }
    } else {
        const uint32_t ci = item - p.n_gates - nc;
        const uint32_t t_lk = nc + nc * (p.npp + 1);
        for (uint32_t j = 0; j < nc; j++) ap[j] = gl::pow(alphas[j], t_lk + ci * p.n_lk_terms);
        auto sel = [&](uint32_t i) { return opening(p.e_consts + p.num_selectors + i); };
        auto lz = [&](uint32_t i) { return opening(p.e_lk + ci * p.n_lk_per_round + i); };
        auto lz_next = [&](uint32_t i) { return opening(p.e_lk_next + ci * p.n_lk_per_round + i); };
        gext::eval_lookup_ext(p.lk, wire, sel, lz, lz_next, pp + PP_DELTAS + 4 * ci, pp + PP_LUT + ci * p.lk.num_luts, emit);
    }
    for (uint32_t j = 0; j < nc; j++) {
        uint64_t* out = p.part + (((size_t)proof * p.n_items + item) * nc + j) * 2;
        out[0] = acc[j].a;
        out[1] = acc[j].b;
    }
}

// Lane = proof, blockIdx.y = item: the gate kind is block-uniform, nothing diverges on it, and a wave's loads of one opening
// word of its 64 proofs are one line.
__global__ __launch_bounds__(64) void k_plonk_constraints(ConsParams p) {
    const uint32_t proof = blockIdx.x * blockDim.x + threadIdx.x;
    if (proof >= p.n_proofs) return;   // nothing below talks to another lane
    constraints_item(p, proof, blockIdx.y);
}

}  // namespace pv
}  // namespace nlx

struct nlx_verifier {
    nlx_ctx* ctx = nullptr;
    // common data: the descriptor, its arrays copied, and the derived counts
    nlx_circuit_desc d{};
    std::vector<nlx_gate_desc> gates;
    std::vector<uint64_t> k_is;
    std::vector<uint32_t> lut_sizes, lut_offsets, lookup_rows, lut_num_lookups;
    std::vector<uint16_t> lut_pairs;
    uint32_t n_consts_all = 0, n_cs = 0, n_zs = 0, n_zpp = 0, n_q = 0, n_lk_sel = 0, n_lk_polys = 0, n_lk_terms = 0, n_fri_rounds = 0,
             max_gate_constraints = 0;
    LookupShape lk{};
    // verifier-only data
    std::vector<uint64_t> cs_cap;
    uint64_t digest[4] = {0, 0, 0, 0};
    ppl::Layout lay{};
    // device: gates | k_is | cap, one block
    void* d_block = nullptr;
    GateDev* d_gates = nullptr;
    uint64_t *d_k_is = nullptr, *d_cs_cap = nullptr;
};

namespace {

using namespace nlx::pv;

// the host half of a verifier: the copies, the derived counts, the layout; gd: the gates as the kernels read them
int32_t verifier_fill(nlx_ctx* ctx, nlx_verifier* v, const nlx_circuit_desc& d, const uint64_t* cap, const uint64_t digest[4],
                      std::vector<GateDev>& gd) {
    v->ctx = ctx;
    v->d = d;
    v->gates.assign(d.gates, d.gates + d.num_gates);
    v->k_is.assign(d.k_is, d.k_is + d.num_routed_wires);
    v->d.gates = v->gates.data();
    v->d.k_is = v->k_is.data();
    if (d.num_luts) {
        const uint32_t T = d.num_luts;
        v->lk.num_luts = T;
        v->lk.n_lu_slots = d.num_routed_wires / 2;
        v->lk.n_lut_slots = d.num_routed_wires / 3;
        v->lk.lu_degree = d.quotient_degree_factor - 1;
        v->lk.n_sldc = (v->lk.n_lu_slots + v->lk.lu_degree - 1) / v->lk.lu_degree;
        v->lk.lut_degree = (v->lk.n_lut_slots + v->lk.n_sldc - 1) / v->lk.n_sldc;
        v->n_lk_sel = 4 + T;
        v->n_lk_polys = d.num_challenges * (1 + v->lk.n_sldc);
        v->n_lk_terms = 4 + T + 2 * v->lk.n_sldc;
        v->lut_sizes.assign(d.lut_sizes, d.lut_sizes + T);
        v->lut_num_lookups.assign(d.lut_num_lookups, d.lut_num_lookups + T);
        v->lookup_rows.assign(d.lookup_rows, d.lookup_rows + 3 * T);
        v->lut_offsets.assign(T + 1, 0);
        for (uint32_t t = 0; t < T; t++) v->lut_offsets[t + 1] = v->lut_offsets[t] + v->lut_sizes[t];
        v->lut_pairs.assign(d.lut_pairs, d.lut_pairs + 2 * (size_t)v->lut_offsets[T]);
        v->d.lut_sizes = v->lut_sizes.data(); v->d.lut_num_lookups = v->lut_num_lookups.data();
        v->d.lookup_rows = v->lookup_rows.data(); v->d.lut_pairs = v->lut_pairs.data();
    }
    v->n_consts_all = d.num_selectors + v->n_lk_sel + d.num_constants;
    v->n_cs = v->n_consts_all + d.num_routed_wires;
    v->n_zpp = d.num_challenges * (1 + d.num_partial_products);
    v->n_zs = v->n_zpp + v->n_lk_polys;
    v->n_q = d.num_challenges * d.quotient_degree_factor;
    v->n_fri_rounds = fri_num_rounds(d.degree_bits, d.rate_bits, d.cap_height, d.fri_arity_bits, d.fri_final_poly_bits);
    gd.resize(d.num_gates);
    for (uint32_t g = 0; g < d.num_gates; g++) {
        const nlx_gate_desc& s = d.gates[g];
        gd[g] = GateDev{s.kind, s.selector_index, s.group_start, s.group_end, s.index, s.param0, s.param1};
        v->max_gate_constraints = std::max(v->max_gate_constraints, gext::gate_num_constraints(gd[g]));
    }
    const size_t capw = (size_t)4 << d.cap_height;
    v->cs_cap.assign(cap, cap + capw);
    for (uint64_t w : v->cs_cap)
        if (w >= gl::P) return ctx->fail(NLX_E_RANGE, "a word of constants_sigmas_cap is not canonical");
    memcpy(v->digest, digest, 32);
    memcpy(v->d.circuit_digest, digest, 32);
    ppl::Shape sh{};
    sh.degree_bits = d.degree_bits; sh.rate_bits = d.rate_bits; sh.cap_height = d.cap_height; sh.arity_bits = d.fri_arity_bits;
    sh.final_poly_bits = d.fri_final_poly_bits; sh.n_queries = d.fri_num_queries; sh.n_pis = d.num_public_inputs;
    sh.n_constants = v->n_consts_all; sh.n_sigmas = d.num_routed_wires; sh.n_wires = d.num_wires; sh.n_challenges = d.num_challenges;
    sh.n_partial = d.num_challenges * d.num_partial_products; sh.n_lookup_polys = v->n_lk_polys; sh.n_quotient = v->n_q;
    if (!ppl::make_layout(sh, &v->lay) || v->lay.n_layers != v->n_fri_rounds)
        return ctx->fail(NLX_E_UNSUPPORTED, "the circuit's proofs have a shape the verifier does not take");
    if (d.num_gates + 2 * d.num_challenges > 65535) return ctx->fail(NLX_E_RANGE, "too many gate kinds");
    if (d.fri_num_queries == 0) return ctx->fail(NLX_E_RANGE, "a proof without FRI queries is not verified");
    return NLX_OK;
}

int32_t verifier_build(nlx_ctx* ctx, const nlx_circuit_desc& d, const uint64_t* cap, const uint64_t digest[4], nlx_verifier** out) {
    std::unique_ptr<nlx_verifier> v(new nlx_verifier());
    std::vector<GateDev> gd;
    NLX_RC(verifier_fill(ctx, v.get(), d, cap, digest, gd));
    const size_t capw = (size_t)4 << d.cap_height;
    // device copies of what the kernels index by descriptor values
    (void)hipSetDevice(ctx->device);
    const size_t b_gates = (gd.size() * sizeof(GateDev) + 15) & ~(size_t)15, b_k = v->k_is.size() * 8, b_cap = capw * 8;
    v->d_block = ctx->alloc(b_gates + b_k + b_cap);
    if (!v->d_block) return ctx->fail(NLX_E_NOMEM, "out of device memory");
    std::vector<uint8_t> img(b_gates + b_k + b_cap, 0);
    if (!gd.empty()) memcpy(img.data(), gd.data(), gd.size() * sizeof(GateDev));
    memcpy(img.data() + b_gates, v->k_is.data(), b_k);
    memcpy(img.data() + b_gates + b_k, v->cs_cap.data(), b_cap);
    hipError_t e = hipMemcpyAsync(v->d_block, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->release(v->d_block);
        return ctx->hip_fail(e, "hipMemcpyAsync(verifier data)");
    }
    v->d_gates = (GateDev*)v->d_block;
    v->d_k_is = (uint64_t*)((uint8_t*)v->d_block + b_gates);
    v->d_cs_cap = (uint64_t*)((uint8_t*)v->d_block + b_gates + b_k);
    *out = v.release();
    return NLX_OK;
}

const char* reason_name(uint32_t r) {
    static const char* const names[] = {"accept", "malformed", "public inputs", "constraints", "proof of work", "trace path",
                                        "FRI fold", "FRI path", "final polynomial"};
    return r <= NLX_VERIFY_FINAL_POLY ? names[r] : "?";
}

// What one call holds until its stream work has drained.  Members go in reverse order: the scratch first - which synchronises -,
// then the host sources of the asynchronous copies.
struct VerifyCall {
    std::vector<uint64_t> stage, pp, open;
    std::vector<uint32_t> qidx;
    Scratch scratch;
    explicit VerifyCall(nlx_ctx* ctx) : scratch(ctx) {}
};

// everything of one proof that is one chain: the transcript, the proof of work, the query indices, the reduced openings,
// get_lut_poly, L_0(zeta).  w: the staging copy; pp: PP_STRIDE words, zeroed; qidx: fri_num_queries entries.  Returns whether the
// proof of work fails.
bool host_transcript(const nlx_verifier* v, const uint64_t* w, uint64_t* pp, uint32_t* qidx) {
    const nlx_circuit_desc& d = v->d;
    const ppl::Layout& l = v->lay;
    const uint32_t nc = d.num_challenges, nlk = v->n_lk_polys, R = l.n_layers;
    const size_t capw = l.cap_words;
    const uint64_t* pis = w + l.w_public_inputs;
    hash_no_pad_host(pis, d.num_public_inputs, pp + PP_PIH);
    Challenger ch;
    ch.observe(v->digest, 4);
    ch.observe(pp + PP_PIH, 4);
    ch.observe(w + l.w_caps, capw);                                   // wires cap
    for (uint32_t i = 0; i < nc; i++) pp[PP_BETAS + i] = ch.challenge();
    for (uint32_t i = 0; i < nc; i++) pp[PP_GAMMAS + i] = ch.challenge();
    if (d.num_luts) {
        // the lookup challenges: the betas and gammas again, then 2 nc more; round ci takes four consecutive entries
        uint64_t* deltas = pp + PP_DELTAS;
        for (uint32_t i = 0; i < nc; i++) { deltas[i] = pp[PP_BETAS + i]; deltas[nc + i] = pp[PP_GAMMAS + i]; }
        for (uint32_t i = 0; i < 2 * nc; i++) deltas[2 * nc + i] = ch.challenge();
        // vanishing_poly::get_lut_poly per (round, table): the pairs (inp + B out) as coefficients in delta, first entry highest,
        // zero-padded to whole table rows
        for (uint32_t ci = 0; ci < nc; ci++)
            for (uint32_t t = 0; t < d.num_luts; t++) {
                const uint32_t len = v->lut_sizes[t], slots = v->lk.n_lut_slots;
                const uint32_t degree = slots * ((len + slots - 1) / slots);
                const uint16_t* pr = &v->lut_pairs[2 * (size_t)v->lut_offsets[t]];
                const uint64_t B = deltas[4 * ci + 1], dl = deltas[4 * ci + 3];
                uint64_t acc = 0;
                for (uint32_t i = 0; i < len; i++) acc = gl::add(gl::mul(acc, dl), gl::add((uint64_t)pr[2 * i], gl::mul(B, (uint64_t)pr[2 * i + 1])));
                pp[PP_LUT + ci * d.num_luts + t] = gl::mul(acc, gl::pow(dl, degree - len));
            }
    }
    ch.observe(w + l.w_caps + capw, capw);                            // Zs / partial products cap
    for (uint32_t i = 0; i < nc; i++) pp[PP_ALPHAS + i] = ch.challenge();
    ch.observe(w + l.w_caps + 2 * capw, capw);                        // quotient cap
    ch.ext_challenge(pp + PP_ZETA);
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
    const gl::Ext gzeta = gl::mul(zeta, gl::root_of_unity(d.degree_bits));
    pp[PP_GZETA] = gzeta.a;
    pp[PP_GZETA + 1] = gzeta.b;
    // the openings as the prover observed them: the zeta batch (constants .. zs, then partial products and quotient, then the
    // lookup polynomials), then the g zeta batch
    auto cls = [&](uint32_t c) { return w + l.w_openings[c]; };
    ch.observe(cls(ppl::O_CONSTANTS), 2 * (size_t)(v->n_cs + d.num_wires + nc));
    ch.observe(cls(ppl::O_PARTIAL_PRODUCTS), 2 * (size_t)(nc * d.num_partial_products + v->n_q));
    ch.observe(cls(ppl::O_LOOKUP_ZS), 2 * (size_t)nlk);
    ch.observe(cls(ppl::O_ZS_NEXT), 2 * (size_t)nc);
    ch.observe(cls(ppl::O_LOOKUP_ZS_NEXT), 2 * (size_t)nlk);
    ch.ext_challenge(pp + PP_FRI_ALPHA);
    for (uint32_t k = 0; k < R; k++) {
        ch.observe(w + l.w_fri_caps + k * capw, capw);
        ch.ext_challenge(pp + PP_FRI_BETAS + 2 * k);
    }
    ch.observe(w + l.w_final_poly, 2 * (size_t)l.final_len);
    ch.observe(w[l.w_pow_witness]);
    const uint64_t pow_response = ch.challenge();
    const bool pow_bad = d.fri_pow_bits && (pow_response >> (64 - d.fri_pow_bits)) != 0;
    for (uint32_t q = 0; q < d.fri_num_queries; q++) qidx[q] = (uint32_t)(ch.challenge() & (((uint64_t)1 << l.log_L) - 1));
    {
        // PrecomputedReducedOpenings: sum_j alpha^j opened[j] per batch.  The lookup polynomials sit after the quotient in the
        // zeta batch and after the Zs in the g zeta batch.
        const gl::Ext fa{pp[PP_FRI_ALPHA], pp[PP_FRI_ALPHA + 1]};
        gl::Ext ap{1, 0}, r0{0, 0}, r1{0, 0};
        auto run = [&](gl::Ext& r, uint32_t c, size_t count) {
            const uint64_t* o = cls(c);
            for (size_t j = 0; j < count; j++) {
                r = gl::add(r, gl::mul(ap, gl::Ext{o[2 * j], o[2 * j + 1]}));
                ap = gl::mul(ap, fa);
            }
        };
        run(r0, ppl::O_CONSTANTS, (size_t)v->n_cs + d.num_wires + nc);   // constants, sigmas, wires, zs: contiguous
        run(r0, ppl::O_PARTIAL_PRODUCTS, (size_t)nc * d.num_partial_products + v->n_q);
        run(r0, ppl::O_LOOKUP_ZS, nlk);
        ap = gl::Ext{1, 0};
        run(r1, ppl::O_ZS_NEXT, nc);
        run(r1, ppl::O_LOOKUP_ZS_NEXT, nlk);
        pp[PP_RED0] = r0.a; pp[PP_RED0 + 1] = r0.b;
        pp[PP_RED1] = r1.a; pp[PP_RED1 + 1] = r1.b;
    }
    {
        // eval_l_0(n, zeta) = (zeta^n - 1) / (n (zeta - 1))
        gl::Ext zeta_n = zeta;
        for (uint32_t k = 0; k < d.degree_bits; k++) zeta_n = gl::mul(zeta_n, zeta_n);
        const gl::Ext z_h = gl::sub(zeta_n, gl::Ext{1, 0});
        const gl::Ext l0 = gl::mul(z_h, gl::inv(gl::mul(gl::sub(zeta, gl::Ext{1, 0}), (uint64_t)1 << d.degree_bits)));
        pp[PP_L0] = l0.a;
        pp[PP_L0 + 1] = l0.b;
    }
    return pow_bad;
}

void fill_cons_params(const nlx_verifier* v, ConsParams& cp) {
    const nlx_circuit_desc& d = v->d;
    const ppl::Layout& l = v->lay;
    const uint32_t nc = d.num_challenges;
    cp.n_gates = d.num_gates; cp.nc = nc; cp.npp = d.num_partial_products; cp.routed = d.num_routed_wires;
    cp.chunk = d.quotient_degree_factor; cp.num_wires = d.num_wires; cp.num_constants = d.num_constants;
    cp.num_selectors = d.num_selectors; cp.n_lk_sel = v->n_lk_sel; cp.n_lk_terms = v->n_lk_terms;
    cp.n_lk_per_round = d.num_luts ? 1 + v->lk.n_sldc : 0;
    cp.n_items = d.num_gates + nc + (d.num_luts ? nc : 0);
    const size_t w0 = l.w_openings[0];
    auto el = [&](uint32_t c) { return (uint32_t)((l.w_openings[c] - w0) / 2); };
    cp.e_consts = el(ppl::O_CONSTANTS); cp.e_sigmas = el(ppl::O_SIGMAS); cp.e_wires = el(ppl::O_WIRES); cp.e_zs = el(ppl::O_ZS);
    cp.e_zs_next = el(ppl::O_ZS_NEXT); cp.e_lk = el(ppl::O_LOOKUP_ZS); cp.e_lk_next = el(ppl::O_LOOKUP_ZS_NEXT);
    cp.e_pp = el(ppl::O_PARTIAL_PRODUCTS);
    cp.lk = v->lk;
}

int32_t verify_batch(nlx_verifier* v, VerifyCall& vc, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                     const uint64_t* public_inputs, nlx_proof_verdict* verdicts) {
    nlx_ctx* ctx = v->ctx;
    const nlx_circuit_desc& d = v->d;
    const ppl::Layout& l = v->lay;
    hipStream_t st = ctx->stream;
    const uint32_t nQ = d.fri_num_queries, nc = d.num_challenges, qdf = d.quotient_degree_factor, n_pis = d.num_public_inputs;
    const uint32_t R = l.n_layers, nlk = v->n_lk_polys;
    const unsigned log_n = d.degree_bits;
    const size_t capw = l.cap_words;
    const size_t open_words = l.w_fri_caps - l.w_openings[0];
    auto reject = [&](size_t i, uint32_t reason) -> nlx_proof_verdict& {
        verdicts[i].accepted = 0;
        verdicts[i].reason = reason;
        return verdicts[i];
    };

    // ---- host: structure, public inputs, transcript, proof of work, query indices ----
    std::vector<size_t> live;            // proofs that reach the device, by index
    std::vector<uint8_t> pow_bad;        // per live proof
    vc.stage.reserve(l.w_total);
    for (size_t i = 0; i < n_proofs; i++) {
        const size_t at = live.size();
        vc.stage.resize((at + 1) * l.w_total);
        uint64_t* w = vc.stage.data() + at * l.w_total;
        ppl::Finding f;
        if (ppl::parse(l, proofs[i], lens[i], w, &f) != ppl::SOUND) {
            nlx_proof_verdict& vd = reject(i, NLX_VERIFY_MALFORMED);
            if (f.what == ppl::BAD_PATH_LENGTH) {
                vd.query = f.query;
                if (f.tree < ppl::N_TREES) vd.tree = f.tree;
                else vd.layer = f.layer;
            }
            continue;
        }
        if (public_inputs && memcmp(public_inputs + i * n_pis, w + l.w_public_inputs, 8 * (size_t)n_pis) != 0) {
            reject(i, NLX_VERIFY_PUBLIC_INPUTS);
            continue;
        }
        vc.pp.resize((at + 1) * PP_STRIDE, 0);
        vc.qidx.resize((at + 1) * nQ);
        pow_bad.push_back(host_transcript(v, w, vc.pp.data() + at * PP_STRIDE, vc.qidx.data() + at * nQ));
        live.push_back(i);
    }
    const size_t np = live.size();
    if (np) {
        // the openings as [word][proof]: a wave of the constraint kernel reads one word of its 64 proofs in one line
        vc.open.resize(open_words * np);
        for (size_t at = 0; at < np; at++) {
            const uint64_t* o = vc.stage.data() + at * l.w_total + l.w_openings[0];
            for (size_t k = 0; k < open_words; k++) vc.open[k * np + at] = o[k];
        }
        // ---- device ----
        (void)hipSetDevice(ctx->device);
        Scratch& scratch = vc.scratch;
        const uint32_t n_trees = ppl::N_TREES + R;
        const size_t n_items = np * nQ;
        if (n_items > 0x7FFFFFFFu) return ctx->fail(NLX_E_RANGE, "too many proofs in one batch");
        ConsParams cp{};
        fill_cons_params(v, cp);
        const size_t part_words = np * cp.n_items * nc * 2;
        uint64_t* d_stage = scratch.alloc_as<uint64_t>(np * l.w_total * 8);
        uint64_t* d_open = scratch.alloc_as<uint64_t>(open_words * np * 8);
        uint64_t* d_pp = scratch.alloc_as<uint64_t>(np * PP_STRIDE * 8);
        uint32_t* d_qidx = scratch.alloc_as<uint32_t>(n_items * 4);
        uint8_t* d_path_fail = scratch.alloc_as<uint8_t>(n_items * n_trees);
        uint32_t* d_fri_fail = scratch.alloc_as<uint32_t>(n_items * 4);
        uint64_t* d_part = scratch.alloc_as<uint64_t>(part_words * 8);
        if (!d_stage || !d_open || !d_pp || !d_qidx || !d_path_fail || !d_fri_fail || !d_part) return ctx->fail(NLX_E_NOMEM, "out of device memory");
        NLX_HIP(ctx, hipMemcpyAsync(d_stage, vc.stage.data(), np * l.w_total * 8, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemcpyAsync(d_open, vc.open.data(), open_words * np * 8, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemcpyAsync(d_pp, vc.pp.data(), np * PP_STRIDE * 8, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemcpyAsync(d_qidx, vc.qidx.data(), n_items * 4, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemsetAsync(d_path_fail, 0xFF, n_items * n_trees, st));   // as the two below: what no kernel writes
        NLX_HIP(ctx, hipMemsetAsync(d_fri_fail, 0xFF, n_items * 4, st));
        NLX_HIP(ctx, hipMemsetAsync(d_part, 0xFF, part_words * 8, st));   // an item that did not run can never pass for one that did

        {
            PathParams pa{};
            pa.stage = d_stage; pa.cs_cap = v->d_cs_cap; pa.qidx = d_qidx; pa.fail = d_path_fail;
            pa.w_total = l.w_total; pa.w_queries = l.w_queries; pa.w_query_words = l.w_query_words;
            pa.n_items = (uint32_t)n_items; pa.n_queries = nQ; pa.n_trees = n_trees;
            for (uint32_t o = 0; o < ppl::N_TREES; o++)
                pa.trees[o] = VTree{(uint32_t)l.w_row[o], l.tree_cols[o], (uint32_t)l.w_path[o], l.tree_plen,
                                    o ? (uint32_t)(l.w_caps + (o - 1) * capw) : 0, 0, o ? 1u : 0u, 0};
            for (uint32_t k = 0; k < R; k++)
                pa.trees[ppl::N_TREES + k] = VTree{(uint32_t)l.w_layer_evals[k], 2 * l.arity, (uint32_t)l.w_layer_path[k], l.layer_plen[k],
                                                   (uint32_t)(l.w_fri_caps + k * capw), (k + 1) * d.fri_arity_bits, 1, 0};
            size_t perms = 0;
            for (uint32_t t = 0; t < n_trees; t++) perms += (pa.trees[t].width + 7) / 8 + pa.trees[t].path_len;
            ctx->begin_kernel("plonk_verify_paths", 8.0 * np * l.w_total, (double)perms * n_items);
            hipLaunchKernelGGL(k_plonk_paths, dim3((unsigned)((n_items + 15) / 16), n_trees), dim3(64), 0, st, pa);
            ctx->end_kernel();
        }
        {
            FriParams fp{};
            fp.stage = d_stage; fp.pp = d_pp; fp.qidx = d_qidx; fp.fail = d_fri_fail;
            fp.w_total = l.w_total; fp.w_queries = l.w_queries; fp.w_query_words = l.w_query_words; fp.w_final_poly = l.w_final_poly;
            fp.n_queries = nQ; fp.log_L = l.log_L; fp.arity_bits = d.fri_arity_bits; fp.n_layers = R; fp.final_len = l.final_len;
            // the zeta batch walks constants_sigmas, wires, the Zs and partial products, the quotient, then the lookup columns of
            // the Zs row; the g zeta batch takes the Zs, then the lookup columns
            uint32_t pow0 = 0, ns = 0;
            auto seg = [&](uint32_t tree, uint32_t col0, uint32_t count, uint32_t batch, uint32_t& pw) {
                if (count) fp.seg[ns++] = FriSeg{(uint32_t)l.w_row[tree] + col0, count, pw, batch};
                pw += count;
            };
            seg(0, 0, v->n_cs, 0, pow0);
            seg(1, 0, d.num_wires, 0, pow0);
            seg(2, 0, v->n_zpp, 0, pow0);
            seg(3, 0, v->n_q, 0, pow0);
            seg(2, v->n_zpp, nlk, 0, pow0);
            uint32_t pow1 = 0;
            seg(2, 0, nc, 1, pow1);
            seg(2, v->n_zpp, nlk, 1, pow1);
            fp.n_segs = ns;
            fp.n_batch1 = nc + nlk;
            for (uint32_t k = 0; k < R; k++) fp.w_layer_evals[k] = (uint32_t)l.w_layer_evals[k];
            ctx->begin_kernel("plonk_verify_fri", 8.0 * n_items * l.w_query_words);
            hipLaunchKernelGGL(k_plonk_fri, dim3((unsigned)n_items), dim3(64), 0, st, fp);
            ctx->end_kernel();
        }
        {
            cp.open = d_open; cp.pp = d_pp; cp.gates = v->d_gates; cp.k_is = v->d_k_is; cp.part = d_part;
            cp.n_proofs = (uint32_t)np;
            unsigned bs = 64;
            while (bs > 1 && bs / 2 >= np) bs >>= 1;
            ctx->begin_kernel("plonk_verify_constraints", 8.0 * np * open_words);
            hipLaunchKernelGGL(k_plonk_constraints, dim3((unsigned)((np + bs - 1) / bs), cp.n_items), dim3(bs), 0, st, cp);
            ctx->end_kernel();
        }
        std::vector<uint8_t> path_fail(n_items * n_trees);
        std::vector<uint32_t> fri_fail(n_items);
        std::vector<uint64_t> part(part_words);
        NLX_RC(fetch(ctx, path_fail.data(), d_path_fail, path_fail.size()));
        NLX_RC(fetch(ctx, fri_fail.data(), d_fri_fail, fri_fail.size() * 4));
        NLX_RC(fetch(ctx, part.data(), d_part, part_words * 8));
        for (uint8_t f : path_fail)
            if (f > 1) return ctx->fail(NLX_E_HIP, "the path kernel left a tree unwritten");
        for (uint64_t pw : part)
            if (pw >= gl::P) return ctx->fail(NLX_E_HIP, "the constraint kernel left an item unwritten");

        // ---- the verdicts, in the order of a sequential verifier ----
        const uint32_t t_gate = nc + nc * (d.num_partial_products + 1) + nc * v->n_lk_terms;
        for (size_t at = 0; at < np; at++) {
            const size_t i = live[at];
            const uint64_t* w = vc.stage.data() + at * l.w_total;
            const uint64_t* pp = vc.pp.data() + at * PP_STRIDE;
            const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
            gl::Ext zeta_n = zeta;
            for (unsigned k = 0; k < log_n; k++) zeta_n = gl::mul(zeta_n, zeta_n);
            const gl::Ext z_h = gl::sub(zeta_n, gl::Ext{1, 0});
            bool done = false;
            for (uint32_t j = 0; j < nc && !done; j++) {
                gl::Ext gates{0, 0}, rest{0, 0}, t{0, 0};
                for (uint32_t it = 0; it < cp.n_items; it++) {
                    const uint64_t* pv = part.data() + ((at * cp.n_items + it) * nc + j) * 2;
                    if (it < d.num_gates) gates = gl::add(gates, gl::Ext{pv[0], pv[1]});
                    else rest = gl::add(rest, gl::Ext{pv[0], pv[1]});
                }
                const gl::Ext sum = gl::add(rest, gl::mul(gates, gl::pow(pp[PP_ALPHAS + j], t_gate)));
                const uint64_t* o_q = w + l.w_openings[ppl::O_QUOTIENT] + 2 * (size_t)j * qdf;
                for (uint32_t k = qdf; k-- > 0;) t = gl::add(gl::mul(t, zeta_n), gl::Ext{o_q[2 * k], o_q[2 * k + 1]});
                if (!gl::eq(sum, gl::mul(z_h, t))) {
                    reject(i, NLX_VERIFY_CONSTRAINTS).challenge = j;
                    done = true;
                }
            }
            if (done) continue;
            if (pow_bad[at]) {
                reject(i, NLX_VERIFY_POW);
                continue;
            }
            for (uint32_t q = 0; q < nQ && !done; q++) {
                const size_t item = at * nQ + q;
                const uint8_t* pf = path_fail.data() + item * n_trees;
                const uint32_t ff = fri_fail[item];
                if (ff == 0xFFFFFFFFu) return ctx->fail(NLX_E_HIP, "the FRI kernel left a query unwritten");
                uint32_t reason = 0, tree = 0, layer = 0;
                for (uint32_t o = 0; o < ppl::N_TREES && !reason; o++)
                    if (pf[o]) { reason = NLX_VERIFY_TRACE_PATH; tree = o; }
                for (uint32_t k = 0; k < R && !reason; k++) {
                    if ((ff >> 8) == FRI_FAIL_FOLD && (ff & 0xFF) == k) { reason = NLX_VERIFY_FRI_FOLD; layer = k; }
                    else if (pf[ppl::N_TREES + k]) { reason = NLX_VERIFY_FRI_PATH; layer = k; }
                }
                if (!reason && (ff >> 8) == FRI_FAIL_FINAL) reason = NLX_VERIFY_FINAL_POLY;
                if (reason) {
                    nlx_proof_verdict& vd = reject(i, reason);
                    vd.query = q; vd.tree = tree; vd.layer = layer; vd.x_index = vc.qidx[item];
                    done = true;
                }
            }
            if (!done) {
                verdicts[i].accepted = 1;
                verdicts[i].reason = NLX_VERIFY_ACCEPT;
            }
        }
    }
    for (size_t i = 0; i < n_proofs; i++)
        if (!verdicts[i].accepted) {
            const nlx_proof_verdict& vd = verdicts[i];
            // NLX_OK: the check ran.  The line is for nlx_last_error.
            ctx->fail(NLX_OK, "proof %llu does not verify: %s (reason %u), challenge %u, query %u (x_index %llu), tree %u, layer %u",
                      (unsigned long long)i, reason_name(vd.reason), vd.reason, vd.challenge, vd.query, (unsigned long long)vd.x_index, vd.tree, vd.layer);
            return NLX_OK;
        }
    ctx->err.clear();   // every proof verifies: no line of an earlier rejection stays behind
    return NLX_OK;
}

}  // namespace

extern "C" {

int32_t nlx_verifier_create(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap,
                            const uint64_t digest[4], nlx_verifier** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !constants_sigmas_cap || !digest || !out || !desc->gates || !desc->k_is) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    NLX_RC(validate_circuit_desc(ctx, *desc, NLX_HASHER_POSEIDON_GOLDILOCKS));
    bool zero = true;
    for (int i = 0; i < 4; i++) zero = zero && desc->circuit_digest[i] == 0;
    if (!zero && memcmp(desc->circuit_digest, digest, 32) != 0)
        return ctx->fail(NLX_E_INVAL, "the descriptor's circuit_digest differs from the verifier-only data's");
    return verifier_build(ctx, *desc, constants_sigmas_cap, digest, out);
} NLX_CATCH(ctx)

int32_t nlx_verifier_from_circuit(const nlx_circuit* c, nlx_verifier** out) NLX_TRY {
    if (!c || !out) return NLX_E_INVAL;
    *out = nullptr;
    nlx_ctx* ctx = circuit_ctx(c);
    if (nlx_circuit_hasher(c) != NLX_HASHER_POSEIDON_GOLDILOCKS)
        return ctx->fail(NLX_E_UNSUPPORTED, "proofs under the PoseidonBN128 config are not verified on the device");
    const nlx_circuit_desc& d = circuit_desc(c);
    std::vector<uint64_t> cap((size_t)4 << d.cap_height);
    NLX_RC(nlx_circuit_constants_sigmas_cap(c, cap.data()));
    return verifier_build(ctx, d, cap.data(), d.circuit_digest, out);
} NLX_CATCH(c ? circuit_ctx(c) : nullptr)

void nlx_verifier_destroy(nlx_verifier* v) NLX_TRY {
    if (!v) return;
    nlx_ctx* ctx = v->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->release(v->d_block);
    delete v;
} NLX_CATCH_VOID(nullptr)

size_t nlx_verifier_proof_bytes(const nlx_verifier* v) NLX_TRY {
    return v ? v->lay.total : 0;
} NLX_CATCH_VALUE(nullptr, 0)

int32_t nlx_verify_batch(nlx_verifier* v, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                         const uint64_t* public_inputs, nlx_proof_verdict* verdicts) NLX_TRY {
    if (verdicts && n_proofs) memset(verdicts, 0, n_proofs * sizeof *verdicts);
    if (!v) return NLX_E_INVAL;
    nlx_ctx* ctx = v->ctx;
    if (n_proofs && (!proofs || !lens || !verdicts)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ctx->fail(NLX_E_INVAL, "proof %llu is NULL", (unsigned long long)i);
    if (public_inputs)
        for (size_t i = 0; i < n_proofs * v->d.num_public_inputs; i++)
            if (public_inputs[i] >= gl::P)
                return ctx->fail(NLX_E_RANGE, "public input %llu of proof %llu is not canonical", (unsigned long long)(i % v->d.num_public_inputs),
                                 (unsigned long long)(i / v->d.num_public_inputs));
    if (!n_proofs) return NLX_OK;
    VerifyCall vc(ctx);
    const int32_t rc = vc.scratch.finish(verify_batch(v, vc, proofs, lens, n_proofs, public_inputs, verdicts));
    if (rc) memset(verdicts, 0, n_proofs * sizeof *verdicts);   // an error is no verdict
    return rc;
} NLX_CATCH(v ? v->ctx : nullptr)

int32_t nlx_verify(nlx_verifier* v, const uint8_t* proof, size_t len, const uint64_t* public_inputs, nlx_proof_verdict* verdict) NLX_TRY {
    if (verdict) memset(verdict, 0, sizeof *verdict);
    if (!v) return NLX_E_INVAL;
    if (!proof || !verdict) return v->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_verify_batch(v, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(v ? v->ctx : nullptr)

}  // extern "C"
