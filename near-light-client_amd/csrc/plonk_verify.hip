// plonky2 verifier (C ABI: nlx_verifier_*, nlx_verify, nlx_verify_batch): does a ProofWithPublicInputs verify, and if not, which
// check breaks.
//
// plonky2::plonk::verifier::verify + fri::verifier::verify_fri_proof for the proofs of prover.hip, one proof or a batch of proofs
// of one circuit.  What a plonky2 proof shares with every proof that has a FRI proof in it is fri_verify.hip's: the parser, the
// transcript from the FRI caps on, the path and query kernels, the verdicts.  Here is what is plonky2's own: the head of the
// transcript (plonk_proof_layout.hpp) with the public-inputs hash, get_lut_poly and L_0(zeta), the seven runs of opened columns
// that enter the FRI batches, and the third launch with its judgement:
//   k_plonk_constraints  one lane per proof, one block row per gate (then per challenge: the permutation argument, the lookup
//                        argument): the constraints at zeta over F_p[X]/(X^2 - 7) (gate_eval_ext.hpp), on the openings
//                        transposed to [word][proof]
// A verifier carries its config's Hasher (nlx_verifier_create_hasher, nlx_verifier_from_circuit_hasher):
// under NLX_HASHER_POSEIDON_BN128 the circuit digest and the caps enter the transcript through observe_hash, the parser checks
// digests against r, and the path launch is fri_verify.hip's k_fri_paths_bn128.  The constraint launch, the FRI launch and the
// judgement do not know of it.
#include <algorithm>
#include <memory>
#include <vector>
#include "fri_verify.hpp"
#include "gate_eval_ext.hpp"
#include "plonk_proof_layout.hpp"
#include "prover.hpp"

using namespace nlx;

namespace nlx {
namespace pv {

using namespace fv;
// per proof, what the transcript gave after the common prefix (64-bit words)
enum : uint32_t { PP_ALPHAS = PP_OWN, PP_BETAS = PP_ALPHAS + 2, PP_GAMMAS = PP_BETAS + 2, PP_PIH = PP_GAMMAS + 2, PP_L0 = PP_PIH + 4,
                  PP_DELTAS = PP_L0 + 2, PP_LUT = PP_DELTAS + 8, PP_STRIDE = PP_LUT + 32 };
constexpr uint64_t UNUSED_SELECTOR = 0xFFFFFFFFULL;          // gates::selectors::UNUSED_SELECTOR

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
    uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS;   // the config's Hasher: of every tree, the cap and the digest
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
                      uint32_t hasher, std::vector<GateDev>& gd) {
    v->ctx = ctx;
    v->hasher = hasher;
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
    if (hasher == NLX_HASHER_POSEIDON_BN128) {
        // digests of this hasher: one integer below r each, whatever its words are against p
        if (fpl::first_digest_not_below_r(v->cs_cap.data(), 0, capw) != capw)
            return ctx->fail(NLX_E_RANGE, "a digest of constants_sigmas_cap is not below r");
        if (!pbn::lt_r(digest[0], digest[1], digest[2], digest[3])) return ctx->fail(NLX_E_RANGE, "circuit_digest is not below r");
    } else {
        for (uint64_t w : v->cs_cap)
            if (w >= gl::P) return ctx->fail(NLX_E_RANGE, "a word of constants_sigmas_cap is not canonical");
    }
    memcpy(v->digest, digest, 32);
    memcpy(v->d.circuit_digest, digest, 32);
    ppl::Shape sh{};
    sh.degree_bits = d.degree_bits; sh.rate_bits = d.rate_bits; sh.cap_height = d.cap_height; sh.arity_bits = d.fri_arity_bits;
    sh.final_poly_bits = d.fri_final_poly_bits; sh.n_queries = d.fri_num_queries; sh.n_pis = d.num_public_inputs;
    sh.n_constants = v->n_consts_all; sh.n_sigmas = d.num_routed_wires; sh.n_wires = d.num_wires; sh.n_challenges = d.num_challenges;
    sh.n_partial = d.num_challenges * d.num_partial_products; sh.n_lookup_polys = v->n_lk_polys; sh.n_quotient = v->n_q;
    if (!ppl::make_layout(sh, &v->lay, hasher) || v->lay.n_layers != v->n_fri_rounds)
        return ctx->fail(NLX_E_UNSUPPORTED, "the circuit's proofs have a shape the verifier does not take");
    if (d.num_gates + 2 * d.num_challenges > 65535) return ctx->fail(NLX_E_RANGE, "too many gate kinds");
    if (d.fri_num_queries == 0) return ctx->fail(NLX_E_RANGE, "a proof without FRI queries is not verified");
    return NLX_OK;
}

int32_t verifier_build(nlx_ctx* ctx, const nlx_circuit_desc& d, const uint64_t* cap, const uint64_t digest[4], uint32_t hasher,
                       nlx_verifier** out) {
    std::unique_ptr<nlx_verifier> v(new nlx_verifier());
    std::vector<GateDev> gd;
    NLX_RC(verifier_fill(ctx, v.get(), d, cap, digest, hasher, gd));
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

// the head of one proof's chain: the transcript up to the FRI alpha, the reduced openings, get_lut_poly, L_0(zeta).  w: the
// staging copy; pp: PP_STRIDE words, zeroed.  Rules 1 - 5 of DESIGN.md section 17: the circuit digest and every cap enter through
// observe_hash - under BN128 five limbs a digest, each found below r by verifier_fill or the parser -, while the public-inputs
// hash and the sponge stay Goldilocks under both configs.
void transcript_head(const nlx_verifier* v, const uint64_t* w, uint64_t* pp, Challenger& ch) {
    const nlx_circuit_desc& d = v->d;
    const ppl::Layout& l = v->lay;
    const uint32_t nc = d.num_challenges, nlk = v->n_lk_polys;
    const size_t capw = l.cap_words;
    const uint64_t* pis = w + l.w_public_inputs;
    hash_no_pad_host(pis, d.num_public_inputs, pp + PP_PIH);
    (void)observe_hash(v->hasher, ch, v->digest, 1);
    ch.observe(pp + PP_PIH, 4);
    (void)observe_hash(v->hasher, ch, w + l.w_caps, capw / 4);        // wires cap
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
    (void)observe_hash(v->hasher, ch, w + l.w_caps + capw, capw / 4);   // Zs / partial products cap
    for (uint32_t i = 0; i < nc; i++) pp[PP_ALPHAS + i] = ch.challenge();
    (void)observe_hash(v->hasher, ch, w + l.w_caps + 2 * capw, capw / 4);   // quotient cap
    const gl::Ext zeta = draw_zeta(ch, pp, d.degree_bits);
    // the openings as the prover observed them: the zeta batch (constants .. zs, then partial products and quotient, then the
    // lookup polynomials), then the g zeta batch.  constants, sigmas, wires, zs are contiguous.
    auto cls = [&](uint32_t c) { return w + l.w_openings[c]; };
    const ExtRun head{cls(ppl::O_CONSTANTS), (size_t)v->n_cs + d.num_wires + nc};
    const ExtRun pp_q{cls(ppl::O_PARTIAL_PRODUCTS), (size_t)nc * d.num_partial_products + v->n_q};
    const ExtRun lk{cls(ppl::O_LOOKUP_ZS), nlk}, zs_next{cls(ppl::O_ZS_NEXT), nc}, lk_next{cls(ppl::O_LOOKUP_ZS_NEXT), nlk};
    for (const ExtRun& r : {head, pp_q, lk, zs_next, lk_next}) ch.observe(r.o, 2 * r.count);
    ch.ext_challenge(pp + PP_FRI_ALPHA);
    // PrecomputedReducedOpenings: the lookup polynomials sit after the quotient in the zeta batch and after the Zs in the g zeta one
    reduce_openings(pp, {head, pp_q, lk}, pp + PP_RED0);
    reduce_openings(pp, {zs_next, lk_next}, pp + PP_RED1);
    // eval_l_0(n, zeta) = (zeta^n - 1) / (n (zeta - 1))
    const gl::Ext l0 = gl::mul(ZetaN(zeta, d.degree_bits).z_h, gl::inv(gl::mul(gl::sub(zeta, gl::Ext{1, 0}), (uint64_t)1 << d.degree_bits)));
    pp[PP_L0] = l0.a;
    pp[PP_L0 + 1] = l0.b;
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

// What one call holds until its stream work has drained: the transposed openings outlive the scratch, which synchronises.
struct PlonkCall {
    std::vector<uint64_t> open;
    VerifyCall base;
    explicit PlonkCall(nlx_ctx* ctx) : base(ctx) {}
};

int32_t verify_batch(nlx_verifier* v, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs, const uint64_t* public_inputs,
                     nlx_proof_verdict* verdicts) {
    nlx_ctx* ctx = v->ctx;
    const nlx_circuit_desc& d = v->d;
    const ppl::Layout& l = v->lay;
    const uint32_t nc = d.num_challenges, qdf = d.quotient_degree_factor, nlk = v->n_lk_polys;
    const size_t open_words = l.w_fri_caps - l.w_openings[0];
    PlonkCall call(ctx);
    ConsParams cp{};
    fill_cons_params(v, cp);
    Verifier fvv;
    fvv.ctx = ctx; fvv.lay = &l; fvv.hasher = v->hasher;
    fvv.log_n = d.degree_bits; fvv.arity_bits = d.fri_arity_bits; fvv.pow_bits = d.fri_pow_bits; fvv.pp_stride = PP_STRIDE;
    fvv.w_caps = l.w_caps; fvv.ext_cap = v->d_cs_cap;   // tree 0 is the circuit's own constants_sigmas
    // the zeta batch walks constants_sigmas, wires, the Zs and partial products, the quotient, then the lookup columns of the Zs
    // row; the g zeta batch takes the Zs, then the lookup columns
    uint32_t pow0 = 0, pow1 = 0;
    auto run = [&](uint32_t tree, uint32_t col0, uint32_t count, uint32_t batches, uint32_t& pw) {
        if (count) fvv.runs[fvv.n_runs++] = FriRun{(uint32_t)l.w_row[tree] + col0, count, pw, batches};
        pw += count;
    };
    run(0, 0, v->n_cs, 1, pow0);
    run(1, 0, d.num_wires, 1, pow0);
    run(2, 0, v->n_zpp, 1, pow0);
    run(3, 0, v->n_q, 1, pow0);
    run(2, v->n_zpp, nlk, 1, pow0);
    run(2, 0, nc, 2, pow1);
    run(2, v->n_zpp, nlk, 2, pow1);
    fvv.batch_shift = pow1;
    fvv.part_words = (size_t)cp.n_items * nc * 2;
    fvv.name_paths = v->hasher == NLX_HASHER_POSEIDON_BN128 ? "plonk_verify_paths_bn128" : "plonk_verify_paths"; fvv.name_fri = "plonk_verify_fri";
    fvv.part_unwritten = "the constraint kernel left an item unwritten";
    fvv.head = [&](const uint64_t* w, uint64_t* pp, Challenger& ch) { transcript_head(v, w, pp, ch); };
    fvv.constraints = [&](const Device& dev) {
        // the openings as [word][proof]: a wave of the constraint kernel reads one word of its 64 proofs in one line
        const size_t np = dev.n_proofs;
        call.open.resize(open_words * np);
        for (size_t at = 0; at < np; at++) {
            const uint64_t* o = call.base.stage.data() + at * l.w_total + l.w_openings[0];
            for (size_t k = 0; k < open_words; k++) call.open[k * np + at] = o[k];
        }
        uint64_t* d_open = call.base.scratch.alloc_as<uint64_t>(open_words * np * 8);
        if (!d_open) return ctx->fail(NLX_E_NOMEM, "out of device memory");
        NLX_HIP(ctx, hipMemcpyAsync(d_open, call.open.data(), open_words * np * 8, hipMemcpyHostToDevice, ctx->stream));
        cp.open = d_open; cp.pp = dev.pp; cp.gates = v->d_gates; cp.k_is = v->d_k_is; cp.part = dev.part;
        cp.n_proofs = (uint32_t)np;
        unsigned bs = 64;
        while (bs > 1 && bs / 2 >= np) bs >>= 1;
        ctx->begin_kernel("plonk_verify_constraints", 8.0 * np * open_words);
        hipLaunchKernelGGL(k_plonk_constraints, dim3((unsigned)((np + bs - 1) / bs), cp.n_items), dim3(bs), 0, ctx->stream, cp);
        ctx->end_kernel();
        return (int32_t)NLX_OK;
    };
    const uint32_t t_gate = nc + nc * (d.num_partial_products + 1) + nc * v->n_lk_terms;
    fvv.judge = [&](const uint64_t* w, const uint64_t* pp, const uint64_t* part) {
        const ZetaN z(gl::Ext{pp[PP_ZETA], pp[PP_ZETA + 1]}, d.degree_bits);
        for (uint32_t j = 0; j < nc; j++) {
            gl::Ext gates{0, 0}, rest{0, 0};
            for (uint32_t it = 0; it < cp.n_items; it++) {
                const gl::Ext pv{part[(it * nc + j) * 2], part[(it * nc + j) * 2 + 1]};
                if (it < d.num_gates) gates = gl::add(gates, pv);
                else rest = gl::add(rest, pv);
            }
            const gl::Ext sum = gl::add(rest, gl::mul(gates, gl::pow(pp[PP_ALPHAS + j], t_gate)));
            if (!z.divides(sum, w + l.w_openings[ppl::O_QUOTIENT] + 2 * (size_t)j * qdf, qdf)) return j;
        }
        return NO_CHALLENGE;
    };
    return fv::verify_batch(fvv, call.base, proofs, lens, n_proofs, public_inputs, verdicts);
}

// nlx_verifier_create and nlx_verifier_create_hasher
int32_t verifier_create(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t digest[4],
                        uint32_t hasher, nlx_verifier** out) {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !constants_sigmas_cap || !digest || !out || !desc->gates || !desc->k_is) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    NLX_RC(validate_circuit_desc(ctx, *desc, hasher));
    bool zero = true;
    for (int i = 0; i < 4; i++) zero = zero && desc->circuit_digest[i] == 0;
    if (!zero && memcmp(desc->circuit_digest, digest, 32) != 0)
        return ctx->fail(NLX_E_INVAL, "the descriptor's circuit_digest differs from the verifier-only data's");
    return verifier_build(ctx, *desc, constants_sigmas_cap, digest, hasher, out);
}

}  // namespace

extern "C" {

int32_t nlx_verifier_create(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap,
                            const uint64_t digest[4], nlx_verifier** out) NLX_TRY {
    return verifier_create(ctx, desc, constants_sigmas_cap, digest, NLX_HASHER_POSEIDON_GOLDILOCKS, out);
} NLX_CATCH(ctx)

int32_t nlx_verifier_create_hasher(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap,
                                   const uint64_t digest[4], uint32_t hasher, nlx_verifier** out) NLX_TRY {
    return verifier_create(ctx, desc, constants_sigmas_cap, digest, hasher, out);
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
    return verifier_build(ctx, d, cap.data(), d.circuit_digest, NLX_HASHER_POSEIDON_GOLDILOCKS, out);
} NLX_CATCH(c ? circuit_ctx(c) : nullptr)

int32_t nlx_verifier_from_circuit_hasher(const nlx_circuit* c, uint32_t hasher, nlx_verifier** out) NLX_TRY {
    if (!c || !out) return NLX_E_INVAL;
    *out = nullptr;
    nlx_ctx* ctx = circuit_ctx(c);
    if (hasher != NLX_HASHER_POSEIDON_GOLDILOCKS && hasher != NLX_HASHER_POSEIDON_BN128) return ctx->fail(NLX_E_RANGE, "unknown hasher %u", hasher);
    if ((uint32_t)nlx_circuit_hasher(c) != hasher)
        return ctx->fail(NLX_E_INVAL, "the circuit was built under hasher %d, not %u", nlx_circuit_hasher(c), hasher);
    const nlx_circuit_desc& d = circuit_desc(c);
    std::vector<uint64_t> cap((size_t)4 << d.cap_height);
    NLX_RC(nlx_circuit_constants_sigmas_cap(c, cap.data()));
    return verifier_build(ctx, d, cap.data(), d.circuit_digest, hasher, out);
} NLX_CATCH(c ? circuit_ctx(c) : nullptr)

int32_t nlx_verifier_hasher(const nlx_verifier* v) NLX_TRY {
    return v ? (int32_t)v->hasher : NLX_E_INVAL;
} NLX_CATCH_VALUE(nullptr, NLX_E_INVAL)

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
    NLX_RC(check_batch_args(v->ctx, proofs, lens, n_proofs, public_inputs, v->d.num_public_inputs, verdicts));
    return n_proofs ? verify_batch(v, proofs, lens, n_proofs, public_inputs, verdicts) : NLX_OK;
} NLX_CATCH(v ? v->ctx : nullptr)

int32_t nlx_verify(nlx_verifier* v, const uint8_t* proof, size_t len, const uint64_t* public_inputs, nlx_proof_verdict* verdict) NLX_TRY {
    if (verdict) memset(verdict, 0, sizeof *verdict);
    if (!v) return NLX_E_INVAL;
    if (!proof || !verdict) return v->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_verify_batch(v, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(v ? v->ctx : nullptr)

}  // extern "C"
