// What the two device verifiers share (stark_verify.hip, plonk_verify.hip): everything of a proof from its
// FRI commit caps onwards, and the batch call around it.  A verifier describes its format in a Verifier - layout, trees, the runs
// of opened columns that enter the two FRI batches - and plugs in what is its own: the head of the transcript, the constraint
// launch and the judgement of what that launch leaves.  fri_verify.hip has the two kernels every verifier runs
//   k_fri_paths    one quad of lanes per (proof, query, tree): leaf digest of the opened row, the sibling path, the cap
//                  (k_fri_paths_bn128 for a verifier whose trees are PoseidonBN128's: DESIGN.md section 33)
//   k_fri_queries  one wave per (proof, query): fri_combine_initial, the fold chain, the final polynomial; and one wave per
//                  (proof, periodic column) of a verifier that has such columns
// and the host driver from parsing to the verdicts.
#pragma once
#include <functional>
#include <vector>
#include "fri_proof_layout.hpp"
#include "gl.hpp"
#include "transcript.hpp"

namespace nlx {
namespace fv {

// per proof, what the transcript gave (64-bit words): this prefix, then the verifier's own words
enum : uint32_t { PP_ZETA = 0, PP_GZETA = 2, PP_FRI_ALPHA = 4, PP_RED0 = 6, PP_RED1 = 8, PP_FRI_BETAS = 10,
                  PP_OWN = PP_FRI_BETAS + 2 * fpl::MAX_LAYERS };

// a run of opened columns that enters the FRI batches
struct FriRun {
    uint32_t w_off;     // word offset of its first column within the query
    uint32_t count;
    uint32_t pow0;      // its first column's power of alpha
    uint32_t batches;   // bit 0: the batch opened at zeta, bit 1: the one at g zeta - the columns are read once for both
};

// What one call holds until its stream work has drained.  Members go in reverse order: the scratch first - which synchronises -,
// then the host sources of the asynchronous copies.
struct VerifyCall {
    std::vector<uint64_t> stage, pp;
    std::vector<uint32_t> qidx;
    Scratch scratch;
    explicit VerifyCall(nlx_ctx* ctx) : scratch(ctx) {}
};

// the device side of one call, as the constraint launch sees it
struct Device {
    const uint64_t *stage, *pp;   // [proof][w_total], [proof][pp_stride]
    const uint64_t* per;          // [proof][periodic column]: the column at zeta, an extension element
    uint64_t* part;               // [proof][part_words], preset to 0xFF
    size_t n_proofs;              // the proofs that reached the device
};

constexpr uint32_t NO_CHALLENGE = 0xFFFFFFFFu;

struct Verifier {
    nlx_ctx* ctx = nullptr;
    const fpl::Layout* lay = nullptr;
    uint32_t log_n = 0, arity_bits = 0, pow_bits = 0, pp_stride = 0;
    // of the proof's Merkle trees: which path kernel runs and how a cap enters the transcript (observe_hash); lay->hasher, which
    // tells the parser which words are digests, is the same value
    uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS;
    size_t w_caps = 0;                     // the first cap the proof carries; one per initial tree follows
    const uint64_t* ext_cap = nullptr;      // device: tree 0's cap where the proof does not carry it
    bool grouped_leaves = false;            // the format has leaf_group_cols, and leaf_group is this verifier's value (0: none)
    uint32_t leaf_group = 0;
    FriRun runs[fpl::MAX_TREES];
    uint32_t n_runs = 0, batch_shift = 0;   // batch_shift: the columns of the batch at g zeta
    const uint64_t* per_coeffs = nullptr;   // device: [column][period] coefficients of the periodic columns' interpolations
    uint32_t n_periodic = 0, period_bits = 0;
    size_t part_words = 0;                  // what the constraint launch leaves per proof
    const char *name_paths = "", *name_fri = "", *part_unwritten = "";
    // the transcript of one proof up to the FRI alpha, with the reduced openings and the verifier's own words of pp
    std::function<void(const uint64_t* w, uint64_t* pp, Challenger& ch)> head;
    std::function<int32_t()> prepare;       // before the first launch of a call, or empty
    std::function<int32_t(const Device&)> constraints;   // the third launch
    // the first challenge whose constraints fail at zeta, or NO_CHALLENGE; part: this proof's words
    std::function<uint32_t(const uint64_t* w, const uint64_t* pp, const uint64_t* part)> judge;
};

// the checks of a batch entry point that come before any work
int32_t check_batch_args(nlx_ctx* ctx, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs, const uint64_t* public_inputs,
                         uint32_t n_pis, const nlx_stark_verdict* verdicts);
// n_proofs >= 1 proofs through the verifier: NLX_OK and a verdict each, or an error and the verdicts zeroed
int32_t verify_batch(Verifier& v, VerifyCall& vc, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                     const uint64_t* public_inputs, nlx_stark_verdict* verdicts);

// draws zeta; pp gets it and g zeta
inline gl::Ext draw_zeta(Challenger& ch, uint64_t* pp, uint32_t log_n) {
    ch.ext_challenge(pp + PP_ZETA);
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
    const gl::Ext gzeta = gl::mul(zeta, gl::root_of_unity(log_n));
    pp[PP_GZETA] = gzeta.a;
    pp[PP_GZETA + 1] = gzeta.b;
    return zeta;
}

// PrecomputedReducedOpenings of one FRI batch: sum_j alpha^j opened[j] over the runs of extension elements, one after the other
struct ExtRun { const uint64_t* o; size_t count; };
inline void reduce_openings(const uint64_t* pp, std::initializer_list<ExtRun> runs, uint64_t* out) {
    const gl::Ext fa{pp[PP_FRI_ALPHA], pp[PP_FRI_ALPHA + 1]};
    gl::Ext ap{1, 0}, r{0, 0};
    for (const ExtRun& run : runs)
        for (size_t j = 0; j < run.count; j++) {
            r = gl::add(r, gl::mul(ap, gl::Ext{run.o[2 * j], run.o[2 * j + 1]}));
            ap = gl::mul(ap, fa);
        }
    out[0] = r.a;
    out[1] = r.b;
}

// zeta^n and Z_H(zeta) = zeta^n - 1 for n = 2^log_n
struct ZetaN {
    gl::Ext zeta_n, z_h;
    ZetaN(gl::Ext zeta, uint32_t log_n) : zeta_n(zeta) {
        for (uint32_t k = 0; k < log_n; k++) zeta_n = gl::mul(zeta_n, zeta_n);
        z_h = gl::sub(zeta_n, gl::Ext{1, 0});
    }
    // does `sum`, the constraints at zeta, equal Z_H(zeta) t(zeta) for the quotient's qdf chunks opened at o_q
    bool divides(gl::Ext sum, const uint64_t* o_q, uint32_t qdf) const {
        gl::Ext t{0, 0};
        for (uint32_t k = qdf; k-- > 0;) t = gl::add(gl::mul(t, zeta_n), gl::Ext{o_q[2 * k], o_q[2 * k + 1]});
        return gl::eq(sum, gl::mul(z_h, t));
    }
};

}  // namespace fv
}  // namespace nlx
