// Host orchestration of a whole plonky2 proof on one MI355X (C ABI: nlx_circuit_build, nlx_prove).
//
// Replaces plonky2::plonk::prover::prove_with_partition_witness (after witness generation),
// plonky2::plonk::circuit_builder::CircuitBuilder::build's constants/sigmas commitment and
// util::serialization's ProofWithPublicInputs::to_bytes, reached
// from nearx/src/test_utils.rs:29 (build) and :62 (prove).
//
// Division of labour: every O(n) stage runs on the GPU with tables
// resident in HBM; the Fiat-Shamir transcript is ~120 strictly sequential Poseidon permutations
// over a few KB and runs on the host, as it does in the reference - only
// Merkle caps (512 B), openings (~4.5 KB), the final polynomial and the query answers cross
// PCIe.  It is not a fallback for any device stage.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "commit.hpp"
#include "gl.hpp"
#include "poly.hpp"
#include "poseidon.hpp"
#include "prover.hpp"
#include "fri.hpp"
#include "transcript.hpp"

using namespace nlx;

namespace {
uint32_t fri_num_rounds(const nlx_circuit_desc& d) {
    return nlx::fri_num_rounds(d.degree_bits, d.rate_bits, d.cap_height, d.fri_arity_bits, d.fri_final_poly_bits);
}

// plonky2 Gate::num_constraints() of every gate kind k_quotient evaluates: the alpha-power table of the quotient stage
// must hold one power per constraint of the widest gate (the circuit's `num_gate_constraints`).
uint32_t gate_num_constraints(const nlx_gate_desc& g) {
    const uint32_t p0 = g.param0, p1 = g.param1;
    switch (g.kind) {
        case NLX_GATE_CONSTANT: case NLX_GATE_ARITHMETIC: return p0;
        case NLX_GATE_PUBLIC_INPUT: return 4;
        case NLX_GATE_BASE_SUM: return 1 + p1;                      // the sum + one range product per limb
        case NLX_GATE_POSEIDON: return 123;                         // 1 swap bit + 4 deltas + 3*12 + 22 + 4*12 + 12 outputs
        case NLX_GATE_ARITHMETIC_EXT: case NLX_GATE_MUL_EXT: case NLX_GATE_REDUCING: case NLX_GATE_REDUCING_EXT:
            return 2 * p0;                                          // D = 2 base constraints per extension constraint
        case NLX_GATE_POSEIDON_MDS: return 24;
        case NLX_GATE_EXPONENTIATION: return p0 + 1;
        case NLX_GATE_RANDOM_ACCESS: return (p1 & 0xFFFF) * (p0 + 2) + (p1 >> 16);
        case NLX_GATE_COSET_INTERPOLATION: return 2 * (2 + 2 * (((1u << p0) - 2) / (p1 - 1)));
        case NLX_GATE_U32_ADD_MANY: return p1 * (3 + 18);
        case NLX_GATE_U32_ARITHMETIC: return p0 * (4 + 32);
        case NLX_GATE_U32_SUBTRACTION: return p0 * (3 + 16);
        case NLX_GATE_U32_RANGE_CHECK: return p0 * 17;
        case NLX_GATE_COMPARISON: return 6 + 5 * p1 + (p0 + p1 - 1) / p1;
        default: return 0;
    }
}

// Cost of one gate's evaluation at one point, in microseconds of k_quotient's time per 2^19 points when every wave of a
// tile evaluates that item alone, less the 234 us an empty item list takes (measured on MI355X with the calibration build,
// tools/quotient_calibrate.sh, standard parameters - round 3's kernel: profiles/r03_quotient_calibrate.txt; scaled linearly in
// the parameter that multiplies the work).  Only the RATIOS matter: they balance the work split.
uint32_t gate_eval_cost(const nlx_gate_desc& g) {
    const uint32_t p0 = g.param0, p1 = g.param1;
    switch (g.kind) {
        case NLX_GATE_ARITHMETIC: return 10 + 6 * p0;                      // 130 for 20 operations
        case NLX_GATE_BASE_SUM: return 10 + 95 * p1 * (1 + p0) / 30;      // 610 for 63 limbs in base 2
        case NLX_GATE_POSEIDON: return 2540;                                // evaluated in three parts, see POSEIDON_PARTS
        case NLX_GATE_ARITHMETIC_EXT: return 10 + 16 * p0;                 // 170
        case NLX_GATE_MUL_EXT: return 10 + 13 * p0;                        // 180
        case NLX_GATE_REDUCING: return 10 + 165 * p0 / 10;                 // 720
        case NLX_GATE_REDUCING_EXT: return 10 + 160 * p0 / 10;             // 520
        case NLX_GATE_POSEIDON_MDS: return 120;
        case NLX_GATE_EXPONENTIATION: return 10 + 80 * p0 / 10;            // 540
        case NLX_GATE_RANDOM_ACCESS: return 10 + 128 * (p1 & 0xFFFF) * (1u << p0) / 16;   // 520
        case NLX_GATE_COSET_INTERPOLATION: return 10 + (34u << p0);        // 550
        case NLX_GATE_U32_ADD_MANY: return 10 + 136 * p1;                  // 690
        case NLX_GATE_U32_ARITHMETIC: return 10 + 250 * p0;                // 760
        case NLX_GATE_U32_SUBTRACTION: return 10 + 132 * p0;               // 800
        case NLX_GATE_U32_RANGE_CHECK: return 10 + 109 * p0;               // 770
        case NLX_GATE_COMPARISON: return 10 + 27 * p1;                     // 440
        default: return 10;
    }
}
// PoseidonGate's three parts (prover_kernels.hip gate_poseidon): part mask, share of the gate's cost in percent
constexpr uint32_t POSEIDON_PARTS[3][2] = {{1, 17}, {2, 59}, {4, 24}};   // measured 440 / 1 490 / 610
// Part 2 (the 22 partial rounds) runs in a kernel of its own before k_quotient (launch_quotient_poseidon: the permutation's
// fused-block schedule, prover_kernels.hip) unless NLX_QUOTIENT_POSEIDON_INLINE=1 keeps it among k_quotient's items.
bool poseidon_part2_separate_default() {
    const char* e = getenv("NLX_QUOTIENT_POSEIDON_INLINE");
    return !(e && e[0] == '1');
}
}  // namespace

struct nlx_circuit {
    nlx_ctx* ctx = nullptr;
    nlx_circuit_desc d{};
    std::vector<nlx_gate_desc> gates;
    std::vector<uint64_t> k_is;
    uint32_t n_consts_all = 0, n_cs = 0, n_zs = 0, n_q = 0, n_fri_rounds = 0, n_terms = 0, max_gate_constraints = 0;
    CommitPtr cs;                       // constants + sigmas commitment
    uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS;   // the config's Hasher: every Merkle tree of the proof, and how digests enter the transcript
    uint32_t* d_bad = nullptr;          // BN128: the leaf kernels' range word (never set: oracles of <= 4 columns are refused at build)
    std::vector<uint64_t> cs_cap;       // host copy
    uint64_t* d_sigma_values = nullptr; // [routed][n]
    GateDev* d_gates = nullptr;
    uint32_t* d_work = nullptr;         // k_quotient's work split: [quotient_waves()][work_stride]
    bool poseidon_part2_separate = poseidon_part2_separate_default();
    std::vector<uint32_t> poseidon_gates;   // PoseidonGates whose part 2 runs in k_quotient_poseidon
    uint32_t work_stride = 0;
    uint64_t* d_small = nullptr;        // k_is | coset_base | zh_inv | w_R_inv_pows | chunk_scale | w_A_inv_pows
    uint64_t *d_k_is = nullptr, *d_coset_base = nullptr, *d_zh_inv = nullptr, *d_wR_inv = nullptr,
             *d_chunk_scale = nullptr, *d_wA_inv = nullptr;
    uint64_t* d_l0_scaled = nullptr;
    const uint64_t* d_inv_scale_br = nullptr;  // ctx-owned
    // lookup tables (all empty / zero without them)
    uint32_t n_zpp = 0;        // Zs + partial products columns; n_zs = n_zpp + n_lk_polys
    uint32_t n_lk_sel = 0;     // lookup selector columns (4 + tables), between the gate selectors and the gate constants
    uint32_t n_lk_polys = 0;   // num_challenges * (1 + S)
    uint32_t n_lk_terms = 0;   // 4 + tables + 2 S vanishing terms per challenge round
    LookupShape lk{};
    std::vector<uint32_t> lut_sizes, lut_offsets, lookup_rows, lut_num_lookups;
    std::vector<uint16_t> lut_pairs;
    std::vector<LookupTableDev> h_tabs;
    LookupTableDev* d_tabs = nullptr;
    uint32_t* d_lut_pairs = nullptr;  // all tables, input | output << 16
    int32_t* d_idx_of = nullptr;      // [tables][65536]
    uint32_t* d_mult = nullptr;       // multiplicity counters of all tables, then the error word
    size_t mult_words = 0;
    // the witness checker's (nlx_circuit_check_witness): made by the first check that needs them, null in a circuit never checked
    uint64_t* d_consts_h = nullptr;     // [n_consts_all][n]: the constants' values on H (build keeps coefficients and LDE only)
    uint32_t* d_sigma_row = nullptr;    // [routed][n]: sigma(x) decoded to its row ...
    uint16_t* d_sigma_col = nullptr;    // ... and column
    CheckBlock* d_check = nullptr;      // the passes' counters and minima
    StageClock clock;
    size_t n() const { return (size_t)1 << d.degree_bits; }
    size_t L() const { return (size_t)1 << (d.degree_bits + d.rate_bits); }
};

namespace nlx {
nlx_ctx* circuit_ctx(const nlx_circuit* c) { return c->ctx; }
const nlx_circuit_desc& circuit_desc(const nlx_circuit* c) { return c->d; }
}  // namespace nlx

namespace {
// every commitment of a circuit's proofs carries the circuit's hasher
int32_t commit_for(nlx_circuit* c, const uint64_t* d_in, CommitInput kind, uint32_t n_cols, CommitPtr& out) {
    return commit_build(c->ctx, d_in, c->n(), kind, n_cols, c->d.degree_bits, c->d.rate_bits, c->d.cap_height, out, 0, 0, c->hasher, c->d_bad);
}

// The descriptor checks every consumer of a circuit shares: nlx_circuit_build and the verifier built from a verifying key alone
// (plonk_verify.hip).  The message is left in ctx.
}  // namespace
int32_t nlx::validate_circuit_desc(nlx_ctx* ctx, const nlx_circuit_desc& d, uint32_t hasher) {
    if (d.num_challenges < 1 || d.num_challenges > 2) return ctx->fail(NLX_E_UNSUPPORTED, "num_challenges must be 1 or 2");
    if (d.rate_bits < 1 || d.rate_bits > 3) return ctx->fail(NLX_E_UNSUPPORTED, "rate_bits must be in [1, 3]");
    if ((1u << d.rate_bits) != d.quotient_degree_factor)
        return ctx->fail(NLX_E_UNSUPPORTED, "quotient_degree_factor must equal 2^rate_bits");
    if (d.fri_arity_bits < 2 || d.fri_arity_bits > 4) return ctx->fail(NLX_E_UNSUPPORTED, "fri_arity_bits must be in [2, 4]");
    if (d.degree_bits < d.fri_arity_bits || d.degree_bits + d.rate_bits > 30) return ctx->fail(NLX_E_RANGE, "degree_bits out of range");
    if (d.num_routed_wires > d.num_wires || d.num_routed_wires == 0) return ctx->fail(NLX_E_INVAL, "bad wire counts");
    if (hasher != NLX_HASHER_POSEIDON_GOLDILOCKS && hasher != NLX_HASHER_POSEIDON_BN128) return ctx->fail(NLX_E_RANGE, "unknown hasher %u", hasher);
    if (hasher == NLX_HASHER_POSEIDON_BN128) {
        if (d.num_luts) return ctx->fail(NLX_E_UNSUPPORTED, "circuits with lookup tables are not proved under the PoseidonBN128 config");
        // hash_or_noop: a row of <= 4 elements is its own digest and has none when it packs to a value >= r, which a random LDE
        // row does - such an oracle cannot be committed
        const uint32_t zs_cols = d.num_challenges * (1 + d.num_partial_products);
        if (d.num_challenges * d.quotient_degree_factor <= 4 || zs_cols <= 4 || d.num_wires <= 4 ||
            d.num_selectors + d.num_constants + d.num_routed_wires <= 4)
            return ctx->fail(NLX_E_UNSUPPORTED, "PoseidonBN128 config: every oracle needs more than 4 columns (num_challenges * quotient_degree_factor = %u)",
                             d.num_challenges * d.quotient_degree_factor);
    }
    const uint32_t n_chunks = (d.num_routed_wires + d.quotient_degree_factor - 1) / d.quotient_degree_factor;
    if (n_chunks > 10 || n_chunks != d.num_partial_products + 1) return ctx->fail(NLX_E_INVAL, "num_partial_products mismatch");
    if (d.fri_num_queries > 128 || d.cap_height > 6) return ctx->fail(NLX_E_RANGE, "FRI parameters out of range");
    for (uint32_t g = 0; g < d.num_gates; g++) {
        const nlx_gate_desc& gt = d.gates[g];
        if (gt.kind > NLX_GATE_KIND_MAX) return ctx->fail(NLX_E_UNSUPPORTED, "gate kind %u not supported", gt.kind);
        if (gt.kind == NLX_GATE_ARITHMETIC_EXT && (8 * gt.param0 > d.num_wires || d.num_constants < 2)) return ctx->fail(NLX_E_INVAL, "ArithmeticExtensionGate too wide");
        if (gt.kind == NLX_GATE_MUL_EXT && 6 * gt.param0 > d.num_wires) return ctx->fail(NLX_E_INVAL, "MulExtensionGate too wide");
        if (gt.kind == NLX_GATE_REDUCING && (gt.param0 < 1 || 6 + gt.param0 + 2 * (gt.param0 - 1) > d.num_wires)) return ctx->fail(NLX_E_INVAL, "ReducingGate too wide");
        if (gt.kind == NLX_GATE_POSEIDON_MDS && d.num_wires < 48) return ctx->fail(NLX_E_INVAL, "PoseidonMdsGate needs 48 wires");
        if (gt.kind == NLX_GATE_EXPONENTIATION && (gt.param0 < 1 || 2 + 2 * gt.param0 > d.num_wires)) return ctx->fail(NLX_E_INVAL, "ExponentiationGate too wide");
        if (gt.kind == NLX_GATE_U32_ADD_MANY && (gt.param0 < 1 || gt.param0 > 15 || gt.param1 < 1 || (gt.param0 + 3 + 18) * gt.param1 > d.num_wires))
            return ctx->fail(NLX_E_INVAL, "U32AddManyGate does not fit the wires");
        if (gt.kind == NLX_GATE_U32_ARITHMETIC && (gt.param0 < 1 || (6 + 32) * gt.param0 > d.num_wires)) return ctx->fail(NLX_E_INVAL, "U32ArithmeticGate too wide");
        if (gt.kind == NLX_GATE_U32_SUBTRACTION && (gt.param0 < 1 || (5 + 16) * gt.param0 > d.num_wires)) return ctx->fail(NLX_E_INVAL, "U32SubtractionGate too wide");
        if (gt.kind == NLX_GATE_U32_RANGE_CHECK && (gt.param0 < 1 || 17 * gt.param0 > d.num_wires)) return ctx->fail(NLX_E_INVAL, "U32RangeCheckGate too wide");
        if (gt.kind == NLX_GATE_COMPARISON) {
            const uint32_t cb = gt.param1 ? (gt.param0 + gt.param1 - 1) / gt.param1 : 0;
            if (gt.param1 < 1 || cb < 1 || cb > 3 || cb * gt.param1 > 62 || 4 + 5 * gt.param1 + cb + 1 > d.num_wires)
                return ctx->fail(NLX_E_INVAL, "ComparisonGate: chunk_bits must be in [1, 3] and the gate must fit the wires");
        }
        if (gt.kind == NLX_GATE_COSET_INTERPOLATION) {
            const uint32_t np = gt.param0 <= 5 ? 1u << gt.param0 : 0;
            if (np < 4 || gt.param1 < 2 || gt.param1 > np || d.degree_bits < gt.param0 + 1 ||
                1 + 2 * np + 4 + 4 * ((np - 2) / (gt.param1 - 1)) + 2 > d.num_wires)
                return ctx->fail(NLX_E_INVAL, "CosetInterpolationGate does not fit");
        }
        if (gt.kind == NLX_GATE_RANDOM_ACCESS) {
            const uint32_t bits = gt.param0, copies = gt.param1 & 0xFFFF, extra = gt.param1 >> 16;
            if (bits < 1 || bits > 6 || copies < 1 || extra > d.num_constants ||
                (2 + (1u << bits)) * copies + extra + copies * bits > d.num_wires)
                return ctx->fail(NLX_E_INVAL, "RandomAccessGate does not fit the wires");
        }
        if (gt.kind == NLX_GATE_REDUCING_EXT && (gt.param0 < 1 || 6 + 2 * gt.param0 + 2 * (gt.param0 - 1) > d.num_wires)) return ctx->fail(NLX_E_INVAL, "ReducingExtensionGate too wide");
        if (gt.selector_index >= d.num_selectors || gt.group_end > d.num_gates || gt.group_start > gt.group_end)
            return ctx->fail(NLX_E_INVAL, "gate %u: bad selector group", g);
        if (gt.kind == NLX_GATE_POSEIDON && d.num_wires < 135) return ctx->fail(NLX_E_INVAL, "PoseidonGate needs 135 wires");
        if (gt.kind == NLX_GATE_ARITHMETIC && 4 * gt.param0 > d.num_wires) return ctx->fail(NLX_E_INVAL, "ArithmeticGate too wide");
        if (gt.kind == NLX_GATE_BASE_SUM && 1 + gt.param1 > d.num_wires) return ctx->fail(NLX_E_INVAL, "BaseSumGate too wide");
        if (gt.kind == NLX_GATE_CONSTANT && gt.param0 > d.num_constants) return ctx->fail(NLX_E_INVAL, "ConstantGate too wide");
    }
    if (d.num_luts) {
        // CommonCircuitData::luts + ProverOnlyCircuitData::lookup_rows: shapes as CircuitBuilder::add_all_lookups lays them out
        if (d.num_luts > 16) return ctx->fail(NLX_E_RANGE, "at most 16 lookup tables");
        if (!d.lut_sizes || !d.lut_pairs || !d.lookup_rows || !d.lut_num_lookups) return ctx->fail(NLX_E_INVAL, "NULL lookup table array");
        const uint32_t n_lu = d.num_routed_wires / 2, n_lut = d.num_routed_wires / 3;
        if (n_lut < 1 || d.quotient_degree_factor < 2) return ctx->fail(NLX_E_INVAL, "too few routed wires for the lookup gates");
        for (uint32_t t = 0; t < d.num_luts; t++) {
            const uint32_t len = d.lut_sizes[t], lookups = d.lut_num_lookups[t];
            const uint32_t last_lu = d.lookup_rows[3 * t], last_lut = d.lookup_rows[3 * t + 1], first_lut = d.lookup_rows[3 * t + 2];
            if (len < 1 || len > 65536 || lookups < 1) return ctx->fail(NLX_E_RANGE, "table %u: 1 .. 65536 entries and at least one lookup", t);
            if (!(last_lu < last_lut && last_lut <= first_lut) || (uint64_t)first_lut + 1 >= ((uint64_t)1 << d.degree_bits))
                return ctx->fail(NLX_E_INVAL, "table %u: lookup rows out of order or past the circuit", t);
            if (last_lut - last_lu != (lookups + n_lu - 1) / n_lu || first_lut - last_lut + 1 != (len + n_lut - 1) / n_lut)
                return ctx->fail(NLX_E_INVAL, "table %u: row counts do not match its lookups / entries", t);
        }
    }
    return NLX_OK;
}
namespace {
int32_t circuit_build(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants, const uint64_t* sigmas,
                      uint32_t hasher, nlx_circuit** out) {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !constants || !sigmas || !out || !desc->gates || !desc->k_is)
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    const nlx_circuit_desc& d = *desc;
    NLX_RC(validate_circuit_desc(ctx, d, hasher));
    (void)hipSetDevice(ctx->device);
    nlx_circuit* c = new (std::nothrow) nlx_circuit();
    if (!c) return ctx->fail(NLX_E_NOMEM, "host allocation failed");
    c->ctx = ctx;
    c->d = d;
    c->hasher = hasher;
    c->gates.assign(d.gates, d.gates + d.num_gates);
    for (const nlx_gate_desc& gt : c->gates) c->max_gate_constraints = std::max(c->max_gate_constraints, gate_num_constraints(gt));
#ifdef NLX_GATEACC_LIMBS3
    // the three-limb accumulator has no carry counters: a gate folds once, so its constraints must fit the columns' headroom
    if (c->max_gate_constraints > GATEACC3_MAX_TERMS || d.num_partial_products + 1 > GATEACC3_MAX_TERMS) {
        delete c;
        return ctx->fail(NLX_E_INVAL, "a gate with more than %u constraints (this build accumulates them without carry counters)", GATEACC3_MAX_TERMS);
    }
#endif
    c->k_is.assign(d.k_is, d.k_is + d.num_routed_wires);
    c->d.gates = c->gates.data();
    c->d.k_is = c->k_is.data();
    if (d.num_luts) {
        const uint32_t T = d.num_luts;
        c->lk.num_luts = T;
        c->lk.n_lu_slots = d.num_routed_wires / 2;
        c->lk.n_lut_slots = d.num_routed_wires / 3;
        c->lk.lu_degree = d.quotient_degree_factor - 1;
        c->lk.n_sldc = (c->lk.n_lu_slots + c->lk.lu_degree - 1) / c->lk.lu_degree;
        c->lk.lut_degree = (c->lk.n_lut_slots + c->lk.n_sldc - 1) / c->lk.n_sldc;
        c->n_lk_sel = 4 + T;
        c->n_lk_polys = d.num_challenges * (1 + c->lk.n_sldc);
        c->n_lk_terms = 4 + T + 2 * c->lk.n_sldc;
        c->lut_sizes.assign(d.lut_sizes, d.lut_sizes + T);
        c->lut_num_lookups.assign(d.lut_num_lookups, d.lut_num_lookups + T);
        c->lookup_rows.assign(d.lookup_rows, d.lookup_rows + 3 * T);
        c->lut_offsets.assign(T + 1, 0);
        for (uint32_t t = 0; t < T; t++) c->lut_offsets[t + 1] = c->lut_offsets[t] + c->lut_sizes[t];
        c->lut_pairs.assign(d.lut_pairs, d.lut_pairs + 2 * (size_t)c->lut_offsets[T]);
        c->d.lut_sizes = c->lut_sizes.data(); c->d.lut_num_lookups = c->lut_num_lookups.data();
        c->d.lookup_rows = c->lookup_rows.data(); c->d.lut_pairs = c->lut_pairs.data();
    }
    c->n_consts_all = d.num_selectors + c->n_lk_sel + d.num_constants;
    c->n_cs = c->n_consts_all + d.num_routed_wires;
    c->n_zpp = d.num_challenges * (1 + d.num_partial_products);
    c->n_zs = c->n_zpp + c->n_lk_polys;
    c->n_q = d.num_challenges * d.quotient_degree_factor;
    c->n_fri_rounds = fri_num_rounds(d);
    const size_t n = c->n(), L = c->L();
    const unsigned log_n = d.degree_bits, log_L = d.degree_bits + d.rate_bits;
    const uint32_t R = 1u << d.rate_bits, A = 1u << d.fri_arity_bits;
    int32_t rc = ctx->ensure_tables(log_L);
    auto fail = [&](int32_t code) {
        nlx_circuit_destroy(c);
        return code;
    };
    if (rc) return fail(rc);
    rc = ctx->get_coset_scale(log_n, d.rate_bits, &c->d_inv_scale_br, true);
    if (rc) return fail(rc);
    if (hasher == NLX_HASHER_POSEIDON_BN128) {
        c->d_bad = (uint32_t*)ctx->alloc(256);
        if (!c->d_bad) return fail(NLX_E_NOMEM);
        if (hipMemsetAsync(c->d_bad, 0, 4, ctx->stream) != hipSuccess) return fail(ctx->fail(NLX_E_HIP, "hipMemsetAsync failed"));
    }

    // constants ++ sigmas -> one device matrix -> commitment
    {
        uint64_t* d_vals = (uint64_t*)ctx->alloc((size_t)c->n_cs * n * 8);
        if (!d_vals) return fail(NLX_E_NOMEM);
        const size_t cb = (size_t)c->n_consts_all * n * 8, sb = (size_t)d.num_routed_wires * n * 8;
        hipError_t e1 = hipMemcpyAsync(d_vals, constants, cb, is_device_ptr(constants) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        hipError_t e2 = hipMemcpyAsync((uint8_t*)d_vals + cb, sigmas, sb, is_device_ptr(sigmas) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        if (e1 != hipSuccess || e2 != hipSuccess) { ctx->release(d_vals); return fail(ctx->hip_fail(e1 != hipSuccess ? e1 : e2, "hipMemcpyAsync")); }
        rc = commit_for(c, d_vals, CommitInput::ValuesNatural, c->n_cs, c->cs);
        if (rc) { ctx->release(d_vals); return fail(rc); }
        c->d_sigma_values = (uint64_t*)ctx->alloc(sb);
        if (!c->d_sigma_values) { ctx->release(d_vals); return fail(NLX_E_NOMEM); }
        (void)hipMemcpyAsync(c->d_sigma_values, (uint8_t*)d_vals + cb, sb, hipMemcpyDeviceToDevice, ctx->stream);
        ctx->release(d_vals);
    }
    // small tables
    {
        const uint32_t routed = d.num_routed_wires;
        std::vector<uint64_t> small(routed + 3 * R + R + A);
        uint64_t* h_k = small.data();
        uint64_t* h_cb = h_k + routed;
        uint64_t* h_zh = h_cb + R;
        uint64_t* h_wR = h_zh + R;
        uint64_t* h_cs = h_wR + R;
        uint64_t* h_wA = h_cs + R;
        memcpy(h_k, c->k_is.data(), routed * 8);
        const uint64_t w_L = gl::root_of_unity(log_L), w_R = gl::root_of_unity(d.rate_bits);
        const uint64_t g_n = gl::exp_pow2(gl::GEN, log_n);
        const uint64_t g_n_inv = gl::inv(g_n), R_inv = gl::inv((uint64_t)R);
        for (uint32_t r = 0; r < R; r++) {
            h_cb[r] = gl::mul(gl::GEN, gl::pow(w_L, r));
            h_zh[r] = gl::inv(gl::sub(gl::mul(g_n, gl::pow(w_R, r)), 1));  // 1 / (x^n - 1) on coset r
            h_wR[r] = gl::pow(gl::inv(w_R), r);
            h_cs[r] = gl::mul(gl::pow(g_n_inv, r), R_inv);
        }
        const uint64_t w_A_inv = gl::inv(gl::root_of_unity(d.fri_arity_bits));
        for (uint32_t i = 0; i < A; i++) h_wA[i] = gl::pow(w_A_inv, i);
        c->d_small = (uint64_t*)ctx->alloc(small.size() * 8);
        c->d_gates = (GateDev*)ctx->alloc(sizeof(GateDev) * (d.num_gates ? d.num_gates : 1));
        c->d_l0_scaled = (uint64_t*)ctx->alloc(L * 8);
        if (!c->d_small || !c->d_gates || !c->d_l0_scaled) return fail(NLX_E_NOMEM);
        static_assert(sizeof(GateDev) == sizeof(nlx_gate_desc), "gate descriptor layout");
        hipError_t e = hipMemcpy(c->d_small, small.data(), small.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && d.num_gates) e = hipMemcpy(c->d_gates, c->gates.data(), sizeof(GateDev) * d.num_gates, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(ctx->hip_fail(e, "hipMemcpy(tables)"));
        c->d_k_is = c->d_small;
        c->d_coset_base = c->d_k_is + routed;
        c->d_zh_inv = c->d_coset_base + R;
        c->d_wR_inv = c->d_zh_inv + R;
        c->d_chunk_scale = c->d_wR_inv + R;
        c->d_wA_inv = c->d_chunk_scale + R;
        launch_l0_table(ctx->stream, c->d_l0_scaled, log_n, d.rate_bits, c->d_coset_base, ctx->tables.fwd[log_n]);
    }
    if (d.num_luts) {
        // the tables on the device: packed pairs, the input -> index map of set_lookup_wires (HashMap collect: the last entry
        // with an input wins), multiplicity counters
        const uint32_t T = d.num_luts, total = c->lut_offsets[T];
        std::vector<uint32_t> packed(total);
        std::vector<int32_t> idx_of((size_t)T << 16, -1);
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t i = 0; i < c->lut_sizes[t]; i++) {
                const uint16_t* pr = &c->lut_pairs[2 * (size_t)(c->lut_offsets[t] + i)];
                packed[c->lut_offsets[t] + i] = (uint32_t)pr[0] | ((uint32_t)pr[1] << 16);
                idx_of[((size_t)t << 16) + pr[0]] = (int32_t)i;
            }
        c->mult_words = total;
        c->d_lut_pairs = (uint32_t*)ctx->alloc((size_t)total * 4);
        c->d_idx_of = (int32_t*)ctx->alloc(idx_of.size() * 4);
        c->d_mult = (uint32_t*)ctx->alloc(((size_t)total + 1) * 4);
        c->d_tabs = (LookupTableDev*)ctx->alloc(sizeof(LookupTableDev) * T);
        if (!c->d_lut_pairs || !c->d_idx_of || !c->d_mult || !c->d_tabs) return fail(NLX_E_NOMEM);
        c->h_tabs.resize(T);
        for (uint32_t t = 0; t < T; t++) {
            LookupTableDev& lt = c->h_tabs[t];
            lt.len = c->lut_sizes[t]; lt.lookups = c->lut_num_lookups[t];
            lt.last_lu = c->lookup_rows[3 * t]; lt.last_lut = c->lookup_rows[3 * t + 1]; lt.first_lut = c->lookup_rows[3 * t + 2];
            lt.pad_ = 0;
            lt.pairs = c->d_lut_pairs + c->lut_offsets[t];
            lt.idx_of = c->d_idx_of + ((size_t)t << 16);
            lt.mult = c->d_mult + c->lut_offsets[t];
        }
        hipError_t e = hipMemcpy(c->d_lut_pairs, packed.data(), packed.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(c->d_idx_of, idx_of.data(), idx_of.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(c->d_tabs, c->h_tabs.data(), sizeof(LookupTableDev) * T, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(ctx->hip_fail(e, "hipMemcpy(lookup tables)"));
    }
    {
        // k_quotient's work split: items = every gate + the permutation argument of each challenge; longest item first into
        // the least loaded wave.  Wave w and wave w + QW/2 of a block share a SIMD, so the bins are then paired heavy with
        // light: what has to balance is the load per SIMD (the same split runs on every tile).
        const uint32_t QWv = quotient_waves();
        if (d.num_gates + d.num_challenges > 0xFFFFu) return fail(ctx->fail(NLX_E_RANGE, "too many gates"));
        std::vector<std::pair<uint32_t, uint32_t>> items;  // (cost, id)
        uint32_t n_words = 0;
        for (uint32_t g = 0; g < d.num_gates; g++) {
            const uint32_t cost = gate_eval_cost(c->gates[g]);
            if (c->gates[g].kind == NLX_GATE_POSEIDON) {
                for (const auto& part : POSEIDON_PARTS) {
                    if (part[0] == 2 && c->poseidon_part2_separate) {
                        c->poseidon_gates.push_back(g);
                        continue;
                    }
                    items.push_back({cost * part[1] / 100, g | (part[0] << 16)});
                }
            } else {
                items.push_back({cost, g});
            }
        }
        for (uint32_t ch = 0; ch < d.num_challenges; ch++) items.push_back({10 + 45 * d.num_routed_wires / 4, d.num_gates + ch});  // 910 for 80 routed wires
        n_words = (uint32_t)items.size();
        std::sort(items.begin(), items.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        std::vector<std::vector<uint32_t>> bins(QWv);
        std::vector<uint64_t> load(QWv, 0);
        for (const auto& it : items) {
            const uint32_t b = (uint32_t)(std::min_element(load.begin(), load.end()) - load.begin());
            bins[b].push_back(it.second);
            load[b] += it.first;
        }
        std::vector<uint32_t> order(QWv);
        for (uint32_t i = 0; i < QWv; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return load[a] != load[b] ? load[a] > load[b] : a < b; });
        c->work_stride = n_words + 1;
        std::vector<uint32_t> work((size_t)QWv * c->work_stride, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < QWv; i++) {
            // heaviest bins on waves 0 .. QW/2-1, lightest first on waves QW/2 .. QW-1: SIMD s gets bins order[s] and order[QW-1-s]
            const uint32_t wave = i < QWv / 2 ? i : QWv / 2 + (QWv - 1 - i);
            std::copy(bins[order[i]].begin(), bins[order[i]].end(), work.begin() + (size_t)wave * c->work_stride);
        }
#ifdef NLX_QUOTIENT_CALIBRATE
        // kernel-tuning build only (build.py, NLX_BUILD_VARIANT): every wave evaluates the ONE item named by NLX_Q_ONLY, so
        // that the stage time ranks the items' real costs (tools/quotient_calibrate.sh); the proof is wrong by design
        if (const char* only = getenv("NLX_Q_ONLY")) {
            std::fill(work.begin(), work.end(), 0xFFFFFFFFu);
            for (uint32_t w = 0; w < QWv; w++) work[(size_t)w * c->work_stride] = (uint32_t)atoi(only);
        }
#endif
        c->d_work = (uint32_t*)ctx->alloc(work.size() * 4);
        if (!c->d_work) return fail(NLX_E_NOMEM);
        hipError_t e = hipMemcpy(c->d_work, work.data(), work.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(ctx->hip_fail(e, "hipMemcpy(work split)"));
        if (quotient_lds_bytes(d.num_wires, c->n_consts_all) > 160 * 1024)
            return fail(ctx->fail(NLX_E_UNSUPPORTED, "num_wires %u: the quotient kernel's wire tile does not fit the 160 KB of LDS", d.num_wires));
    }
    c->cs_cap.resize((size_t)4 << d.cap_height);
    rc = fetch(ctx, c->cs_cap.data(), c->cs->cap, c->cs_cap.size() * 8);
    if (rc) return fail(rc);
    bool zero = true;
    for (int i = 0; i < 4; i++) zero = zero && d.circuit_digest[i] == 0;
    if (zero && hasher == NLX_HASHER_POSEIDON_BN128) {
        // the same under Hasher = PoseidonBN128Hash (tools/bn128_config_model.py rule 4, recalled): the cap flattened to five
        // limbs per digest, the domain separator's BN128 digest as five limbs, degree_bits; a BN128 digest, four words
        const size_t n_cap = c->cs_cap.size() / 4;
        std::vector<uint64_t> parts(n_cap * BN128_DIGEST_LIMBS);
        for (size_t i = 0; i < n_cap; i++) bn128_digest_limbs(&c->cs_cap[4 * i], &parts[i * BN128_DIGEST_LIMBS]);
        uint64_t pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, dom[4], dl[BN128_DIGEST_LIMBS];
        bn128_hash_no_pad_host(pad, 12, dom);
        bn128_digest_limbs(dom, dl);
        parts.insert(parts.end(), dl, dl + BN128_DIGEST_LIMBS);
        parts.push_back(d.degree_bits);
        bn128_hash_no_pad_host(parts.data(), parts.size(), c->d.circuit_digest);
    } else if (zero) {
        // circuit_digest = hash_no_pad(cap || hash_pad([]) || degree_bits)   (CircuitBuilder::build)
        std::vector<uint64_t> parts(c->cs_cap);
        uint64_t pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, dom[4];
        hash_no_pad_host(pad, 12, dom);
        parts.insert(parts.end(), dom, dom + 4);
        parts.push_back(d.degree_bits);
        hash_no_pad_host(parts.data(), parts.size(), c->d.circuit_digest);
    }
    rc = c->clock.create(ctx);
    if (rc) return fail(rc);
    *out = c;
    return NLX_OK;
}
}  // namespace

extern "C" {

int32_t nlx_circuit_build(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants,
                          const uint64_t* sigmas, nlx_circuit** out) NLX_TRY {
    return circuit_build(ctx, desc, constants, sigmas, NLX_HASHER_POSEIDON_GOLDILOCKS, out);
} NLX_CATCH(ctx)

int32_t nlx_circuit_build_hasher(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants, const uint64_t* sigmas,
                                 uint32_t hasher, nlx_circuit** out) NLX_TRY {
    return circuit_build(ctx, desc, constants, sigmas, hasher, out);
} NLX_CATCH(ctx)

int32_t nlx_circuit_hasher(const nlx_circuit* c) NLX_TRY {
    if (!c) return NLX_E_INVAL;
    return (int32_t)c->hasher;
} NLX_CATCH(nullptr)

void nlx_circuit_destroy(nlx_circuit* c) NLX_TRY {
    if (!c) return;
    nlx_ctx* ctx = c->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->release(c->d_sigma_values);
    ctx->release(c->d_gates);
    ctx->release(c->d_work);
    ctx->release(c->d_small);
    ctx->release(c->d_l0_scaled);
    ctx->release(c->d_lut_pairs);
    ctx->release(c->d_idx_of);
    ctx->release(c->d_mult);
    ctx->release(c->d_tabs);
    ctx->release(c->d_bad);
    ctx->release(c->d_consts_h);
    ctx->release(c->d_sigma_row);
    ctx->release(c->d_sigma_col);
    ctx->release(c->d_check);
    delete c;   // and with it the constants + sigmas commitment and the stage clock's events
} NLX_CATCH_VOID(nullptr)

int32_t nlx_circuit_digest(const nlx_circuit* c, uint64_t out[4]) NLX_TRY {
    if (!c || !out) return NLX_E_INVAL;
    memcpy(out, c->d.circuit_digest, 32);
    return NLX_OK;
} NLX_CATCH(nullptr)

int32_t nlx_circuit_constants_sigmas_cap(const nlx_circuit* c, uint64_t* cap_out) NLX_TRY {
    if (!c || !cap_out) return NLX_E_INVAL;
    memcpy(cap_out, c->cs_cap.data(), c->cs_cap.size() * 8);
    return NLX_OK;
} NLX_CATCH(nullptr)

size_t nlx_proof_max_bytes(const nlx_circuit* c) NLX_TRY {
    if (!c) return 0;
    const nlx_circuit_desc& d = c->d;
    const size_t capb = (size_t)32 << d.cap_height;
    const unsigned log_L = d.degree_bits + d.rate_bits;
    size_t bytes = 3 * capb + 16 * (size_t)(c->n_cs + d.num_wires + c->n_zs + d.num_challenges + c->n_lk_polys + c->n_q) + c->n_fri_rounds * capb;
    size_t per_query = 0;
    const uint32_t cols[4] = {c->n_cs, d.num_wires, c->n_zs, c->n_q};
    for (int o = 0; o < 4; o++) per_query += cols[o] * 8 + 1 + 32 * (size_t)(log_L - d.cap_height);
    per_query += c->n_fri_rounds * ((size_t)16 << d.fri_arity_bits) + c->n_fri_rounds * (1 + 32 * (size_t)log_L);
    bytes += per_query * d.fri_num_queries;
    bytes += ((size_t)16 << (d.degree_bits - c->n_fri_rounds * d.fri_arity_bits)) + 8 + 8 + 8 * (size_t)d.num_public_inputs;
    return bytes + 64;
} NLX_CATCH_VALUE(nullptr, 0)

int32_t nlx_pow_grind(nlx_ctx* ctx, const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t* nonce_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!state || !nonce_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (pos >= 8 || bits > 40) return ctx->fail(NLX_E_RANGE, "pos must be < 8 and bits <= 40");
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    unsigned long long* d_best = scratch.alloc_as<unsigned long long>(256);
    if (!d_best) return NLX_E_NOMEM;
    PowParams pp{};
    for (int i = 0; i < 12; i++) pp.state[i] = state[i];
    pp.pos = pos;
    pp.bits = bits;
    pp.max_rounds = (uint64_t)1 << 24;
    launch_pow_grind(ctx->stream, pp, d_best);
    uint64_t best = 0;
    NLX_RC(fetch(ctx, &best, d_best, 8, &scratch));
    if (best == ~0ull) return ctx->fail(NLX_E_RANGE, "proof of work: no witness found");
    *nonce_out = best;
    return NLX_OK;
} NLX_CATCH(ctx)

int32_t nlx_prove_stage_times(const nlx_circuit* c, uint32_t* n_stages, const char** names_out, float* ms_out) NLX_TRY {
    return c ? c->clock.times(n_stages, names_out, ms_out) : NLX_E_INVAL;
} NLX_CATCH(nullptr)

}  // extern "C"

namespace {

// a8: Z and partial-product polynomials from the wires' subgroup values (device), committed.
// Everything is only enqueued; the temporaries come from the caller's `scratch` and go back when the caller drains it.
// With lookup tables the same commitment carries, after them, every challenge round's RE and partial-sum polynomials
// (compute_all_lookup_polys); d_deltas = the rounds' (A, B, alpha, delta) on the device.
int32_t zs_stage(nlx_circuit* c, const uint64_t* d_wire_values, const uint64_t betas[2], const uint64_t gammas[2],
                 const uint64_t* d_deltas, CommitPtr& cz, Scratch& scratch) {
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    const unsigned log_n = d.degree_bits;
    const size_t n = c->n();
    uint64_t* d_zs = scratch.alloc_as<uint64_t>((size_t)c->n_zs * n * 8);
    uint64_t* d_zs_scratch = scratch.alloc_as<uint64_t>(zs_scratch_words(log_n, d.num_challenges) * 8);
    if (!d_zs || !d_zs_scratch) return NLX_E_NOMEM;
    ZsParams zp{};
    zp.wires = d_wire_values;
    zp.wires_stride = n;
    zp.sigmas = c->d_sigma_values;
    zp.k_is = c->d_k_is;
    zp.w_n_table = ctx->tables.fwd[log_n];
    for (int i = 0; i < 2; i++) { zp.betas[i] = betas[i]; zp.gammas[i] = gammas[i]; }
    zp.out = d_zs;
    zp.log_n = log_n; zp.routed = d.num_routed_wires; zp.chunk = d.quotient_degree_factor; zp.nc = d.num_challenges;
    zp.npp = d.num_partial_products;
    launch_zs(ctx->stream, zp, d_zs_scratch);
    if (c->n_lk_polys)
        launch_lookup_polys(ctx->stream, c->lk, c->d_tabs, c->h_tabs.data(), d_wire_values, n, d.num_challenges, d_deltas,
                            d_zs + (size_t)c->n_zpp * n);
    return commit_for(c, d_zs, CommitInput::ValuesNatural, c->n_zs, cz);
}

// The quotient degree check (BN128 circuits; the Goldilocks entries keep returning a proof, as they always have).
// plonky2's `trim_to_len(quotient_degree)` is vacuous here, the quotient being interpolated on exactly quotient_degree = R n points
// (R = quotient_degree_factor = 2^rate_bits).  But the quotient has slack at the top: every constraint has degree at most
// (R + 1)(n - 1) - a higher one would alias on the R n points and no proof of the circuit would verify - so for a satisfied
// witness t = V / Z_H has degree at most R n - (R + 1) and its top R coefficients are zero.  If V = Z_H t0 + r with r != 0
// (deg r < n), the values V / Z_H on the coset interpolate to t0 + r (1 + x^n + ... + x^((R-1) n)) / (g^(R n) - 1) exactly
// (1 / (y - 1) = (1 + y + ... + y^(R-1)) / (G - 1) modulo y^R - G), so the top R coefficients of the last chunk are those of
// r / (G - 1): the remainder's x^(n-R) .. x^(n-1).  A row where V != 0 contributes V(x0) (x0 / n) (x^n - 1) / (x - x0) to r, every
// coefficient of which is non-zero, and V is a random combination (alphas, drawn after the witness is committed) of the
// constraints: an unsatisfied witness leaves these R coefficients zero only if sum_x x^j C_k(x) = 0 for every constraint k and
// every j = 1 .. R, or with probability ~R / p over alpha.  This is a check against wrong witnesses, not a verifier: the full
// identity is the verifier's check at zeta.
// Coefficient i of chunk c sits at [challenge R + c][bitrev(i)]; i = n - R + k is position rev(k) n / R + n / R - 1.
int32_t quotient_degree_check(nlx_circuit* c, const uint64_t* d_qchunks) {
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    const size_t n = c->n();
    const uint32_t R = 1u << d.rate_bits, nc = d.num_challenges;
    if (n < 2 * (size_t)R) return NLX_OK;   // the bound above needs the top R coefficients inside the last chunk's upper half
    uint64_t top[2 * 8];
    const size_t stride = n / R;
    int32_t rc = ensure_pinned(ctx, 1u << 20);
    if (rc) return rc;
    for (uint32_t ch = 0; ch < nc; ch++) {
        const uint64_t* src = d_qchunks + ((size_t)ch * R + (R - 1)) * n + (stride - 1);
        NLX_HIP(ctx, hipMemcpy2DAsync((uint64_t*)ctx->pinned + (size_t)ch * R, 8, src, stride * 8, 8, R, hipMemcpyDeviceToHost, ctx->stream));
    }
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(top, ctx->pinned, (size_t)nc * R * 8);
    for (uint32_t i = 0; i < nc * R; i++)
        if (gl::canon(top[i]) != 0)
            return ctx->fail(NLX_E_INVAL, "the witness does not satisfy the circuit: the quotient of challenge %u has degree above %u n - %u (the vanishing polynomial is not divisible by Z_H)",
                             i / R, R, R + 1);
    return NLX_OK;
}

// a9: quotient polynomials (compute_quotient_polys) from the three LDE tables, committed from coefficients.
int32_t quotient_stage(nlx_circuit* c, const nlx_commit* cw, const nlx_commit* cz, const uint64_t betas[2],
                       const uint64_t gammas[2], const uint64_t alphas[2], const uint64_t pih[4],
                       const uint64_t* d_deltas, const uint64_t* d_lut_polys, CommitPtr& cq, StageClock& clock, Scratch& scratch) {
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    hipStream_t st = ctx->stream;
    const unsigned log_n = d.degree_bits;
    const size_t L = c->L();
    const uint32_t nc = d.num_challenges, npp = d.num_partial_products;
    // one alpha power per vanishing term (GateAcc reads ap[T0 + k]): Z(1) terms, permutation terms, lookup terms, gate constraints
    c->n_terms = nc + nc * (npp + 1) + nc * c->n_lk_terms + c->max_gate_constraints;
    uint64_t* d_alpha_pows = scratch.alloc_as<uint64_t>((size_t)2 * c->n_terms * 8);
    uint64_t* d_qvals = scratch.alloc_as<uint64_t>((size_t)nc * L * 8);
    uint64_t* d_qchunks = scratch.alloc_as<uint64_t>((size_t)nc * L * 8);
    if (!d_alpha_pows || !d_qvals || !d_qchunks) return NLX_E_NOMEM;
    launch_pow_table(st, d_alpha_pows, alphas[0], alphas[1], c->n_terms, c->n_terms);
    QuotientParams qp{};
#ifdef NLX_GATEACC_LIMBS3
    uint32_t* d_alpha_limbs = scratch.alloc_as<uint32_t>((size_t)2 * c->n_terms * 16);
    if (!d_alpha_limbs) return NLX_E_NOMEM;
    launch_pow_limbs(st, d_alpha_limbs, d_alpha_pows, 2 * c->n_terms);
    qp.alpha_limbs = d_alpha_limbs;
#endif
    qp.cs = c->cs->lde; qp.wires = cw->lde; qp.zs = cz->lde;
    qp.gates = c->d_gates; qp.k_is = c->d_k_is; qp.coset_base = c->d_coset_base;
    qp.w_n_table = ctx->tables.fwd[log_n];
    qp.zh_inv = c->d_zh_inv; qp.l0_scaled = c->d_l0_scaled; qp.alpha_pows = d_alpha_pows;
    qp.out = d_qvals;
    for (int i = 0; i < 2; i++) { qp.betas[i] = betas[i]; qp.gammas[i] = gammas[i]; }
    for (int i = 0; i < 4; i++) qp.pih[i] = pih[i];
    qp.alpha_stride = c->n_terms;
    qp.num_wires = d.num_wires; qp.work = c->d_work; qp.work_stride = c->work_stride;
    qp.log_n = log_n; qp.rate_bits = d.rate_bits; qp.n_gates = d.num_gates; qp.n_selectors = d.num_selectors;
    qp.n_consts_all = c->n_consts_all; qp.routed = d.num_routed_wires; qp.chunk = d.quotient_degree_factor; qp.nc = nc; qp.npp = npp;
    qp.gate_const0 = d.num_selectors + c->n_lk_sel;
    qp.n_lk_terms = c->n_lk_terms;
    if (c->n_lk_terms) {
        // check_lookup_constraints_batch: the lookup terms' share of both alpha sums goes into d_qvals first, k_quotient adds it
        LookupTermsParams lp{};
        lp.cs = c->cs->lde; lp.wires = cw->lde; lp.zs = cz->lde;
        lp.deltas = d_deltas; lp.lut_polys = d_lut_polys; lp.alpha_pows = d_alpha_pows; lp.out = d_qvals;
        lp.alpha_stride = c->n_terms; lp.t_lk = nc + nc * (npp + 1);
        lp.log_n = log_n; lp.rate_bits = d.rate_bits; lp.nc = nc; lp.sel0 = d.num_selectors; lp.lk0 = c->n_zpp;
        lp.n_lk_terms = c->n_lk_terms; lp.s = c->lk;
        ctx->begin_kernel("lookup_terms", 8.0 * L * (c->n_lk_sel + d.num_routed_wires + 2.0 * c->n_lk_polys + nc));
        launch_lookup_terms(st, lp);
        ctx->end_kernel();
        qp.accumulate = 1;
    }
    ctx->begin_kernel("quotient", 8.0 * L * (c->n_cs + d.num_wires + c->n_zs + nc) + 8.0 * L * nc);
    for (uint32_t g : c->poseidon_gates) {   // their part 2 ahead of the main kernel, which adds the rest
        launch_quotient_poseidon(st, qp, g, qp.accumulate != 0);
        qp.accumulate = 1;
    }
    launch_quotient(st, qp);
    ctx->end_kernel();
    clock.stage("quotient_intt");
    launch_intt_dif_cosets(st, ctx->tables, d_qvals, nc, log_n, d.rate_bits, c->d_inv_scale_br);
    launch_quotient_chunks(st, d_qvals, d_qchunks, log_n, d.rate_bits, nc, c->d_wR_inv, c->d_chunk_scale);
    clock.stage("commit_quotient");
    NLX_RC(commit_for(c, d_qchunks, CommitInput::CoeffsBitrev, c->n_q, cq));
    // a refused stage hands no commitment out: its owner gives it back, after the caller's scratch has drained the stream
    return c->hasher == NLX_HASHER_POSEIDON_BN128 ? quotient_degree_check(c, d_qchunks) : NLX_OK;
}

// What one nlx_prove call holds until its stream work has drained.  Members go in reverse order: the scratch first - which
// synchronises -, then the host sources of the asynchronous copies, then the commitments.
struct ProveCall {
    CommitPtr cw, cz, cq;
    uint64_t deltas[8] = {}, lut_polys[2 * 16] = {};
    OpeningPoints points;
    Scratch scratch;
    explicit ProveCall(nlx_ctx* ctx) : scratch(ctx) {}
};

int32_t prove_stages(nlx_circuit* c, ProveCall& pc, const uint64_t* wires, const uint64_t* public_inputs, Writer& w, size_t* proof_len) {
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    hipStream_t st = ctx->stream;
    const size_t n = c->n();
    const unsigned log_n = d.degree_bits, cap_h = d.cap_height;
    const uint32_t nc = d.num_challenges, npp = d.num_partial_products;
    const uint32_t NR = c->n_fri_rounds;
    const size_t capw = (size_t)4 << cap_h;
    Scratch& scratch = pc.scratch;
    CommitPtr &cw = pc.cw, &cz = pc.cz, &cq = pc.cq;
    Challenger ch;
    std::vector<uint64_t> cap(capw);
    uint64_t pih[4];
    std::vector<uint64_t> h_pis(public_inputs, public_inputs + d.num_public_inputs);
    hash_no_pad_host(h_pis.data(), h_pis.size(), pih);

    c->clock.begin(st);
    c->clock.stage("commit_wires");
    // ---- 2. wires commitment ----
    Staged sw(ctx, wires, (size_t)d.num_wires * n * 8, true, false);
    NLX_RC(sw.status);
    // prover::set_lookup_wires, the first thing prove_with_partition_witness does to the witness it is handed: multiplicity
    // wires and padding slots, on the device copy (a device witness is written in place, as upstream's PartitionWitness is)
    if (d.num_luts)
        launch_set_lookup_wires(st, c->lk, c->d_tabs, c->h_tabs.data(), sw.as<uint64_t>(), n, c->d_mult, c->mult_words,
                                c->d_mult + c->mult_words);
    NLX_RC(commit_for(c, sw.as<uint64_t>(), CommitInput::ValuesNatural, d.num_wires, cw));
    NLX_RC(fetch(ctx, cap.data(), cw->cap, capw * 8));
    if (d.num_luts) {
        uint32_t bad = 0;
        NLX_RC(fetch(ctx, &bad, c->d_mult + c->mult_words, 4));
        if (bad) return ctx->fail(NLX_E_INVAL, "a looked-up input is not in its table (set_lookup_wires)");
    }
    w.u64s(cap.data(), capw);
    NLX_RC(observe_hash(c->hasher, ch, d.circuit_digest, 1));
    ch.observe(pih, 4);   // InnerHasher: Goldilocks Poseidon under both configs
    NLX_RC(observe_hash(c->hasher, ch, cap.data(), capw / 4));
    uint64_t betas[2] = {0, 0}, gammas[2] = {0, 0}, alphas[2] = {0, 0};
    for (uint32_t i = 0; i < nc; i++) betas[i] = ch.challenge();
    for (uint32_t i = 0; i < nc; i++) gammas[i] = ch.challenge();
    // lookup challenges: deltas = betas ++ gammas ++ 2 nc more, NUM_COINS_LOOKUP = 4 per round (A, B, alpha, delta)
    // deltas and lut_polys are the SOURCES of asynchronous host-to-device copies: they live in the call's state, past its drain
    uint64_t* const deltas = pc.deltas;
    uint64_t* const lut_polys = pc.lut_polys;
    uint64_t* d_deltas = nullptr;   // deltas[4 nc] | lut_polys[nc tables]
    if (d.num_luts) {
        for (uint32_t i = 0; i < nc; i++) { deltas[i] = betas[i]; deltas[nc + i] = gammas[i]; }
        for (uint32_t i = 0; i < 2 * nc; i++) deltas[2 * nc + i] = ch.challenge();
        d_deltas = scratch.alloc_as<uint64_t>((size_t)(8 + 2 * 16) * 8);
        if (!d_deltas) return NLX_E_NOMEM;
        NLX_HIP(ctx, hipMemcpyAsync(d_deltas, deltas, sizeof pc.deltas, hipMemcpyHostToDevice, st));
    }

    // ---- 4. partial products and Z ----
    c->clock.stage("zs_partial_products");
    NLX_RC(zs_stage(c, sw.as<uint64_t>(), betas, gammas, d_deltas, cz, scratch));
    if (d.num_luts) {
        // vanishing_poly::get_lut_poly per (round, table), on the host while the device builds the Zs commitment: the pairs
        // (inp + B out) as coefficients in delta, first entry highest, zero-padded to whole table rows
        for (uint32_t ci = 0; ci < nc; ci++)
            for (uint32_t t = 0; t < d.num_luts; t++) {
                const uint32_t len = c->lut_sizes[t], slots = c->lk.n_lut_slots;
                const uint32_t degree = slots * ((len + slots - 1) / slots);
                const uint16_t* pr = &c->lut_pairs[2 * (size_t)c->lut_offsets[t]];
                const uint64_t B = deltas[4 * ci + 1], dl = deltas[4 * ci + 3];
                uint64_t acc = 0;
                for (uint32_t i = 0; i < len; i++) acc = gl::add(gl::mul(acc, dl), gl::add((uint64_t)pr[2 * i], gl::mul(B, (uint64_t)pr[2 * i + 1])));
                acc = gl::mul(acc, gl::pow(dl, degree - len));
                lut_polys[ci * d.num_luts + t] = acc;
            }
        NLX_HIP(ctx, hipMemcpyAsync(d_deltas + 8, lut_polys, sizeof(uint64_t) * nc * d.num_luts, hipMemcpyHostToDevice, st));
    }
    NLX_RC(fetch(ctx, cap.data(), cz->cap, capw * 8));
    w.u64s(cap.data(), capw);
    NLX_RC(observe_hash(c->hasher, ch, cap.data(), capw / 4));
    for (uint32_t i = 0; i < nc; i++) alphas[i] = ch.challenge();

    // ---- 5. quotient ----
    c->clock.stage("quotient_eval");
    NLX_RC(quotient_stage(c, cw.get(), cz.get(), betas, gammas, alphas, pih, d_deltas, d_deltas ? d_deltas + 8 : nullptr, cq, c->clock, scratch));
    NLX_RC(fetch(ctx, cap.data(), cq->cap, capw * 8));
    w.u64s(cap.data(), capw);
    NLX_RC(observe_hash(c->hasher, ch, cap.data(), capw / 4));

    // ---- 6. openings ----
    c->clock.stage("openings");
    uint64_t zeta[2], gzeta[2];
    ch.ext_challenge(zeta);
    {
        const uint64_t g = gl::root_of_unity(log_n);
        gzeta[0] = gl::mul(zeta[0], g);
        gzeta[1] = gl::mul(zeta[1], g);
    }
    const nlx_commit* oracles[4] = {c->cs.get(), cw.get(), cz.get(), cq.get()};
    const uint32_t n_open = c->n_cs + d.num_wires + c->n_zs + c->n_q;
    const OpeningPoints& pts = pc.points;
    NLX_RC(pc.points.upload(scratch, zeta, gzeta, log_n));
    const uint32_t nlk = c->n_lk_polys, n_next = nc + nlk;
    uint64_t* d_open = scratch.alloc_as<uint64_t>((size_t)(n_open + n_next) * 16);
    uint64_t* d_eval_scratch = scratch.alloc_as<uint64_t>(eval_scratch_words(d.num_wires > c->n_cs ? d.num_wires : c->n_cs, log_n) * 8);
    if (!d_open || !d_eval_scratch) return NLX_E_NOMEM;
    {
        uint32_t off = 0;
        for (int o = 0; o < 4; o++) {
            launch_eval_br(st, oracles[o]->coeffs_br, n, oracles[o]->n_cols, log_n, pts.zeta(), d_open + 2 * (size_t)off,
                           d_eval_scratch, pts.zeta_pows());
            off += oracles[o]->n_cols;
        }
        launch_eval_br(st, cz->coeffs_br, n, nc, log_n, pts.gzeta(), d_open + 2 * (size_t)n_open, d_eval_scratch,
                       pts.gzeta_pows());
        if (nlk)  // lookup_zs_next: the lookup polynomials (columns n_zpp.. of the Zs commitment) at g zeta
            launch_eval_br(st, cz->coeffs_br + (size_t)c->n_zpp * n, n, nlk, log_n, pts.gzeta(),
                           d_open + 2 * (size_t)(n_open + nc), d_eval_scratch, pts.gzeta_pows());
        NLX_HIP(ctx, hipStreamSynchronize(st));
    }
    std::vector<uint64_t> open((size_t)(n_open + n_next) * 2);
    NLX_RC(fetch(ctx, open.data(), d_open, open.size() * 8));
    if (nlk) {
        // CommonCircuitData::fri_all_polys lists the lookup polynomials LAST in the zeta batch (after the quotient chunks):
        // move their openings from the middle (commitment order) to the end, then everything below reads FRI order
        uint64_t* zs0 = open.data() + 2 * (size_t)(c->n_cs + d.num_wires);
        std::vector<uint64_t> lkv(zs0 + 2 * (size_t)c->n_zpp, zs0 + 2 * (size_t)c->n_zs);
        memmove(zs0 + 2 * (size_t)c->n_zpp, zs0 + 2 * (size_t)c->n_zs, 2 * (size_t)c->n_q * 8);
        memcpy(zs0 + 2 * (size_t)(c->n_zpp + c->n_q), lkv.data(), lkv.size() * 8);
    }
    {
        // OpeningSet wire order: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys
        const uint64_t* o_cs = open.data();
        const uint64_t* o_w = o_cs + 2 * (size_t)c->n_cs;
        const uint64_t* o_zs = o_w + 2 * (size_t)d.num_wires;
        const uint64_t* o_pp = o_zs + 2 * (size_t)nc;
        const uint64_t* o_q = o_zs + 2 * (size_t)c->n_zpp;
        const uint64_t* o_lk = o_q + 2 * (size_t)c->n_q;
        const uint64_t* o_next = open.data() + 2 * (size_t)n_open;
        w.u64s(o_cs, 2 * (size_t)c->n_cs);
        w.u64s(o_w, 2 * (size_t)d.num_wires);
        w.u64s(o_zs, 2 * (size_t)nc);
        w.u64s(o_next, 2 * (size_t)nc);
        w.u64s(o_lk, 2 * (size_t)nlk);                    // lookup_zs, lookup_zs_next (read_opening_set order)
        w.u64s(o_next + 2 * (size_t)nc, 2 * (size_t)nlk);
        w.u64s(o_pp, 2 * (size_t)nc * npp);
        w.u64s(o_q, 2 * (size_t)c->n_q);
        ch.observe(open.data(), 2 * (size_t)n_open);
        ch.observe(o_next, 2 * (size_t)n_next);
    }

    // ---- 7. FRI ----
    {
        FriProveArgs fa;
        for (int o = 0; o < 4; o++) fa.oracles[o] = oracles[o];
        fa.n_oracles = 4;
        fa.nz[2] = nc;  // plonk_zs_next: the first nc columns of the Zs / partial-products oracle
        fa.tail_oracle = 2;  // the lookup polynomials: its last nlk columns, a group of their own at the end of both batches
        fa.tail_cols = nlk;
        for (int i = 0; i < 2; i++) { fa.zeta[i] = zeta[i]; fa.gzeta[i] = gzeta[i]; }
        fa.open0 = open.data();
        fa.open1 = open.data() + 2 * (size_t)n_open;
        fa.log_n = log_n; fa.rate_bits = d.rate_bits; fa.cap_height = cap_h; fa.arity_bits = d.fri_arity_bits;
        fa.pow_bits = d.fri_pow_bits; fa.n_queries = d.fri_num_queries; fa.n_rounds = NR;
        fa.d_coset_base = c->d_coset_base;
        fa.d_wA_inv = c->d_wA_inv;
        fa.hasher = c->hasher;
        NLX_RC(fri_prove(ctx, fa, ch, w, scratch, c->clock));
    }
    w.usize(d.num_public_inputs);  // write_proof_with_public_inputs: write_usize(len), then the field vec
    w.u64s(h_pis.data(), h_pis.size());
    c->clock.end();
    if (w.overflow) return ctx->fail(NLX_E_RANGE, "proof buffer too small (need %zu bytes)", nlx_proof_max_bytes(c));
    *proof_len = w.len;
    return NLX_OK;
}

}  // namespace

extern "C" {

int32_t nlx_prove(nlx_circuit* c, const uint64_t* wires, const uint64_t* public_inputs, uint8_t* proof_out,
                  size_t proof_cap, size_t* proof_len) NLX_TRY {
    if (!c) return NLX_E_INVAL;
    nlx_ctx* ctx = c->ctx;
    if (!wires || !proof_out || !proof_len || (!public_inputs && c->d.num_public_inputs))
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    *proof_len = 0;
    (void)hipSetDevice(ctx->device);
    Writer w{proof_out, 0, proof_cap};
    ProveCall pc(ctx);
    return pc.scratch.finish(prove_stages(c, pc, wires, public_inputs, w, proof_len));
} NLX_CATCH(nullptr)

int32_t nlx_batch_prove(nlx_circuit* const* workers, uint32_t n_workers, nlx_prove_job* jobs, size_t n_jobs) NLX_TRY {
    return batch_prove("nlx_batch_prove", workers, n_workers, jobs, n_jobs, [](nlx_circuit* c, nlx_prove_job& job) {
        return nlx_prove(c, job.wires, job.public_inputs, job.proof_out, job.proof_cap, &job.proof_len);
    });
} NLX_CATCH(nullptr)

// ---- the witness checker ----
}  // extern "C"

namespace {
// plonky2's type names, by NLX_GATE_*
const char* const GATE_NAMES[NLX_GATE_KIND_MAX + 1] = {
    "NoopGate", "ConstantGate", "PublicInputGate", "ArithmeticGate", "BaseSumGate", "PoseidonGate", "ArithmeticExtensionGate",
    "MulExtensionGate", "ReducingGate", "ReducingExtensionGate", "PoseidonMdsGate", "ExponentiationGate", "RandomAccessGate",
    "CosetInterpolationGate", "U32AddManyGate", "U32ArithmeticGate", "U32SubtractionGate", "U32RangeCheckGate", "ComparisonGate",
    "LookupGate", "LookupTableGate"};

// the sigma values as cells, once per circuit: kept only when every cell decoded
int32_t ensure_sigma_cells(nlx_circuit* c, Scratch& scratch) {
    if (c->d_sigma_row) return NLX_OK;
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    const size_t n = c->n(), cells = (size_t)d.num_routed_wires * n;
    const uint32_t routed = d.num_routed_wires;
    std::vector<uint64_t> h(2 * (size_t)routed);   // k_i^n | 1 / k_i
    for (uint32_t i = 0; i < routed; i++) {
        h[i] = gl::exp_pow2(c->k_is[i], d.degree_bits);
        h[routed + i] = gl::inv(c->k_is[i]);
    }
    uint64_t* d_h = scratch.alloc_as<uint64_t>(h.size() * 8);
    uint32_t* d_row = (uint32_t*)ctx->alloc(cells * 4);
    uint16_t* d_col = (uint16_t*)ctx->alloc(cells * 2);
    auto give_back = [&](int32_t rc) {
        ctx->release(d_row);
        ctx->release(d_col);
        return rc;
    };
    if (!d_h || !d_row || !d_col) return give_back(ctx->fail(NLX_E_NOMEM, "out of device memory (sigma cells)"));
    hipError_t e = hipMemcpy(d_h, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return give_back(ctx->hip_fail(e, "hipMemcpy(coset tables)"));
    launch_sigma_decode(ctx->stream, c->d_sigma_values, c->d_k_is, d_h, d_h + routed, ctx->tables.fwd[d.degree_bits],
                        ctx->tables.inv[d.degree_bits], d.degree_bits, routed, d_row, d_col, c->d_check);
    CheckBlock b;
    int32_t rc = fetch(ctx, &b, c->d_check, sizeof b);
    if (rc) return give_back(rc);
    if (b.sigma_undecodable != CHECK_NONE)
        return give_back(ctx->fail(NLX_E_INVAL, "sigma value at row %llu, column %llu lies in no coset k_i H of the descriptor's k_is",
                                   b.sigma_undecodable % n, b.sigma_undecodable / n));
    c->d_sigma_row = d_row;
    c->d_sigma_col = d_col;
    return NLX_OK;
}

int32_t check_witness(nlx_circuit* c, const uint64_t* wires, const uint64_t* public_inputs, uint32_t what, nlx_witness_report* rep,
                      Scratch& scratch) {
    nlx_ctx* ctx = c->ctx;
    const nlx_circuit_desc& d = c->d;
    hipStream_t st = ctx->stream;
    const size_t n = c->n();
    if (!d.num_luts) what &= ~NLX_CHECK_LOOKUPS;
    rep->checked = what;
    rep->satisfied = 1;
    if (!what) return NLX_OK;
    Staged sw(ctx, wires, (size_t)d.num_wires * n * 8, true, false);
    NLX_RC(sw.status);
    const uint64_t* d_w = sw.as<uint64_t>();
    if (!c->d_check) {
        c->d_check = (CheckBlock*)ctx->alloc(256);
        if (!c->d_check) return ctx->fail(NLX_E_NOMEM, "out of device memory (check block)");
    }
    launch_check_reset(st, c->d_check);
    CheckGatesParams gp{};
    if (what & NLX_CHECK_GATES) {
        if (!c->d_consts_h) {
            // the constants on H: one forward transform of the commitment's coefficients, no coset scale (the LDE lives on g H)
            uint64_t* t = (uint64_t*)ctx->alloc((size_t)c->n_consts_all * n * 8);
            if (!t) return ctx->fail(NLX_E_NOMEM, "out of device memory (constants on H)");
            launch_lde_dit(st, ctx->tables, c->cs->coeffs_br, n, t, n, c->n_consts_all, d.degree_bits, 0, nullptr);
            c->d_consts_h = t;
        }
        std::vector<uint64_t> h_pis(public_inputs, public_inputs + d.num_public_inputs);
        hash_no_pad_host(h_pis.data(), h_pis.size(), gp.q.pih);
        gp.q.gates = c->d_gates;
        gp.q.w_n_table = ctx->tables.fwd[d.degree_bits];
        gp.q.log_n = d.degree_bits; gp.q.rate_bits = d.rate_bits; gp.q.n_gates = d.num_gates; gp.q.n_selectors = d.num_selectors;
        gp.q.n_consts_all = c->n_consts_all; gp.q.num_wires = d.num_wires;
        gp.q.gate_const0 = d.num_selectors + c->n_lk_sel;
        gp.consts = c->d_consts_h;
        gp.wires = d_w;
        gp.block = c->d_check;
        launch_check_gates(st, gp, 0xFFFFFFFFu);
    }
    if (what & NLX_CHECK_COPIES) {
        NLX_RC(ensure_sigma_cells(c, scratch));
        launch_check_copies(st, d_w, d.degree_bits, d.num_routed_wires, c->d_sigma_row, c->d_sigma_col, c->d_check);
    }
    if (what & NLX_CHECK_LOOKUPS) launch_check_lookups(st, c->lk, c->d_tabs, c->h_tabs.data(), d_w, n, c->d_check);
    CheckBlock b;
    NLX_RC(fetch(ctx, &b, c->d_check, sizeof b));
    rep->gate_rows_bad = b.gate_rows_bad;
    rep->copy_cells_bad = b.copy_cells_bad;
    rep->lookup_slots_bad = b.lookup_slots_bad;
    rep->satisfied = !(b.gate_rows_bad || b.copy_cells_bad || b.lookup_slots_bad);
    if (rep->satisfied) return NLX_OK;
    // the details of each first finding: a handful of words from the device, on the failing path only
    auto word = [&](const uint64_t* src, uint64_t* dst) { return fetch(ctx, dst, src, 8); };
    char line[3][160] = {"", "", ""};
    if (b.gate_rows_bad) {
        rep->gate_row = (uint32_t)(b.gate_first >> 32);
        launch_check_gates(st, gp, rep->gate_row);
        NLX_RC(fetch(ctx, &b, c->d_check, sizeof b));
        rep->gate_index = b.gate_index;
        rep->gate_kind = c->gates[b.gate_index].kind;
        rep->gate_constraint = b.gate_constraint;
        rep->gate_value = b.gate_value;
        snprintf(line[0], sizeof line[0], "row %u (%s, gate %u): constraint %u = %llu, %llu row(s) with a non-zero constraint", rep->gate_row,
                 GATE_NAMES[rep->gate_kind], rep->gate_index, rep->gate_constraint, (unsigned long long)rep->gate_value,
                 (unsigned long long)rep->gate_rows_bad);
    }
    if (b.copy_cells_bad) {
        rep->copy_row = (uint32_t)(b.copy_first >> 32);
        rep->copy_col = (uint32_t)b.copy_first;
        const size_t idx = (size_t)rep->copy_col * n + rep->copy_row;
        uint16_t tc = 0;
        NLX_RC(fetch(ctx, &rep->copy_to_row, c->d_sigma_row + idx, 4));
        NLX_RC(fetch(ctx, &tc, c->d_sigma_col + idx, 2));
        rep->copy_to_col = tc;
        NLX_RC(word(d_w + idx, &rep->copy_value));
        NLX_RC(word(d_w + (size_t)tc * n + rep->copy_to_row, &rep->copy_to_value));
        snprintf(line[1], sizeof line[1], "copy: wire %u of row %u = %llu but sigma sends it to wire %u of row %u = %llu, %llu cell(s) differ from their copy",
                 rep->copy_col, rep->copy_row, (unsigned long long)rep->copy_value, rep->copy_to_col, rep->copy_to_row,
                 (unsigned long long)rep->copy_to_value, (unsigned long long)rep->copy_cells_bad);
    }
    if (b.lookup_slots_bad) {
        rep->lookup_row = (uint32_t)(b.lookup_first >> 32);
        rep->lookup_slot = (uint32_t)b.lookup_first;
        bool table_row = false;
        for (uint32_t t = 0; t < d.num_luts; t++)
            if (rep->lookup_row >= c->h_tabs[t].last_lu && rep->lookup_row <= c->h_tabs[t].first_lut) {
                rep->lookup_table = t;
                table_row = rep->lookup_row >= c->h_tabs[t].last_lut;
            }
        const uint32_t w0 = (table_row ? 3 : 2) * rep->lookup_slot;
        NLX_RC(word(d_w + (size_t)w0 * n + rep->lookup_row, &rep->lookup_input));
        NLX_RC(word(d_w + (size_t)(w0 + 1) * n + rep->lookup_row, &rep->lookup_output));
        snprintf(line[2], sizeof line[2], "lookup: row %u (%s) slot %u holds (%llu, %llu), not a pair of table %u%s, %llu slot(s) wrong", rep->lookup_row,
                 GATE_NAMES[table_row ? NLX_GATE_LOOKUP_TABLE : NLX_GATE_LOOKUP], rep->lookup_slot, (unsigned long long)rep->lookup_input,
                 (unsigned long long)rep->lookup_output, rep->lookup_table, table_row ? " at that entry" : "",
                 (unsigned long long)rep->lookup_slots_bad);
    }
    std::string msg = "the witness does not satisfy the circuit: ";
    bool any = false;
    for (const auto& l : line)
        if (l[0]) {
            if (any) msg += "; ";
            msg += l;
            any = true;
        }
    ctx->err = msg;
    return NLX_OK;
}
}  // namespace

extern "C" {

int32_t nlx_circuit_check_witness(nlx_circuit* c, const uint64_t* wires, const uint64_t* public_inputs, uint32_t what,
                                  nlx_witness_report* report) NLX_TRY {
    if (!c) return NLX_E_INVAL;
    nlx_ctx* ctx = c->ctx;
    if (report) memset(report, 0, sizeof *report);
    if (!wires || !report || (!public_inputs && c->d.num_public_inputs)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (what < 1 || what > NLX_CHECK_ALL) return ctx->fail(NLX_E_INVAL, "what = %u: a non-empty set of NLX_CHECK_* bits (1 .. 7)", what);
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    return scratch.finish(check_witness(c, wires, public_inputs, what, report, scratch));
} NLX_CATCH(c ? c->ctx : nullptr)

// ---- stage-level entry points (the fine seam of INTEGRATION.md §3) ----

const nlx_commit* nlx_circuit_constants_sigmas(const nlx_circuit* c) NLX_TRY { return c ? c->cs.get() : nullptr; } NLX_CATCH_VALUE(nullptr, nullptr)

int32_t nlx_partial_products_and_zs(nlx_circuit* c, const uint64_t* wires, const uint64_t betas[2], const uint64_t gammas[2],
                                    nlx_commit** zs_out) NLX_TRY {
    if (!c) return NLX_E_INVAL;
    nlx_ctx* ctx = c->ctx;
    if (!wires || !betas || !gammas || !zs_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *zs_out = nullptr;
    (void)hipSetDevice(ctx->device);
    if (c->d.num_luts) return ctx->fail(NLX_E_UNSUPPORTED, "circuits with lookup tables are proved through nlx_prove (the stage calls carry no lookup challenges)");
    Staged sw(ctx, wires, (size_t)c->d.num_wires * c->n() * 8, true, false);
    if (sw.status) return sw.status;
    CommitPtr cz;
    Scratch scratch(ctx);
    NLX_RC(scratch.finish(zs_stage(c, sw.as<uint64_t>(), betas, gammas, nullptr, cz, scratch)));
    *zs_out = cz.release();
    return NLX_OK;
} NLX_CATCH(nullptr)

int32_t nlx_quotient_eval(nlx_circuit* c, const nlx_commit* wires, const nlx_commit* zs, const uint64_t betas[2],
                          const uint64_t gammas[2], const uint64_t alphas[2], const uint64_t public_inputs_hash[4],
                          nlx_commit** quotient_out) NLX_TRY {
    if (!c) return NLX_E_INVAL;
    nlx_ctx* ctx = c->ctx;
    if (!wires || !zs || !betas || !gammas || !alphas || !public_inputs_hash || !quotient_out)
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    *quotient_out = nullptr;
    const nlx_circuit_desc& d = c->d;
    if (d.num_luts) return ctx->fail(NLX_E_UNSUPPORTED, "circuits with lookup tables are proved through nlx_prove (the stage calls carry no lookup challenges)");
    if (wires->ctx != ctx || zs->ctx != ctx) return ctx->fail(NLX_E_INVAL, "commitments belong to another context");
    if (wires->hasher != c->hasher || zs->hasher != c->hasher)
        return ctx->fail(NLX_E_UNSUPPORTED, c->hasher == NLX_HASHER_POSEIDON_GOLDILOCKS ? "a PoseidonBN128 commitment cannot enter the Goldilocks transcript"
                                                                                        : "a Goldilocks commitment cannot enter a PoseidonBN128 circuit's proof");
    if (wires->n_cols != d.num_wires || zs->n_cols != c->n_zs || wires->log_n != d.degree_bits || zs->log_n != d.degree_bits ||
        wires->rate_bits != d.rate_bits || zs->rate_bits != d.rate_bits)
        return ctx->fail(NLX_E_INVAL, "commitment shapes do not match the circuit");
    for (int i = 0; i < 4; i++)
        if (public_inputs_hash[i] >= gl::P) return ctx->fail(NLX_E_RANGE, "public inputs hash is not canonical");
    (void)hipSetDevice(ctx->device);
    StageClock untimed;
    CommitPtr cq;
    Scratch scratch(ctx);
    NLX_RC(scratch.finish(quotient_stage(c, wires, zs, betas, gammas, alphas, public_inputs_hash, nullptr, nullptr, cq, untimed, scratch)));
    *quotient_out = cq.release();
    return NLX_OK;
} NLX_CATCH(nullptr)

}  // extern "C"

namespace {
int32_t fri_prove_api(nlx_ctx* ctx, const nlx_commit* const* oracles, uint32_t n_oracles, const uint32_t* n_next,
                      const uint64_t zeta[2], const uint64_t* openings_zeta, const uint64_t* openings_next,
                      const nlx_fri_params* params, uint32_t hasher, nlx_challenger* challenger, uint8_t* proof_out, size_t proof_cap,
                      size_t* proof_len) {
    if (!ctx) return NLX_E_INVAL;
    if (hasher != NLX_HASHER_POSEIDON_GOLDILOCKS && hasher != NLX_HASHER_POSEIDON_BN128) return ctx->fail(NLX_E_RANGE, "unknown hasher %u", hasher);
    if (!oracles || !n_next || !zeta || !openings_zeta || !params || !challenger || !proof_out || !proof_len)
        return ctx->fail(NLX_E_INVAL, "NULL argument");
    *proof_len = 0;
    if (n_oracles < 1 || n_oracles > 4) return ctx->fail(NLX_E_RANGE, "1..4 oracles");
    for (uint32_t o = 0; o < n_oracles; o++) {
        if (!oracles[o] || oracles[o]->ctx != ctx) return ctx->fail(NLX_E_INVAL, "oracle %u: NULL or from another context", o);
        if (oracles[o]->hasher != hasher)
            return ctx->fail(NLX_E_UNSUPPORTED, hasher == NLX_HASHER_POSEIDON_GOLDILOCKS ? "oracle %u: a PoseidonBN128 commitment cannot enter the Goldilocks transcript"
                                                                                          : "oracle %u: its Merkle tree is not PoseidonBN128", o);
        if (oracles[o]->log_n != oracles[0]->log_n || oracles[o]->rate_bits != oracles[0]->rate_bits ||
            oracles[o]->cap_height != oracles[0]->cap_height)
            return ctx->fail(NLX_E_INVAL, "oracles must share degree, rate and cap height");
    }
    uint32_t n_next_total = 0;
    for (uint32_t o = 0; o < n_oracles; o++) {
        if (n_next[o] > oracles[o]->n_cols) return ctx->fail(NLX_E_RANGE, "n_next[%u] exceeds the oracle's columns", o);
        n_next_total += n_next[o];
    }
    if (n_next_total && !openings_next) return ctx->fail(NLX_E_INVAL, "NULL openings_next");
    if (params->arity_bits < 2 || params->arity_bits > 4 || params->num_queries == 0 || params->num_queries > 128 ||
        params->pow_bits > 40 || oracles[0]->log_n < params->arity_bits)
        return ctx->fail(NLX_E_RANGE, "FRI parameters out of range");
    if (challenger->n_input > 8 || challenger->n_output > 8) return ctx->fail(NLX_E_INVAL, "challenger buffers hold at most 8 elements");
    (void)hipSetDevice(ctx->device);
    const unsigned log_n = oracles[0]->log_n, rate_bits = oracles[0]->rate_bits;
    int32_t rc = ctx->ensure_tables(log_n + rate_bits);
    if (rc) return rc;
    Scratch scratch(ctx);
    // coset bases g * w_L^r and w_A^-i
    const uint32_t R = 1u << rate_bits, A = 1u << params->arity_bits;
    std::vector<uint64_t> small(4 * R + A);
    coset_tables_host(log_n, rate_bits, small.data());
    const uint64_t w_A_inv = gl::inv(gl::root_of_unity(params->arity_bits));
    for (uint32_t i = 0; i < A; i++) small[4 * R + i] = gl::pow(w_A_inv, i);
    uint64_t* d_small = scratch.alloc_as<uint64_t>(small.size() * 8);
    if (!d_small) return NLX_E_NOMEM;
    hipError_t e = hipMemcpyAsync(d_small, small.data(), small.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipMemcpyAsync(tables)");
    FriProveArgs fa;
    for (uint32_t o = 0; o < n_oracles; o++) fa.oracles[o] = oracles[o];
    fa.n_oracles = n_oracles;
    for (uint32_t o = 0; o < n_oracles; o++) fa.nz[o] = n_next[o];
    const uint64_t g = gl::root_of_unity(log_n);
    for (int i = 0; i < 2; i++) { fa.zeta[i] = zeta[i]; fa.gzeta[i] = gl::mul(zeta[i], g); }
    fa.open0 = openings_zeta;
    fa.open1 = openings_next;
    fa.log_n = log_n; fa.rate_bits = rate_bits; fa.cap_height = oracles[0]->cap_height; fa.arity_bits = params->arity_bits;
    fa.pow_bits = params->pow_bits; fa.n_queries = params->num_queries;
    fa.n_rounds = nlx::fri_num_rounds(log_n, rate_bits, oracles[0]->cap_height, params->arity_bits, params->final_poly_bits);
    fa.d_coset_base = d_small;
    fa.d_wA_inv = d_small + 4 * R;
    fa.hasher = hasher;
    Challenger ch;
    memcpy(ch.state, challenger->state, sizeof ch.state);
    memcpy(ch.in_buf, challenger->input, sizeof ch.in_buf);
    memcpy(ch.out_buf, challenger->output, sizeof ch.out_buf);
    ch.n_in = challenger->n_input;
    ch.n_out = challenger->n_output;
    Writer w{proof_out, 0, proof_cap};
    StageClock untimed;
    NLX_RC(scratch.finish(fri_prove(ctx, fa, ch, w, scratch, untimed)));
    if (w.overflow) return ctx->fail(NLX_E_RANGE, "proof buffer too small");
    memcpy(challenger->state, ch.state, sizeof ch.state);
    memcpy(challenger->input, ch.in_buf, sizeof ch.in_buf);
    memcpy(challenger->output, ch.out_buf, sizeof ch.out_buf);
    challenger->n_input = ch.n_in;
    challenger->n_output = ch.n_out;
    *proof_len = w.len;
    return NLX_OK;
}
}  // namespace

extern "C" {

int32_t nlx_fri_prove(nlx_ctx* ctx, const nlx_commit* const* oracles, uint32_t n_oracles, const uint32_t* n_next,
                      const uint64_t zeta[2], const uint64_t* openings_zeta, const uint64_t* openings_next,
                      const nlx_fri_params* params, nlx_challenger* challenger, uint8_t* proof_out, size_t proof_cap,
                      size_t* proof_len) NLX_TRY {
    return fri_prove_api(ctx, oracles, n_oracles, n_next, zeta, openings_zeta, openings_next, params, NLX_HASHER_POSEIDON_GOLDILOCKS,
                         challenger, proof_out, proof_cap, proof_len);
} NLX_CATCH(ctx)

int32_t nlx_fri_prove_hasher(nlx_ctx* ctx, const nlx_commit* const* oracles, uint32_t n_oracles, const uint32_t* n_next,
                             const uint64_t zeta[2], const uint64_t* openings_zeta, const uint64_t* openings_next,
                             const nlx_fri_params* params, uint32_t hasher, nlx_challenger* challenger, uint8_t* proof_out,
                             size_t proof_cap, size_t* proof_len) NLX_TRY {
    return fri_prove_api(ctx, oracles, n_oracles, n_next, zeta, openings_zeta, openings_next, params, hasher, challenger, proof_out,
                         proof_cap, proof_len);
} NLX_CATCH(ctx)

// plonky2::iop::challenger::Challenger on the host, for callers without their own (tests, the C example)
void nlx_challenger_init(nlx_challenger* c) NLX_TRY { if (c) memset(c, 0, sizeof *c); } NLX_CATCH_VOID(nullptr)
int32_t nlx_challenger_observe(nlx_challenger* c, const uint64_t* elements, size_t n) NLX_TRY {
    if (!c || (!elements && n) || c->n_input > 8 || c->n_output > 8) return NLX_E_INVAL;
    Challenger ch;
    memcpy(ch.state, c->state, sizeof ch.state); memcpy(ch.in_buf, c->input, sizeof ch.in_buf);
    memcpy(ch.out_buf, c->output, sizeof ch.out_buf); ch.n_in = c->n_input; ch.n_out = c->n_output;
    for (size_t i = 0; i < n; i++) {
        if (elements[i] >= gl::P) return NLX_E_RANGE;
        ch.observe(elements[i]);
    }
    memcpy(c->state, ch.state, sizeof ch.state); memcpy(c->input, ch.in_buf, sizeof ch.in_buf);
    memcpy(c->output, ch.out_buf, sizeof ch.out_buf); c->n_input = ch.n_in; c->n_output = ch.n_out;
    return NLX_OK;
} NLX_CATCH(nullptr)
// Challenger::observe_hash / observe_cap: n_digests digests of four words under the given hasher (transcript.hpp observe_hash)
int32_t nlx_challenger_observe_hash(nlx_challenger* c, const uint64_t* digests, size_t n_digests, uint32_t hasher) NLX_TRY {
    if (!c || (!digests && n_digests) || c->n_input > 8 || c->n_output > 8) return NLX_E_INVAL;
    if (hasher != NLX_HASHER_POSEIDON_GOLDILOCKS && hasher != NLX_HASHER_POSEIDON_BN128) return NLX_E_RANGE;
    if (hasher == NLX_HASHER_POSEIDON_GOLDILOCKS)
        for (size_t i = 0; i < 4 * n_digests; i++)
            if (digests[i] >= gl::P) return NLX_E_RANGE;
    Challenger ch;
    memcpy(ch.state, c->state, sizeof ch.state); memcpy(ch.in_buf, c->input, sizeof ch.in_buf);
    memcpy(ch.out_buf, c->output, sizeof ch.out_buf); ch.n_in = c->n_input; ch.n_out = c->n_output;
    const int32_t rc = observe_hash(hasher, ch, digests, n_digests);
    if (rc) return rc;
    memcpy(c->state, ch.state, sizeof ch.state); memcpy(c->input, ch.in_buf, sizeof ch.in_buf);
    memcpy(c->output, ch.out_buf, sizeof ch.out_buf); c->n_input = ch.n_in; c->n_output = ch.n_out;
    return NLX_OK;
} NLX_CATCH(nullptr)
int32_t nlx_challenger_challenge(nlx_challenger* c, uint64_t* out, size_t n) NLX_TRY {
    if (!c || (!out && n) || c->n_input > 8 || c->n_output > 8) return NLX_E_INVAL;
    Challenger ch;
    memcpy(ch.state, c->state, sizeof ch.state); memcpy(ch.in_buf, c->input, sizeof ch.in_buf);
    memcpy(ch.out_buf, c->output, sizeof ch.out_buf); ch.n_in = c->n_input; ch.n_out = c->n_output;
    for (size_t i = 0; i < n; i++) out[i] = ch.challenge();
    memcpy(c->state, ch.state, sizeof ch.state); memcpy(c->input, ch.in_buf, sizeof ch.in_buf);
    memcpy(c->output, ch.out_buf, sizeof ch.out_buf); c->n_input = ch.n_in; c->n_output = ch.n_out;
    return NLX_OK;
} NLX_CATCH(nullptr)
int32_t nlx_hash_no_pad(const uint64_t* elements, size_t n, uint64_t out[4]) NLX_TRY {
    if ((!elements && n) || !out) return NLX_E_INVAL;
    for (size_t i = 0; i < n; i++)
        if (elements[i] >= gl::P) return NLX_E_RANGE;
    hash_no_pad_host(elements, n, out);
    for (int i = 0; i < 4; i++) out[i] = gl::canon(out[i]);
    return NLX_OK;
} NLX_CATCH(nullptr)

}  // extern "C"
