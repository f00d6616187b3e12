// STARK verifier (C ABI: nlx_stark_verify, nlx_stark_verify_batch, nlx_stark_proof_bytes): does a proof verify, and if not, which
// check breaks.
//
// starky::verifier::verify_stark_proof for the proofs of stark.hip, one proof or a batch of proofs of one STARK.  On the host:
// the structure of the proof against its layout (stark_proof_layout.hpp), the transcript, the proof of work, the query indices -
// a sponge is a chain, and a proof has one.  On the device, in three launches whatever the number of proofs:
//   k_verify_paths        one quad of lanes per (proof, query, tree): leaf digest of the opened row, the sibling path, the cap
//   k_verify_fri          one wave per (proof, query): fri_combine_initial, the fold chain, the final polynomial; and one wave per
//                         (proof, periodic column): the column at zeta, for the launch below
//   k_verify_constraints  one lane per proof, one block per program segment: the register program at zeta over F_p[X]/(X^2 - 7)
// The device reads the aligned staging copy of the proof only; every address and loop bound comes from the descriptor or from a
// transcript output reduced mod the LDE size, none from a byte of the proof.
#include <algorithm>
#include <memory>
#include <vector>
#include "gl.hpp"
#include "poseidon_quad.hpp"
#include "stark.hpp"
#include "stark_proof_layout.hpp"
#include "transcript.hpp"

using namespace nlx;

namespace nlx {

constexpr uint32_t VERIFY_MAX_TREES = spl::MAX_ORACLES + spl::MAX_LAYERS;
// per proof, what the transcript gave (64-bit words)
enum : uint32_t { PP_ZETA = 0, PP_GZETA = 2, PP_FRI_ALPHA = 4, PP_RED0 = 6, PP_RED1 = 8, PP_ALPHAS = 10, PP_BETAS = 12,
                  PP_VALUES = PP_BETAS + 2 * spl::MAX_LAYERS };
enum : uint32_t { FRI_FAIL_FOLD = 1, FRI_FAIL_FINAL = 2 };   // k_verify_fri's code: kind << 8 | layer

// one Merkle tree of the proof: a trace batch, the quotient oracle or a FRI layer
struct VTree {
    uint32_t w_row, width;      // the opened row (or coset): word offset within the query, words
    uint32_t w_path, path_len;  // siblings
    uint32_t w_cap;             // word offset of the cap within the proof
    uint32_t shift;             // leaf index = x_index >> shift
    uint32_t group;             // leaf_group_cols (0 for a FRI layer)
    uint32_t pad_;
};

struct PathParams {
    const uint64_t* stage;      // [proof][w_total]
    const uint32_t* qidx;       // [proof][query]
    uint8_t* fail;              // [proof][query][tree]: 0 the path holds, 1 it does not (preset to 0xFF: not run)
    size_t w_total, w_queries, w_query_words;
    uint32_t n_items, n_queries, n_trees;
    VTree trees[VERIFY_MAX_TREES];
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

// blockIdx.y = tree, so width, grouping and path length are block-uniform; spare quads redo the last item and store nothing.
// Lane q of a quad holds word q of the running digest.
__global__ __launch_bounds__(64) void k_verify_paths(PathParams p) {
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
    } else if (t.group == 0 || t.width <= t.group) {
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
    const bool ok = cur == base[t.w_cap + (size_t)(idx >> t.path_len) * 4 + q];
    const unsigned long long m = __ballot(ok);
    const bool quad_ok = ((m >> (threadIdx.x & 60u)) & 0xFull) == 0xFull;
    if (live && q == 0) p.fail[(size_t)item * p.n_trees + blockIdx.y] = quad_ok ? 0 : 1;
}

struct FriParams {
    const uint64_t* stage;
    const uint64_t* pp;         // [proof][pp_stride]
    const uint32_t* qidx;
    uint32_t* fail;             // [proof][query]: 0, or kind << 8 | layer
    size_t w_total, w_queries, w_query_words, w_final_poly;
    uint32_t pp_stride, n_queries, n_oracles, n_cols, log_L, arity_bits, n_layers, final_len;
    uint32_t w_row[spl::MAX_ORACLES], width[spl::MAX_ORACLES], w_layer_evals[spl::MAX_LAYERS];
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

// One wave per (proof, query).  The lanes stride over the opened columns for sum_j alpha^j row[j] (lane l starts at alpha^(col0 +
// l) and steps by alpha^64), one wave reduction gives the two batches' sums; the fold chain runs on values every lane holds, with
// the arity terms of each interpolation on lanes 0 .. arity - 1.
// The same launch carries what k_verify_constraints needs once per proof and not once per load: blocks past the queries evaluate
// one periodic column each at y = zeta^(n / period), P_a(y) = sum_m c_m y^m with the lanes striding over m as above.
__global__ __launch_bounds__(64) void k_verify_fri(FriParams p) {
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
    gl::Ext acc_t{0, 0}, acc_q{0, 0};   // trace columns, quotient columns
    uint32_t col0 = 0;
    for (uint32_t o = 0; o < p.n_oracles; o++) {
        const uint64_t* row = qs + p.w_row[o];
        const uint32_t w = p.width[o];
        gl::Ext ap = gl::pow(alpha, col0 + lane), part{0, 0};
        for (uint32_t c = lane; c < w; c += 64) {
            part = gl::add(part, gl::mul(ap, row[c]));
            ap = gl::mul(ap, alpha64);
        }
        if (o + 1 < p.n_oracles) acc_t = gl::add(acc_t, part);
        else acc_q = gl::add(acc_q, part);
        col0 += w;
    }
    acc_t = wave_sum(acc_t);
    acc_q = wave_sum(acc_q);
    uint32_t x_index = p.qidx[item];
    uint64_t sx = gl::mul(gl::GEN, gl::pow(gl::root_of_unity(p.log_L), gl::bitrev32(x_index, p.log_L)));
    // fri_combine_initial: batch 0 at zeta (trace ++ quotient), shifted by alpha^(batch 1's count), batch 1 at g zeta (trace)
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]}, gzeta{pp[PP_GZETA], pp[PP_GZETA + 1]};
    const gl::Ext red0{pp[PP_RED0], pp[PP_RED0 + 1]}, red1{pp[PP_RED1], pp[PP_RED1 + 1]};
    gl::Ext old = gl::mul(gl::sub(gl::add(acc_t, acc_q), red0), gl::inv(base_minus(sx, zeta)));
    old = gl::add(gl::mul(old, gl::pow(alpha, p.n_cols)), gl::mul(gl::sub(acc_t, red1), gl::inv(base_minus(sx, gzeta))));
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
        const gl::Ext beta{pp[PP_BETAS + 2 * k], pp[PP_BETAS + 2 * k + 1]};
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
    const uint64_t* stage;
    const uint64_t* pp;
    const uint64_t* program;    // device (the STARK's own words)
    const uint32_t* seg;        // device: {first word, end word} per segment
    const uint64_t* per;        // [proof][column]: the periodic columns at zeta (k_verify_fri's extra blocks)
    uint64_t* part;             // [proof][segment][challenge] extension elements
    size_t w_total, w_local, w_next;
    uint32_t pp_stride, n_proofs, n_seg, seg0, n_regs, nc, n_pis, log_n, n_periodic;
    uint32_t seg_after[NLX_AIR_MAX_SEGMENTS];
};

__device__ __forceinline__ gl::Ext ext_add_base(gl::Ext x, uint64_t b) { return gl::Ext{gl::add(x.a, b), x.b}; }
__device__ __forceinline__ gl::Ext ext_mul_pow2(gl::Ext x, uint32_t sh) { return gl::Ext{mul_pow2(x.a, sh), mul_pow2(x.b, sh)}; }

// Lane = proof, blockIdx.y = program segment (of this launch group); decode as k_air_check, the register file in LDS as pairs of
// words: regs[reg * blockDim + lane] and regs[(n_regs + reg) * blockDim + lane].  local / next = the openings at zeta / g zeta,
// the filters are (zeta - g^-1), L_first(zeta), L_last(zeta), a periodic column is P_a(zeta^(n / period)) from p.per.  Leaves the segment's
// sum times alpha^(constraints after it) per challenge; the host adds the segments up and compares.
__global__ __launch_bounds__(64) void k_verify_constraints(ConsParams p) {
    extern __shared__ uint64_t regs[];
    const uint32_t proof = blockIdx.x * blockDim.x + threadIdx.x;
    if (proof >= p.n_proofs) return;   // nothing below talks to another lane
    const uint32_t bd = blockDim.x;
    uint64_t* ra = regs + threadIdx.x;
    uint64_t* rb = regs + (size_t)p.n_regs * bd + threadIdx.x;
    auto ld = [&](uint32_t r) { return gl::Ext{ra[r * bd], rb[r * bd]}; };
    auto st = [&](uint32_t r, gl::Ext v) { ra[r * bd] = v.a; rb[r * bd] = v.b; };
    const uint64_t* base = p.stage + (size_t)proof * p.w_total;
    const uint64_t* pp = p.pp + (size_t)proof * p.pp_stride;
    const uint64_t* values = pp + PP_VALUES;
    auto local = [&](uint32_t c) { return gl::Ext{base[p.w_local + 2 * (size_t)c], base[p.w_local + 2 * (size_t)c + 1]}; };
    auto next = [&](uint32_t c) { return gl::Ext{base[p.w_next + 2 * (size_t)c], base[p.w_next + 2 * (size_t)c + 1]}; };
    const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
    const uint64_t g = gl::root_of_unity(p.log_n);
    gl::Ext zeta_n = zeta;
    for (uint32_t i = 0; i < p.log_n; i++) zeta_n = gl::mul(zeta_n, zeta_n);
    const gl::Ext z_h = gl::sub(zeta_n, gl::Ext{1, 0});
    const uint64_t n_f = (uint64_t)1 << p.log_n;
    const gl::Ext z_last = gl::sub(zeta, gl::Ext{gl::inv(g), 0});
    const gl::Ext l_first = gl::mul(z_h, gl::inv(gl::mul(gl::sub(zeta, gl::Ext{1, 0}), n_f)));
    const gl::Ext l_last = gl::mul(z_h, gl::inv(gl::mul(gl::sub(gl::mul(zeta, g), gl::Ext{1, 0}), n_f)));
    const uint64_t alphas[2] = {pp[PP_ALPHAS], pp[PP_ALPHAS + 1]};
    gl::Ext acc[2] = {{0, 0}, {0, 0}};
    auto emit = [&](gl::Ext c) {
        for (uint32_t j = 0; j < p.nc; j++) acc[j] = gl::add(gl::mul(acc[j], alphas[j]), c);
    };
    const uint32_t sg = p.seg0 + blockIdx.y;
    const uint32_t pc_end = p.seg[2 * sg + 1];
    for (uint32_t pc = p.seg[2 * sg]; pc < pc_end; pc++) {
        const uint64_t w = p.program[pc];
        const uint32_t op = (uint32_t)(w & 0xFF), dst = (uint32_t)((w >> 8) & 0xFFFF);
        const uint32_t a = (uint32_t)((w >> 24) & 0xFFFF), b = (uint32_t)((w >> 40) & 0xFFFF);
        const uint32_t sh = (uint32_t)(w >> 56) & 0x3F;
        switch (op) {
            case NLX_AIR_LOCAL: st(dst, local(a)); continue;
            case NLX_AIR_NEXT: st(dst, next(a)); continue;
            case NLX_AIR_PUBLIC: st(dst, gl::Ext{values[a], 0}); continue;
            case NLX_AIR_PERIODIC: {
                const uint64_t* v = p.per + 2 * ((size_t)proof * p.n_periodic + a);
                st(dst, gl::Ext{v[0], v[1]});
                continue;
            }
            case NLX_AIR_CONST: st(dst, gl::Ext{p.program[++pc], 0}); continue;
            case NLX_AIR_ADD: st(dst, gl::add(ld(a), ext_mul_pow2(ld(b), sh))); continue;
            case NLX_AIR_SUB: st(dst, gl::sub(ld(a), ext_mul_pow2(ld(b), sh))); continue;
            case NLX_AIR_MUL: st(dst, gl::mul(ld(a), ld(b))); continue;
            case NLX_AIR_MAC: st(dst, gl::add(ld(sh), gl::mul(ld(a), ld(b)))); continue;
            case NLX_AIR_XOR3:
            case NLX_AIR_CH:
            case NLX_AIR_MAJ: {
                const gl::Ext x = ld(a), y = ld(b), z = ld(sh);
                gl::Ext res;
                if (op == NLX_AIR_CH) {
                    res = gl::add(z, gl::mul(x, gl::sub(y, z)));
                } else {
                    const gl::Ext xy = gl::mul(x, y);
                    const gl::Ext sx = gl::sub(gl::add(x, y), gl::add(xy, xy));
                    if (op == NLX_AIR_XOR3) {
                        const gl::Ext sz = gl::mul(sx, z);
                        res = gl::sub(gl::add(sx, z), gl::add(sz, sz));
                    } else {
                        res = gl::add(xy, gl::mul(z, sx));
                    }
                }
                st(dst, res);
                continue;
            }
            case NLX_AIR_PACK_LOCAL:
            case NLX_AIR_PACK_NEXT: {
                gl::Ext v{0, 0};
                for (uint32_t i = 0; i < b; i++) v = gl::add(v, ext_mul_pow2(op == NLX_AIR_PACK_LOCAL ? local(a + i) : next(a + i), i));
                st(dst, v);
                continue;
            }
            case NLX_AIR_EMIT_BOOL: {
                const uint32_t cnt = b ? b : 1;
                for (uint32_t i = 0; i < cnt; i++) {
                    const gl::Ext v = local(a + i);
                    emit(gl::mul(v, gl::sub(v, gl::Ext{1, 0})));
                }
                continue;
            }
            case NLX_AIR_EMIT_LOGUP: {
                // both coefficients of h (al + v1)(al + v2) - (al + v1) - (al + v2), al = a0 + a1 X a pair of base-field challenges,
                // the columns extension elements here
                const uint64_t a0 = values[p.n_pis + sh], a1 = values[p.n_pis + sh + 1];
                const gl::Ext h0 = local(b), h1 = local(b + 1), v1 = local(a);
                gl::Ext c0, c1;
                if (dst == 0xFFFF) {
                    const gl::Ext d0 = ext_add_base(v1, a0);
                    c0 = gl::sub(gl::add(gl::mul(h0, d0), gl::mul(h1, gl::mul(gl::W, a1))), gl::Ext{1, 0});
                    c1 = gl::add(gl::mul(h0, a1), gl::mul(h1, d0));
                } else {
                    const gl::Ext v2 = local(dst);
                    const gl::Ext s = ext_add_base(gl::add(v1, v2), gl::add(a0, a0));
                    const gl::Ext u0 = ext_add_base(gl::mul(ext_add_base(v1, a0), ext_add_base(v2, a0)), gl::mul(gl::W, gl::mul(a1, a1)));
                    const gl::Ext u1 = gl::mul(s, a1);
                    c0 = gl::sub(gl::add(gl::mul(h0, u0), gl::mul(gl::mul(h1, u1), gl::W)), s);
                    c1 = gl::sub(gl::add(gl::mul(h0, u1), gl::mul(h1, u0)), gl::Ext{gl::add(a1, a1), 0});
                }
                emit(c0);
                emit(c1);
                continue;
            }
            case NLX_AIR_LOADV: continue;   // a scheduling hint: the loads that follow are run as the plain words they are
            case NLX_AIR_EMIT_TRANSITION: emit(gl::mul(ld(a), z_last)); continue;
            case NLX_AIR_EMIT_FIRST: emit(gl::mul(ld(a), l_first)); continue;
            case NLX_AIR_EMIT_LAST: emit(gl::mul(ld(a), l_last)); continue;
            default: emit(ld(a)); continue;   // NLX_AIR_EMIT (the builder validated the opcode range)
        }
    }
    for (uint32_t j = 0; j < p.nc; j++) {
        const gl::Ext v = gl::mul(acc[j], gl::pow(alphas[j], p.seg_after[sg]));
        uint64_t* out = p.part + (((size_t)proof * p.n_seg + sg) * p.nc + j) * 2;
        out[0] = v.a;
        out[1] = v.b;
    }
}

}  // namespace nlx

namespace {

// natural order in, natural-order coefficients out (the interpolation over the len-th roots of unity)
void host_intt(std::vector<uint64_t>& a, unsigned log_len) {
    const size_t len = (size_t)1 << log_len;
    for (size_t i = 0; i < len; i++) {
        size_t j = 0;
        for (unsigned b = 0; b < log_len; b++) j |= ((i >> b) & 1) << (log_len - 1 - b);
        if (j > i) std::swap(a[i], a[j]);
    }
    for (unsigned st = 1; st <= log_len; st++) {
        const size_t half = (size_t)1 << (st - 1);
        const uint64_t w_st = gl::inv(gl::root_of_unity(st));
        for (size_t base = 0; base < len; base += 2 * half) {
            uint64_t w = 1;
            for (size_t k = 0; k < half; k++) {
                const uint64_t u = a[base + k], v = gl::mul(a[base + k + half], w);
                a[base + k] = gl::add(u, v);
                a[base + k + half] = gl::sub(u, v);
                w = gl::mul(w, w_st);
            }
        }
    }
    const uint64_t inv_len = gl::inv((uint64_t)len);
    for (auto& v : a) v = gl::mul(v, inv_len);
}

spl::Shape shape_of(const nlx_stark* s) {
    const nlx_stark_desc& d = s->d;
    spl::Shape sh{};
    sh.degree_bits = d.degree_bits; sh.rate_bits = d.rate_bits; sh.cap_height = d.cap_height; sh.arity_bits = d.fri_arity_bits;
    sh.final_poly_bits = d.fri_final_poly_bits; sh.n_queries = d.fri_num_queries;
    sh.n_cols = d.n_cols; sh.nq = s->nq; sh.n_pis = d.num_public_inputs;
    for (uint32_t r = 0; r < s->n_rounds; r++) {
        sh.n_round_values += s->round_values[r];
        const uint32_t rc = s->round_cols[r];
        const uint32_t nb = d.batch_cols && rc > d.batch_cols ? (rc + d.batch_cols - 1) / d.batch_cols : 1;
        for (uint32_t k = 0; k < nb; k++)   // nlx_stark_build bounds the number of batches
            sh.oracle_cols[sh.n_oracles++] = nb == 1 ? rc : std::min(d.batch_cols, rc - k * d.batch_cols);
    }
    sh.oracle_cols[sh.n_oracles++] = s->nq;
    return sh;
}

// the first verify of a STARK: the periodic columns' interpolation coefficients go to the device and stay
int32_t verify_prepare(nlx_stark* s) {
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    if (s->d_verify || !d.n_periodic) return NLX_OK;
    const size_t period = (size_t)1 << d.period_bits;
    std::vector<uint64_t> coeffs((size_t)d.n_periodic * period), col(period);
    for (uint32_t a = 0; a < d.n_periodic; a++) {
        std::copy(s->periodic.begin() + a * period, s->periodic.begin() + (a + 1) * period, col.begin());
        host_intt(col, d.period_bits);
        std::copy(col.begin(), col.end(), coeffs.begin() + a * period);
    }
    uint64_t* dev = (uint64_t*)ctx->alloc(coeffs.size() * 8);
    if (!dev) return ctx->fail(NLX_E_NOMEM, "out of device memory");
    hipError_t e = hipMemcpyAsync(dev, coeffs.data(), coeffs.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->release(dev);
        return ctx->hip_fail(e, "hipMemcpyAsync(periodic coefficients)");
    }
    s->d_verify = dev;
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
    std::vector<uint64_t> stage, pp;
    std::vector<uint32_t> qidx;
    Scratch scratch;
    explicit VerifyCall(nlx_ctx* ctx) : scratch(ctx) {}
};

int32_t verify_batch(nlx_stark* s, VerifyCall& vc, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                     const uint64_t* public_inputs, nlx_stark_verdict* verdicts) {
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    hipStream_t st = ctx->stream;
    spl::Layout l;
    if (!spl::make_layout(shape_of(s), &l)) return ctx->fail(NLX_E_UNSUPPORTED, "the STARK's proofs have more trees than the verifier takes");
    const uint32_t nQ = d.fri_num_queries, nc = d.num_challenges, qdf = d.quotient_degree_factor, ncols = d.n_cols, nq = s->nq;
    const uint32_t n_pis = d.num_public_inputs, NO = l.sh.n_oracles, R = l.n_layers;
    const unsigned log_n = d.degree_bits, log_L = l.log_L;
    const size_t capw = l.cap_words;
    const uint32_t n_values = n_pis + s->n_round_challenges;
    const uint32_t pp_stride = PP_VALUES + n_values + 1;
    auto reject = [&](size_t i, uint32_t reason) -> nlx_stark_verdict& {
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
        spl::Finding f;
        if (spl::parse(l, proofs[i], lens[i], w, &f) != spl::SOUND) {
            nlx_stark_verdict& v = reject(i, NLX_VERIFY_MALFORMED);
            if (f.what == spl::BAD_PATH_LENGTH) {
                v.query = f.query;
                if (f.tree < NO) v.tree = f.tree;
                else v.layer = f.layer;
            }
            continue;
        }
        const uint64_t* pis = w + l.w_public_inputs;
        if (public_inputs && memcmp(public_inputs + i * n_pis, pis, 8 * (size_t)n_pis) != 0) {
            reject(i, NLX_VERIFY_PUBLIC_INPUTS);
            continue;
        }
        vc.pp.resize((at + 1) * pp_stride, 0);
        uint64_t* pp = vc.pp.data() + at * pp_stride;
        uint64_t* values = pp + PP_VALUES;
        std::copy(pis, pis + n_pis, values);
        Challenger ch;
        ch.observe(s->air_digest, 4);
        ch.observe(pis, n_pis);
        {
            const uint64_t* rv = w + l.w_round_values;
            uint32_t n_drawn = 0, o = 0;
            for (uint32_t rd = 0; rd < s->n_rounds; rd++) {
                const uint32_t rc = s->round_cols[rd];
                const uint32_t nb = d.batch_cols && rc > d.batch_cols ? (rc + d.batch_cols - 1) / d.batch_cols : 1;
                for (uint32_t k = 0; k < nb; k++, o++) ch.observe(w + l.w_caps + o * capw, capw);
                for (uint32_t k = 0; k < s->round_values[rd]; k++) values[n_pis + n_drawn++] = rv[k];
                ch.observe(rv, s->round_values[rd]);
                rv += s->round_values[rd];
                for (uint32_t k = 0; k < s->round_challenges[rd]; k++) values[n_pis + n_drawn++] = ch.challenge();
            }
        }
        for (uint32_t j = 0; j < nc; j++) pp[PP_ALPHAS + j] = ch.challenge();
        ch.observe(w + l.w_caps + (NO - 1) * capw, capw);
        ch.ext_challenge(pp + PP_ZETA);
        const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
        const gl::Ext gzeta = gl::mul(zeta, gl::root_of_unity(log_n));
        pp[PP_GZETA] = gzeta.a;
        pp[PP_GZETA + 1] = gzeta.b;
        const uint64_t *o_local = w + l.w_local, *o_next = w + l.w_next, *o_q = w + l.w_quotient;
        if (!d.openings_group) {
            ch.observe(o_local, 2 * (size_t)ncols);
            ch.observe(o_q, 2 * (size_t)nq);
            ch.observe(o_next, 2 * (size_t)ncols);
        } else {
            // the digest of local ++ quotient ++ next, zero-padded to runs of G: run digests, then their digest
            const size_t G = d.openings_group, len = 2 * (size_t)(2 * ncols + nq), K = (len + G - 1) / G;
            std::vector<uint64_t> v(K * G + 4 * K, 0);
            std::copy(o_local, o_local + 2 * (size_t)ncols, v.begin());
            std::copy(o_q, o_q + 2 * (size_t)nq, v.begin() + 2 * (size_t)ncols);
            std::copy(o_next, o_next + 2 * (size_t)ncols, v.begin() + 2 * (size_t)(ncols + nq));
            for (size_t k = 0; k < K; k++) hash_no_pad_host(v.data() + k * G, G, v.data() + K * G + 4 * k);
            uint64_t out[4];
            hash_no_pad_host(v.data() + K * G, 4 * K, out);
            ch.observe(out, 4);
        }
        ch.ext_challenge(pp + PP_FRI_ALPHA);
        for (uint32_t k = 0; k < R; k++) {
            ch.observe(w + l.w_fri_caps + k * capw, capw);
            ch.ext_challenge(pp + PP_BETAS + 2 * k);
        }
        ch.observe(w + l.w_final_poly, 2 * (size_t)l.final_len);
        ch.observe(w[l.w_pow_witness]);
        const uint64_t pow_response = ch.challenge();
        pow_bad.push_back(d.fri_pow_bits && (pow_response >> (64 - d.fri_pow_bits)) != 0);
        vc.qidx.resize((at + 1) * nQ);
        for (uint32_t q = 0; q < nQ; q++) vc.qidx[at * nQ + q] = (uint32_t)(ch.challenge() & (((uint64_t)1 << log_L) - 1));
        {
            // the reduced openings of the two FRI batches: sum_j alpha^j opened[j]
            const gl::Ext fa{pp[PP_FRI_ALPHA], pp[PP_FRI_ALPHA + 1]};
            gl::Ext ap{1, 0}, r0{0, 0}, r1{0, 0};
            for (uint32_t j = 0; j < ncols; j++) {
                r0 = gl::add(r0, gl::mul(ap, gl::Ext{o_local[2 * j], o_local[2 * j + 1]}));
                r1 = gl::add(r1, gl::mul(ap, gl::Ext{o_next[2 * j], o_next[2 * j + 1]}));
                ap = gl::mul(ap, fa);
            }
            for (uint32_t c = 0; c < nq; c++) {
                r0 = gl::add(r0, gl::mul(ap, gl::Ext{o_q[2 * c], o_q[2 * c + 1]}));
                ap = gl::mul(ap, fa);
            }
            pp[PP_RED0] = r0.a; pp[PP_RED0 + 1] = r0.b;
            pp[PP_RED1] = r1.a; pp[PP_RED1 + 1] = r1.b;
        }
        live.push_back(i);
    }
    const size_t np = live.size();
    if (np) {
        // ---- device ----
        (void)hipSetDevice(ctx->device);
        NLX_RC(verify_prepare(s));
        Scratch& scratch = vc.scratch;
        const uint32_t n_trees = NO + R, n_seg = (uint32_t)s->seg_after.size();
        const size_t n_items = np * nQ;
        if (n_items + np * d.n_periodic > 0x7FFFFFFFu) return ctx->fail(NLX_E_RANGE, "too many proofs in one batch");
        const size_t part_words = np * n_seg * nc * 2;
        uint64_t* d_stage = scratch.alloc_as<uint64_t>(np * l.w_total * 8);
        uint64_t* d_pp = scratch.alloc_as<uint64_t>(np * pp_stride * 8);
        uint32_t* d_qidx = scratch.alloc_as<uint32_t>(n_items * 4);
        uint8_t* d_path_fail = scratch.alloc_as<uint8_t>(n_items * n_trees);
        uint32_t* d_fri_fail = scratch.alloc_as<uint32_t>(n_items * 4);
        uint64_t* d_part = scratch.alloc_as<uint64_t>(part_words * 8);
        uint64_t* d_per = scratch.alloc_as<uint64_t>((np * d.n_periodic + 1) * 16);
        if (!d_stage || !d_pp || !d_qidx || !d_path_fail || !d_fri_fail || !d_part || !d_per) return ctx->fail(NLX_E_NOMEM, "out of device memory");
        NLX_HIP(ctx, hipMemcpyAsync(d_stage, vc.stage.data(), np * l.w_total * 8, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemcpyAsync(d_pp, vc.pp.data(), np * pp_stride * 8, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemcpyAsync(d_qidx, vc.qidx.data(), n_items * 4, hipMemcpyHostToDevice, st));
        NLX_HIP(ctx, hipMemsetAsync(d_path_fail, 0xFF, n_items * n_trees, st));   // as the two below: what no kernel writes
        NLX_HIP(ctx, hipMemsetAsync(d_fri_fail, 0xFF, n_items * 4, st));
        NLX_HIP(ctx, hipMemsetAsync(d_part, 0xFF, part_words * 8, st));   // a segment that did not run can never pass for one that did

        {
            PathParams pa{};
            pa.stage = d_stage; pa.qidx = d_qidx; pa.fail = d_path_fail;
            pa.w_total = l.w_total; pa.w_queries = l.w_queries; pa.w_query_words = l.w_query_words;
            pa.n_items = (uint32_t)n_items; pa.n_queries = nQ; pa.n_trees = n_trees;
            for (uint32_t o = 0; o < NO; o++)
                pa.trees[o] = VTree{(uint32_t)l.w_row[o], l.sh.oracle_cols[o], (uint32_t)l.w_path[o], l.oracle_plen,
                                    (uint32_t)(l.w_caps + o * capw), 0, d.leaf_group_cols, 0};
            for (uint32_t k = 0; k < R; k++)
                pa.trees[NO + k] = VTree{(uint32_t)l.w_layer_evals[k], 2 * l.arity, (uint32_t)l.w_layer_path[k], l.layer_plen[k],
                                         (uint32_t)(l.w_fri_caps + k * capw), (k + 1) * d.fri_arity_bits, 0, 0};
            size_t perms = 0;
            for (uint32_t t = 0; t < n_trees; t++) perms += (pa.trees[t].width + 7) / 8 + pa.trees[t].path_len;
            ctx->begin_kernel("stark_verify_paths", 8.0 * np * l.w_total, (double)perms * n_items);
            hipLaunchKernelGGL(k_verify_paths, dim3((unsigned)((n_items + 15) / 16), n_trees), dim3(64), 0, st, pa);
            ctx->end_kernel();
        }
        {
            FriParams fp{};
            fp.stage = d_stage; fp.pp = d_pp; fp.qidx = d_qidx; fp.fail = d_fri_fail;
            fp.w_total = l.w_total; fp.w_queries = l.w_queries; fp.w_query_words = l.w_query_words; fp.w_final_poly = l.w_final_poly;
            fp.pp_stride = pp_stride; fp.n_queries = nQ; fp.n_oracles = NO; fp.n_cols = ncols; fp.log_L = log_L;
            fp.arity_bits = d.fri_arity_bits; fp.n_layers = R; fp.final_len = l.final_len;
            for (uint32_t o = 0; o < NO; o++) { fp.w_row[o] = (uint32_t)l.w_row[o]; fp.width[o] = l.sh.oracle_cols[o]; }
            for (uint32_t k = 0; k < R; k++) fp.w_layer_evals[k] = (uint32_t)l.w_layer_evals[k];
            fp.per_coeffs = s->d_verify; fp.per = d_per;
            fp.n_items = (uint32_t)n_items; fp.n_periodic = d.n_periodic; fp.period_bits = d.n_periodic ? d.period_bits : 0; fp.log_n = log_n;
            ctx->begin_kernel("stark_verify_fri", 8.0 * n_items * l.w_query_words);
            hipLaunchKernelGGL(k_verify_fri, dim3((unsigned)(n_items + np * d.n_periodic)), dim3(64), 0, st, fp);
            ctx->end_kernel();
        }
        {
            ConsParams cp{};
            cp.stage = d_stage; cp.pp = d_pp; cp.program = s->d_program; cp.seg = s->d_seg; cp.per = d_per; cp.part = d_part;
            cp.w_total = l.w_total; cp.w_local = l.w_local; cp.w_next = l.w_next;
            cp.pp_stride = pp_stride; cp.n_proofs = (uint32_t)np; cp.n_seg = n_seg; cp.nc = nc; cp.n_pis = n_pis; cp.log_n = log_n;
            cp.n_periodic = d.n_periodic;
            for (uint32_t sg = 0; sg < n_seg; sg++) cp.seg_after[sg] = s->seg_after[sg];
            unsigned bs = 64;
            while (bs > 1 && bs / 2 >= np) bs >>= 1;
            ctx->begin_kernel("stark_verify_constraints", 8.0 * np * 4.0 * ncols);
            // the launch groups of the quotient: segments of a similar register need share a launch
            for (size_t gi = 0; gi < s->seg_group.size(); gi++) {
                const uint32_t first = s->seg_group[gi], last = gi + 1 < s->seg_group.size() ? s->seg_group[gi + 1] : n_seg;
                cp.seg0 = first;
                cp.n_regs = s->seg_regs[last - 1];
                const size_t lds = (size_t)bs * cp.n_regs * 16;
                hipLaunchKernelGGL(k_verify_constraints, dim3((unsigned)((np + bs - 1) / bs), last - first), dim3(bs), lds, st, cp);
            }
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

        // ---- the verdicts, in the order of a sequential verifier ----
        for (size_t at = 0; at < np; at++) {
            const size_t i = live[at];
            const uint64_t* w = vc.stage.data() + at * l.w_total;
            const uint64_t* pp = vc.pp.data() + at * pp_stride;
            const gl::Ext zeta{pp[PP_ZETA], pp[PP_ZETA + 1]};
            gl::Ext zeta_n = zeta;
            for (unsigned k = 0; k < log_n; k++) zeta_n = gl::mul(zeta_n, zeta_n);
            const gl::Ext z_h = gl::sub(zeta_n, gl::Ext{1, 0});
            bool done = false;
            for (uint32_t j = 0; j < nc && !done; j++) {
                gl::Ext sum{0, 0}, t{0, 0};
                for (uint32_t sg = 0; sg < n_seg; sg++) {
                    const uint64_t* pv = part.data() + ((at * n_seg + sg) * nc + j) * 2;
                    if (pv[0] >= gl::P || pv[1] >= gl::P) return ctx->fail(NLX_E_HIP, "the constraint kernel left a segment unwritten");
                    sum = gl::add(sum, gl::Ext{pv[0], pv[1]});
                }
                const uint64_t* o_q = w + l.w_quotient + 2 * (size_t)j * qdf;
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
                for (uint32_t o = 0; o < NO && !reason; o++)
                    if (pf[o]) { reason = NLX_VERIFY_TRACE_PATH; tree = o; }
                for (uint32_t k = 0; k < R && !reason; k++) {
                    if ((ff >> 8) == FRI_FAIL_FOLD && (ff & 0xFF) == k) { reason = NLX_VERIFY_FRI_FOLD; layer = k; }
                    else if (pf[NO + k]) { reason = NLX_VERIFY_FRI_PATH; layer = k; }
                }
                if (!reason && (ff >> 8) == FRI_FAIL_FINAL) reason = NLX_VERIFY_FINAL_POLY;
                if (reason) {
                    nlx_stark_verdict& v = reject(i, reason);
                    v.query = q; v.tree = tree; v.layer = layer; v.x_index = vc.qidx[item];
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
            const nlx_stark_verdict& v = verdicts[i];
            // NLX_OK: the check ran.  The line is for nlx_last_error.
            ctx->fail(NLX_OK, "proof %llu does not verify: %s (reason %u), challenge %u, query %u (x_index %llu), tree %u, layer %u",
                      (unsigned long long)i, reason_name(v.reason), v.reason, v.challenge, v.query, (unsigned long long)v.x_index, v.tree, v.layer);
            return NLX_OK;
        }
    ctx->err.clear();   // every proof verifies: no line of an earlier rejection stays behind
    return NLX_OK;
}

}  // namespace

extern "C" {

size_t nlx_stark_proof_bytes(const nlx_stark* s) NLX_TRY {
    spl::Layout l;
    return s && spl::make_layout(shape_of(s), &l) ? l.total : 0;
} NLX_CATCH_VALUE(nullptr, 0)

int32_t nlx_stark_verify_batch(nlx_stark* s, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                               const uint64_t* public_inputs, nlx_stark_verdict* verdicts) NLX_TRY {
    if (verdicts && n_proofs) memset(verdicts, 0, n_proofs * sizeof *verdicts);
    if (!s) return NLX_E_INVAL;
    nlx_ctx* ctx = s->ctx;
    if (n_proofs && (!proofs || !lens || !verdicts)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ctx->fail(NLX_E_INVAL, "proof %llu is NULL", (unsigned long long)i);
    if (public_inputs)
        for (size_t i = 0; i < n_proofs * s->d.num_public_inputs; i++)
            if (public_inputs[i] >= gl::P)
                return ctx->fail(NLX_E_RANGE, "public input %llu of proof %llu is not canonical", (unsigned long long)(i % s->d.num_public_inputs),
                                 (unsigned long long)(i / s->d.num_public_inputs));
    if (!n_proofs) return NLX_OK;
    VerifyCall vc(ctx);
    const int32_t rc = vc.scratch.finish(verify_batch(s, vc, proofs, lens, n_proofs, public_inputs, verdicts));
    if (rc) memset(verdicts, 0, n_proofs * sizeof *verdicts);   // an error is no verdict
    return rc;
} NLX_CATCH(s ? s->ctx : nullptr)

int32_t nlx_stark_verify(nlx_stark* s, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                         nlx_stark_verdict* verdict) NLX_TRY {
    if (verdict) memset(verdict, 0, sizeof *verdict);
    if (!s) return NLX_E_INVAL;
    if (!proof || !verdict) return s->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_stark_verify_batch(s, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(s ? s->ctx : nullptr)

}  // extern "C"
