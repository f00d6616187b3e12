// STARK verifier (C ABI: nlx_stark_verify, nlx_stark_verify_batch, nlx_stark_proof_bytes): does a proof verify, and if not, which
// check breaks.
//
// starky::verifier::verify_stark_proof for the proofs of stark.hip, one proof or a batch of proofs of one STARK.  What a STARK
// proof shares with every proof that has a FRI proof in it is fri_verify.hip's: the parser, the transcript from the FRI caps on,
// the path and query kernels, the verdicts.  Here is what is a STARK's own: the head of the transcript (stark_proof_layout.hpp),
// the runs of opened columns that enter the FRI batches, and the third launch with its judgement:
//   k_verify_constraints  one lane per proof, one block per program segment: the register program at zeta over F_p[X]/(X^2 - 7)
#include <algorithm>
#include <memory>
#include <vector>
#include "fri_verify.hpp"
#include "stark.hpp"
#include "stark_proof_layout.hpp"

using namespace nlx;

namespace nlx {

using namespace fv;
// per proof, what the transcript gave after the common prefix (64-bit words)
enum : uint32_t { PP_ALPHAS = PP_OWN, PP_VALUES = PP_ALPHAS + 2 };

struct ConsParams {
    const uint64_t* stage;
    const uint64_t* pp;
    const uint64_t* program;    // device (the STARK's own words)
    const uint32_t* seg;        // device: {first word, end word} per segment
    const uint64_t* per;        // [proof][column]: the periodic columns at zeta (k_fri_queries' extra blocks)
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

int32_t verify_batch(nlx_stark* s, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs, const uint64_t* public_inputs,
                     nlx_stark_verdict* verdicts) {
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    spl::Layout l;
    if (!spl::make_layout(shape_of(s), &l)) return ctx->fail(NLX_E_UNSUPPORTED, "the STARK's proofs have more trees than the verifier takes");
    const uint32_t nc = d.num_challenges, qdf = d.quotient_degree_factor, ncols = d.n_cols, nq = s->nq;
    const uint32_t n_pis = d.num_public_inputs, NO = l.n_trees, n_seg = (uint32_t)s->seg_after.size();
    const size_t capw = l.cap_words;
    Verifier v;
    v.ctx = ctx; v.lay = &l;
    v.log_n = d.degree_bits; v.arity_bits = d.fri_arity_bits; v.pow_bits = d.fri_pow_bits;
    v.pp_stride = PP_VALUES + n_pis + s->n_round_challenges + 1;
    v.w_caps = l.w_caps; v.grouped_leaves = true; v.leaf_group = d.leaf_group_cols;
    // the trace commitments enter both batches with the same powers of alpha, the quotient the batch at zeta alone
    for (uint32_t o = 0, col0 = 0; o < NO; col0 += l.tree_cols[o++])
        v.runs[v.n_runs++] = FriRun{(uint32_t)l.w_row[o], l.tree_cols[o], col0, o + 1 < NO ? 3u : 1u};
    v.batch_shift = ncols;
    v.n_periodic = d.n_periodic; v.period_bits = d.n_periodic ? d.period_bits : 0;
    v.part_words = (size_t)n_seg * nc * 2;
    v.name_paths = "stark_verify_paths"; v.name_fri = "stark_verify_fri";
    v.part_unwritten = "the constraint kernel left a segment unwritten";
    v.head = [&](const uint64_t* w, uint64_t* pp, Challenger& ch) {
        const uint64_t* pis = w + l.w_public_inputs;
        uint64_t* values = pp + PP_VALUES;
        std::copy(pis, pis + n_pis, values);
        ch.observe(s->air_digest, 4);
        ch.observe(pis, n_pis);
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
        for (uint32_t j = 0; j < nc; j++) pp[PP_ALPHAS + j] = ch.challenge();
        ch.observe(w + l.w_caps + (NO - 1) * capw, capw);
        draw_zeta(ch, pp, d.degree_bits);
        const uint64_t *o_local = w + l.w_local, *o_next = w + l.w_next, *o_q = w + l.w_quotient;
        if (!d.openings_group) {
            ch.observe(o_local, 2 * (size_t)ncols);
            ch.observe(o_q, 2 * (size_t)nq);
            ch.observe(o_next, 2 * (size_t)ncols);
        } else {
            // the digest of local ++ quotient ++ next, zero-padded to runs of G: run digests, then their digest
            const size_t G = d.openings_group, len = 2 * (size_t)(2 * ncols + nq), K = (len + G - 1) / G;
            std::vector<uint64_t> run(K * G + 4 * K, 0);
            std::copy(o_local, o_local + 2 * (size_t)ncols, run.begin());
            std::copy(o_q, o_q + 2 * (size_t)nq, run.begin() + 2 * (size_t)ncols);
            std::copy(o_next, o_next + 2 * (size_t)ncols, run.begin() + 2 * (size_t)(ncols + nq));
            for (size_t k = 0; k < K; k++) hash_no_pad_host(run.data() + k * G, G, run.data() + K * G + 4 * k);
            uint64_t out[4];
            hash_no_pad_host(run.data() + K * G, 4 * K, out);
            ch.observe(out, 4);
        }
        ch.ext_challenge(pp + PP_FRI_ALPHA);
        reduce_openings(pp, {{o_local, ncols}, {o_q, nq}}, pp + PP_RED0);
        reduce_openings(pp, {{o_next, ncols}}, pp + PP_RED1);
    };
    v.prepare = [&]() {
        NLX_RC(verify_prepare(s));
        v.per_coeffs = s->d_verify;
        return (int32_t)NLX_OK;
    };
    v.constraints = [&](const Device& dev) {
        const size_t np = dev.n_proofs;
        ConsParams cp{};
        cp.stage = dev.stage; cp.pp = dev.pp; cp.program = s->d_program; cp.seg = s->d_seg; cp.per = dev.per; cp.part = dev.part;
        cp.w_total = l.w_total; cp.w_local = l.w_local; cp.w_next = l.w_next;
        cp.pp_stride = v.pp_stride; cp.n_proofs = (uint32_t)np; cp.n_seg = n_seg; cp.nc = nc; cp.n_pis = n_pis; cp.log_n = d.degree_bits;
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
            hipLaunchKernelGGL(k_verify_constraints, dim3((unsigned)((np + bs - 1) / bs), last - first), dim3(bs), lds, ctx->stream, cp);
        }
        ctx->end_kernel();
        return (int32_t)NLX_OK;
    };
    v.judge = [&](const uint64_t* w, const uint64_t* pp, const uint64_t* part) {
        const ZetaN z(gl::Ext{pp[PP_ZETA], pp[PP_ZETA + 1]}, d.degree_bits);
        for (uint32_t j = 0; j < nc; j++) {
            gl::Ext sum{0, 0};
            for (uint32_t sg = 0; sg < n_seg; sg++) sum = gl::add(sum, gl::Ext{part[(sg * nc + j) * 2], part[(sg * nc + j) * 2 + 1]});
            if (!z.divides(sum, w + l.w_quotient + 2 * (size_t)j * qdf, qdf)) return j;
        }
        return NO_CHALLENGE;
    };
    VerifyCall vc(ctx);
    return fv::verify_batch(v, vc, proofs, lens, n_proofs, public_inputs, verdicts);
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
    NLX_RC(check_batch_args(s->ctx, proofs, lens, n_proofs, public_inputs, s->d.num_public_inputs, verdicts));
    return n_proofs ? verify_batch(s, proofs, lens, n_proofs, public_inputs, verdicts) : NLX_OK;
} NLX_CATCH(s ? s->ctx : nullptr)

int32_t nlx_stark_verify(nlx_stark* s, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                         nlx_stark_verdict* verdict) NLX_TRY {
    if (verdict) memset(verdict, 0, sizeof *verdict);
    if (!s) return NLX_E_INVAL;
    if (!proof || !verdict) return s->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_stark_verify_batch(s, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(s ? s->ctx : nullptr)

}  // extern "C"
