// STARK trace checker (C ABI: nlx_stark_check_trace, nlx_stark_check_rounds): which row and which constraint a trace breaks.
//
// nlx_stark_prove never asks whether the trace satisfies the AIR: a wrong trace becomes proof bytes a verifier rejects.  The
// checker runs the STARK's own register program on the n TRACE ROWS - plain columns in natural order, no LDE, no hashing, no
// transcript - with the filters of the quotient turned into row predicates, and reports every (row, constraint) pair that is not
// zero: the first one (lowest row, then lowest constraint index) with its value and the program word that emitted it, the number
// of bad rows and pairs, and a count per constraint.
//
// The interpreter here is a kernel of its own, beside k_air_quotient (stark.hip) and the generated kernels (csrc/airgen/): those
// keep their code.  It always runs, whether or not the STARK has a generated quotient kernel.
#include <algorithm>
#include <memory>
#include <vector>
#include "gl.hpp"
#include "stark.hpp"
#include "transcript.hpp"

using namespace nlx;

namespace nlx {

// the findings' meeting place on the device (64-bit words)
enum : uint32_t { CHK_FIRST = 0, CHK_PAIRS = 1, CHK_ROWS = 2, CHK_VALUE = 3, CHK_WORD_KIND = 4, CHK_SUB = 5, CHK_WORDS = 8 };

struct AirCheckParams {
    const uint64_t* const* cols;          // device: cols[c] = column c of the trace, n values in natural order
    const uint64_t* program;              // device (the STARK's own words)
    const uint64_t* pis;                  // device: public inputs | round values and challenges in values-array order
    const uint64_t* periodic;             // device: [column][row mod period], the table as the caller gave it
    const uint32_t* seg;                  // device: {first word, end word} per segment of this launch
    const uint32_t* seg_first;            // device: index of the first constraint each of them emits
    unsigned long long* block;            // CHK_*
    unsigned long long* per_constraint;   // [n_constraints]
    uint8_t* row_bad;                     // [n]
    uint32_t log_n, period_bits, n_pis;
    uint32_t row, target;                 // DETAIL: the one row to run and the constraint whose value is wanted
};

// One lane per trace row i, blockIdx.y = program segment; the register file in LDS as in k_air_quotient (regs[reg * blockDim +
// lane]), decode wave-uniform.  local = row i, next = row (i + 1) mod n.  A constraint counts on the rows its instruction names
// (EMIT_FIRST: row 0, EMIT_LAST: row n - 1, EMIT_TRANSITION: rows 0 .. n - 2, the others: every row) and is zero elsewhere.
// A block is one wave or less, so a ballot sees the whole block: per failing constraint one lane adds the wave's count.
// DETAIL: a single lane runs row p.row through one segment and leaves constraint p.target's value, word and kind in the block.
template <bool DETAIL>
__global__ __launch_bounds__(64) void k_air_check(AirCheckParams p) {
    extern __shared__ uint64_t regs[];
    const uint32_t n_mask = (1u << p.log_n) - 1;   // the host checked n >= blockDim.x: whole blocks
    const uint32_t row = DETAIL ? p.row : blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t row_next = (row + 1) & n_mask;
    const bool on_first = row == 0, on_last = row == n_mask;
    const size_t per = row & ((1u << p.period_bits) - 1);
    uint64_t* my = regs + threadIdx.x;
    const uint32_t bd = blockDim.x, lane = threadIdx.x;
    const uint32_t sg = blockIdx.y;
    uint32_t ci = p.seg_first[sg];      // wave-uniform: the index of the next constraint
    uint32_t my_first = 0xFFFFFFFFu;    // this row's lowest failing constraint in this segment
    uint32_t wave_pairs = 0;            // wave-uniform
    auto emit = [&](uint64_t c, bool on, uint32_t op, uint32_t pc, uint32_t sub) {
        if constexpr (DETAIL) {
            if (ci == p.target) {
                p.block[CHK_VALUE] = c;
                p.block[CHK_WORD_KIND] = (unsigned long long)pc | (unsigned long long)op << 32;
                p.block[CHK_SUB] = sub;
            }
        } else {
            const bool bad = on && c != 0;
            const unsigned long long m = __ballot(bad);
            if (m) {
                if (bad && my_first == 0xFFFFFFFFu) my_first = ci;
                const uint32_t cnt = (uint32_t)__popcll(m);
                wave_pairs += cnt;
                if (lane == (uint32_t)__ffsll(m) - 1) atomicAdd(&p.per_constraint[ci], (unsigned long long)cnt);
            }
        }
        ci++;
    };
    const uint32_t pc_end = p.seg[2 * sg + 1];
    for (uint32_t pc = p.seg[2 * sg]; pc < pc_end; pc++) {
        const uint64_t w = p.program[pc];
        const uint32_t op = (uint32_t)(w & 0xFF), dst = (uint32_t)((w >> 8) & 0xFFFF);
        const uint32_t a = (uint32_t)((w >> 24) & 0xFFFF), b = (uint32_t)((w >> 40) & 0xFFFF);
        const uint32_t sh = (uint32_t)(w >> 56) & 0x3F;
        switch (op) {
            case NLX_AIR_LOCAL: my[dst * bd] = p.cols[a][row]; continue;
            case NLX_AIR_NEXT: my[dst * bd] = p.cols[a][row_next]; continue;
            case NLX_AIR_PUBLIC: my[dst * bd] = p.pis[a]; continue;
            case NLX_AIR_PERIODIC: my[dst * bd] = p.periodic[((size_t)a << p.period_bits) + per]; continue;
            case NLX_AIR_CONST: my[dst * bd] = p.program[++pc]; continue;
            case NLX_AIR_ADD: my[dst * bd] = gl::add(my[a * bd], mul_pow2(my[b * bd], sh)); continue;
            case NLX_AIR_SUB: my[dst * bd] = gl::sub(my[a * bd], mul_pow2(my[b * bd], sh)); continue;
            case NLX_AIR_MUL: my[dst * bd] = gl::mul(my[a * bd], my[b * bd]); continue;
            case NLX_AIR_MAC: my[dst * bd] = gl::add(my[sh * bd], gl::mul(my[a * bd], my[b * bd])); continue;
            case NLX_AIR_XOR3:
            case NLX_AIR_CH:
            case NLX_AIR_MAJ: {
                const uint64_t x = my[a * bd], y = my[b * bd], z = my[sh * bd];
                uint64_t res;
                if (op == NLX_AIR_CH) {
                    res = gl::add(z, gl::mul(x, gl::sub(y, z)));
                } else {
                    const uint64_t xy = gl::mul(x, y);
                    const uint64_t sx = gl::sub(gl::add(x, y), gl::add(xy, xy));
                    if (op == NLX_AIR_XOR3) {
                        const uint64_t sz = gl::mul(sx, z);
                        res = gl::sub(gl::add(sx, z), gl::add(sz, sz));
                    } else {
                        res = gl::add(xy, gl::mul(z, sx));
                    }
                }
                my[dst * bd] = res;
                continue;
            }
            case NLX_AIR_PACK_LOCAL:
            case NLX_AIR_PACK_NEXT: {
                const uint32_t rr = op == NLX_AIR_PACK_LOCAL ? row : row_next;
                uint64_t acc = 0;
                for (uint32_t i = 0; i < b; i++) acc = gl::add(acc, mul_pow2(p.cols[a + i][rr], i));
                my[dst * bd] = acc;
                continue;
            }
            case NLX_AIR_EMIT_BOOL: {
                const uint32_t cnt = b ? b : 1;
                for (uint32_t i0 = 0; i0 < cnt; i0 += 8) {
                    uint64_t v[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) v[i] = i0 + i < cnt ? p.cols[a + i0 + i][row] : 0;
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        if (i0 + i < cnt) emit(gl::mul(v[i], gl::sub(v[i], 1)), true, op, pc, i0 + i);
                }
                continue;
            }
            case NLX_AIR_EMIT_LOGUP: {
                // both coefficients of h (al + v1)(al + v2) - (al + v1) - (al + v2) over F_p[X]/(X^2 - 7), as k_air_quotient
                const uint64_t al0 = p.pis[p.n_pis + sh], al1 = p.pis[p.n_pis + sh + 1];
                const uint64_t h0 = p.cols[b][row], h1 = p.cols[b + 1][row], v1 = p.cols[a][row];
                uint64_t c0, c1;
                if (dst == 0xFFFF) {
                    const uint64_t d0 = gl::add(al0, v1);
                    c0 = gl::sub(gl::add(gl::mul(h0, d0), mul_pow2(gl::mul(h1, al1), 3)), gl::add(gl::mul(h1, al1), 1));
                    c1 = gl::add(gl::mul(h0, al1), gl::mul(h1, d0));
                } else {
                    const uint64_t v2 = p.cols[dst][row];
                    const uint64_t s2 = gl::add(gl::add(al0, al0), gl::add(v1, v2));
                    const uint64_t a1sq = gl::mul(al1, al1);
                    const uint64_t u0 = gl::add(gl::mul(gl::add(al0, v1), gl::add(al0, v2)), gl::sub(mul_pow2(a1sq, 3), a1sq));
                    const uint64_t u1 = gl::mul(al1, s2);
                    const uint64_t hu = gl::mul(h1, u1);
                    c0 = gl::sub(gl::add(gl::mul(h0, u0), gl::sub(mul_pow2(hu, 3), hu)), s2);
                    c1 = gl::sub(gl::add(gl::mul(h0, u1), gl::mul(h1, u0)), gl::add(al1, al1));
                }
                emit(c0, true, op, pc, 0);
                emit(c1, true, op, pc, 1);
                continue;
            }
            case NLX_AIR_LOADV: continue;   // a scheduling hint: the loads that follow are run as the plain words they are
            case NLX_AIR_EMIT_TRANSITION: emit(my[a * bd], !on_last, op, pc, 0); continue;
            case NLX_AIR_EMIT_FIRST: emit(my[a * bd], on_first, op, pc, 0); continue;
            case NLX_AIR_EMIT_LAST: emit(my[a * bd], on_last, op, pc, 0); continue;
            default: emit(my[a * bd], true, op, pc, 0); continue;  // NLX_AIR_EMIT (the host validated the opcode range)
        }
    }
    if constexpr (!DETAIL) {
        const bool row_is_bad = my_first != 0xFFFFFFFFu;
        const unsigned long long m = __ballot(row_is_bad);
        if (m) {
            if (row_is_bad) p.row_bad[row] = 1;
            if (lane == (uint32_t)__ffsll(m) - 1) {   // the wave's lowest bad row, and that row's lowest constraint
                atomicMin(&p.block[CHK_FIRST], (unsigned long long)row << 32 | my_first);
                atomicAdd(&p.block[CHK_PAIRS], (unsigned long long)wave_pairs);
            }
        }
    }
}

// rows with a flag
__global__ __launch_bounds__(256) void k_air_check_rows(const uint8_t* __restrict__ row_bad, size_t n, unsigned long long* __restrict__ out) {
    uint32_t cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) cnt += row_bad[i];
    for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, (unsigned long long)cnt);
}

}  // namespace nlx

namespace {

const char* emit_kind_name(uint32_t op) {
    switch (op) {
        case NLX_AIR_EMIT_TRANSITION: return "transition";
        case NLX_AIR_EMIT_FIRST: return "first row";
        case NLX_AIR_EMIT_LAST: return "last row";
        case NLX_AIR_EMIT_BOOL: return "boolean";
        case NLX_AIR_EMIT_LOGUP: return "logup";
        default: return "every row";
    }
}

// what the first check of a STARK makes and the STARK keeps: each segment's first constraint index, the periodic table as it
// stands, the findings block
int32_t check_prepare(nlx_stark* s) {
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    if (s->d_check) return NLX_OK;
    const uint32_t n_seg = (uint32_t)s->seg_after.size();
    s->seg_first.assign(n_seg, 0);
    for (uint32_t sg = 0; sg < n_seg; sg++) {
        uint32_t own = 0;
        for (uint32_t pc = s->seg[2 * sg]; pc < s->seg[2 * sg + 1]; pc++) {
            const uint64_t w = s->program[pc];
            const uint32_t op = (uint32_t)(w & 0xFF), b = (uint32_t)((w >> 40) & 0xFFFF);
            if (op == NLX_AIR_CONST) pc++;
            else if (op >= NLX_AIR_EMIT_TRANSITION && op <= NLX_AIR_EMIT) own++;
            else if (op == NLX_AIR_EMIT_BOOL) own += b ? b : 1;
            else if (op == NLX_AIR_EMIT_LOGUP) own += 2;
        }
        s->seg_first[sg] = s->n_constraints - s->seg_after[sg] - own;
    }
    uint32_t* d_first = (uint32_t*)ctx->alloc((size_t)n_seg * 4);
    uint64_t* d_rows = d.n_periodic ? (uint64_t*)ctx->alloc(s->periodic.size() * 8) : nullptr;
    uint64_t* d_block = (uint64_t*)ctx->alloc(CHK_WORDS * 8);
    hipError_t e = hipSuccess;
    if (d_first && d_block && (d_rows || !d.n_periodic)) {
        e = hipMemcpyAsync(d_first, s->seg_first.data(), (size_t)n_seg * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && d_rows) e = hipMemcpyAsync(d_rows, s->periodic.data(), s->periodic.size() * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) {
            s->d_seg_first = d_first;
            s->d_periodic_rows = d_rows;
            s->d_check = d_block;
            return NLX_OK;
        }
    }
    ctx->release(d_first);
    ctx->release(d_rows);
    ctx->release(d_block);
    return e != hipSuccess ? ctx->hip_fail(e, "hipMemcpyAsync(checker tables)") : ctx->fail(NLX_E_NOMEM, "out of device memory");
}

// What one check holds until its stream work has drained.  Members go in reverse order: the scratch first - which synchronises -,
// then the last round's staging block, then the host sources of the asynchronous copies.
struct CheckCall {
    std::vector<uint64_t> values;           // readable by NLX_AIR_PUBLIC: the public inputs, then round values and challenges
    std::vector<const uint64_t*> h_cols;
    uint64_t block0[CHK_WORDS] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    std::unique_ptr<Staged> last_round;
    Scratch scratch;
    explicit CheckCall(nlx_ctx* ctx) : scratch(ctx) {}
};

int32_t check_rounds(nlx_stark* s, CheckCall& cc, nlx_round_fn round_fn, void* user, const uint64_t* public_inputs,
                     const uint64_t* challenges, nlx_trace_report* rep, uint64_t* per_constraint) {
    Scratch& scratch = cc.scratch;
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    hipStream_t st = ctx->stream;
    const unsigned log_n = d.degree_bits;
    const size_t n = (size_t)1 << log_n;
    const uint32_t ncols = d.n_cols, NRD = s->n_rounds, N = s->n_constraints;
    rep->n_constraints = N;
    NLX_RC(check_prepare(s));

    // the rounds, called as nlx_stark_prove_rounds calls them; nothing is committed, so a round's challenges come from a
    // transcript of the statement and the earlier rounds' values alone (or from the caller)
    Challenger ch;
    ch.observe(s->air_digest, 4);
    ch.observe(public_inputs, d.num_public_inputs);
    std::vector<uint64_t>& values = cc.values;
    values.assign(public_inputs, public_inputs + d.num_public_inputs);
    std::vector<const uint64_t*>& h_cols = cc.h_cols;
    h_cols.resize(ncols);
    std::unique_ptr<Staged>& last_round = cc.last_round;
    uint32_t col0 = 0;
    for (uint32_t r = 0; r < NRD; r++) {
        const uint32_t rcols = s->round_cols[r], n_rv = s->round_values[r];
        uint64_t rv[64];
        const uint64_t* tr_ptr = round_fn(user, r, values.data() + d.num_public_inputs, (uint32_t)(values.size() - d.num_public_inputs),
                                          n_rv ? rv : nullptr);
        if (!tr_ptr) return ctx->fail(NLX_E_INVAL, "round %u: the round callback returned NULL", r);
        for (uint32_t k = 0; k < n_rv; k++) rv[k] %= gl::P;
        const size_t bytes = (size_t)rcols * n * 8;
        const uint64_t* d_tr;
        if (r + 1 < NRD) {
            // the callback's buffer is the caller's again at the next callback, and the kernel runs after the last one: keep a copy
            uint64_t* keep = scratch.alloc_as<uint64_t>(bytes);
            if (!keep) return ctx->fail(NLX_E_NOMEM, "out of device memory");
            NLX_HIP(ctx, hipMemcpyAsync(keep, tr_ptr, bytes, hipMemcpyDefault, st));
            NLX_HIP(ctx, hipStreamSynchronize(st));
            d_tr = keep;
        } else {
            last_round.reset(new Staged(ctx, tr_ptr, bytes, true, false));
            NLX_RC(last_round->status);
            d_tr = last_round->as<uint64_t>();
        }
        if (n_rv) {
            ch.observe(rv, n_rv);
            values.insert(values.end(), rv, rv + n_rv);
        }
        for (uint32_t k = 0; k < s->round_challenges[r]; k++) {
            if (challenges && *challenges >= gl::P) return ctx->fail(NLX_E_RANGE, "a challenge of round %u is not canonical", r);
            values.push_back(challenges ? *challenges++ : ch.challenge());
        }
        for (uint32_t c = 0; c < rcols; c++) h_cols[col0 + c] = d_tr + (size_t)c * n;
        col0 += rcols;
    }

    uint64_t* d_pis = scratch.alloc_as<uint64_t>((values.size() + 1) * 8);
    const uint64_t** d_cols = scratch.alloc_as<const uint64_t*>((size_t)ncols * 8);
    unsigned long long* d_per = scratch.alloc_as<unsigned long long>((size_t)(N + 1) * 8);
    uint8_t* d_rows = scratch.alloc_as<uint8_t>(n);
    if (!d_pis || !d_cols || !d_per || !d_rows) return ctx->fail(NLX_E_NOMEM, "out of device memory");
    if (!values.empty()) NLX_HIP(ctx, hipMemcpyAsync(d_pis, values.data(), values.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_cols, h_cols.data(), (size_t)ncols * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(s->d_check, cc.block0, sizeof cc.block0, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemsetAsync(d_per, 0, (size_t)(N + 1) * 8, st));
    NLX_HIP(ctx, hipMemsetAsync(d_rows, 0, n, st));
    AirCheckParams ap{};
    ap.cols = d_cols; ap.program = s->d_program; ap.pis = d_pis; ap.periodic = s->d_periodic_rows;
    ap.seg = s->d_seg; ap.seg_first = s->d_seg_first;
    ap.block = (unsigned long long*)s->d_check; ap.per_constraint = d_per; ap.row_bad = d_rows;
    ap.log_n = log_n; ap.period_bits = d.period_bits; ap.n_pis = d.num_public_inputs;
    const uint32_t n_seg = (uint32_t)s->seg_after.size();
    unsigned bs = 64;
    while (bs > n) bs >>= 1;
    ctx->begin_kernel("air_check", 8.0 * n * 2.0 * ncols);
    // the launch groups of the quotient: segments of a similar register need share a launch (its LDS is the hungriest one's)
    for (size_t gi = 0; gi < s->seg_group.size(); gi++) {
        const uint32_t first = s->seg_group[gi], last = gi + 1 < s->seg_group.size() ? s->seg_group[gi + 1] : n_seg;
        AirCheckParams gp = ap;
        gp.seg = ap.seg + 2 * first;
        gp.seg_first = ap.seg_first + first;
        const size_t lds = (size_t)bs * s->seg_regs[last - 1] * 8;
        hipLaunchKernelGGL(k_air_check<false>, dim3((unsigned)(n / bs), last - first), dim3(bs), lds, st, gp);
    }
    hipLaunchKernelGGL(k_air_check_rows, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, st, d_rows, n,
                       ap.block + CHK_ROWS);
    ctx->end_kernel();
    uint64_t blk[CHK_WORDS];
    NLX_RC(fetch(ctx, blk, s->d_check, sizeof blk));
    if (per_constraint && N) NLX_RC(fetch(ctx, per_constraint, d_per, (size_t)N * 8));
    rep->rows_bad = blk[CHK_ROWS];
    rep->pairs_bad = blk[CHK_PAIRS];
    if (blk[CHK_FIRST] == ~0ull) {
        rep->satisfied = 1;
        return NLX_OK;
    }
    // the first finding's value and emitting word: that one row through that one segment again, on a single lane
    rep->row = (uint32_t)(blk[CHK_FIRST] >> 32);
    rep->constraint = (uint32_t)blk[CHK_FIRST];
    uint32_t sg = 0;
    for (uint32_t k = 0; k < n_seg; k++)
        if (s->seg_first[k] <= rep->constraint && rep->constraint < N - s->seg_after[k]) sg = k;
    AirCheckParams dp = ap;
    dp.seg = ap.seg + 2 * sg;
    dp.seg_first = ap.seg_first + sg;
    dp.row = rep->row;
    dp.target = rep->constraint;
    hipLaunchKernelGGL(k_air_check<true>, dim3(1, 1), dim3(1), (size_t)s->seg_regs[sg] * 8, st, dp);
    NLX_RC(fetch(ctx, blk, s->d_check, sizeof blk));
    rep->value = blk[CHK_VALUE];
    rep->word = (uint32_t)blk[CHK_WORD_KIND];
    rep->kind = (uint32_t)(blk[CHK_WORD_KIND] >> 32);
    rep->sub = (uint32_t)blk[CHK_SUB];
    // NLX_OK: the check ran.  The line is for nlx_last_error.
    ctx->fail(NLX_OK, "the trace breaks the AIR: row %u, constraint %u (%s, program word %u, sub %u) = %llu (0x%llx); %llu row(s) and %llu (row, constraint) pair(s) are not zero",
              rep->row, rep->constraint, emit_kind_name(rep->kind), rep->word, rep->sub, (unsigned long long)rep->value,
              (unsigned long long)rep->value, (unsigned long long)rep->rows_bad, (unsigned long long)rep->pairs_bad);
    return NLX_OK;
}

const uint64_t* single_round_fn(void* user, uint32_t round, const uint64_t*, uint32_t, uint64_t*) {
    return round == 0 ? (const uint64_t*)user : nullptr;
}

}  // namespace

extern "C" {

uint32_t nlx_stark_num_constraints(const nlx_stark* s) NLX_TRY { return s ? s->n_constraints : 0; } NLX_CATCH_VALUE(nullptr, 0)

int32_t nlx_stark_check_rounds(nlx_stark* s, nlx_round_fn round_fn, void* user, const uint64_t* public_inputs,
                               const uint64_t* challenges, nlx_trace_report* report, uint64_t* per_constraint) NLX_TRY {
    if (report) memset(report, 0, sizeof *report);
    if (!s) return NLX_E_INVAL;
    nlx_ctx* ctx = s->ctx;
    const nlx_stark_desc& d = s->d;
    if (!round_fn || !report || (!public_inputs && d.num_public_inputs)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (uint32_t i = 0; i < d.num_public_inputs; i++)
        if (public_inputs[i] >= gl::P) return ctx->fail(NLX_E_RANGE, "public input %u is not canonical", i);
    (void)hipSetDevice(ctx->device);
    CheckCall cc(ctx);
    return cc.scratch.finish(check_rounds(s, cc, round_fn, user, public_inputs, challenges, report, per_constraint));
} NLX_CATCH(s ? s->ctx : nullptr)

int32_t nlx_stark_check_trace(nlx_stark* s, const uint64_t* trace, const uint64_t* public_inputs, nlx_trace_report* report,
                              uint64_t* per_constraint) NLX_TRY {
    if (report) memset(report, 0, sizeof *report);
    if (!s) return NLX_E_INVAL;
    if (!trace || !report) return s->ctx->fail(NLX_E_INVAL, "NULL argument");
    if (s->n_rounds != 1 || s->n_round_challenges) return s->ctx->fail(NLX_E_INVAL, "a multi-round STARK is checked with nlx_stark_check_rounds");
    return nlx_stark_check_rounds(s, single_round_fn, (void*)trace, public_inputs, nullptr, report, per_constraint);
} NLX_CATCH(s ? s->ctx : nullptr)

}  // extern "C"
