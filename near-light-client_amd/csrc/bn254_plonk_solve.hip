// Row f.4, the PLONK half: gnark's witness solver on the device, by levels - the public and secret inputs
// of a setup's constraint system in, the whole variable vector out, which nlx_bn254_plonk_setup_wires turns into l r o.
//
// The rules are those of tools/gnark_plonk_solve_model.py, the place of record: RECALLED from gnark v0.9
// (constraint/bn254/solver.go, solveSparseR1C, the blueprints' levels), UNPINNED - parity with gnark's solver is not claimed.
// The schedule and the per-item arithmetic are bn254_plonk_solve.hpp's (plain g++ builds and tests them); here:
//   create                 the schedule on the host (every refusal before anything is allocated), the items uploaded in level
//                          order with their cells, and
//   k_pls_gather           a lane per item: its five selectors out of the setup's trace, so that a level reads coalesced;
//   k_pls_invert_const     every constant divisor (qo; ql / qr with qm = 0) inverted once: Montgomery's trick, one a^(r-2) per
//                          lane-run of INV_CHUNK divisors - a solve of such an item costs products only;
//   k_pls_init             per solve: the inputs into `values` (each checked below r), the rest 0, the state bytes;
//   k_pls_level            a lane per item of ONE level, any grid size: operands and state bytes in, solve or check, value and
//                          state byte out (0 unassigned, 1 assigned, 2 poisoned); failures joined per wave, then one atomicMin
//                          on the constraint index and one count;
//   k_pls_levels_fused     a run of consecutive levels of at most FUSE items each in ONE launch of ONE workgroup: plain stores,
//                          every wave waits for its stores, a workgroup barrier, plain loads.  No level hands data to another
//                          workgroup inside a kernel: wide levels are separated by kernel boundaries;
//   k_pls_commit_scatter   a commitment's hint, on the host between launches at its level: the committed variables onto their
//                          rows of an L scratch, nlx_bn254_plonk_commit, c_j into `values`.
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "bn254_fp.hpp"
#include "bn254_plonk_key.hpp"
#include "bn254_plonk_setup.hpp"
#include "bn254_plonk_solve.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

namespace nlx {
namespace plsolve {

using namespace bnf;

constexpr uint32_t FUSE = NLX_BN254_PLONK_SOLVER_FUSE;   // items per level a fused run takes: four per lane of its one workgroup
constexpr uint32_t INV_CHUNK = 32;                       // constant divisors per lane: one inversion among them
constexpr uint32_t INVERTED = 0x80;                      // bit of the form byte: the divisor's slot holds its inverse
enum { REP_MIN = 0, REP_FAILURES = 1, REP_POISONED = 2, REP_BAD_INPUT = 3, REP_WORDS = 4 };

struct SolveParams {
    const uint64_t* q;            // [5][n_items][4]
    const uint32_t* x;            // [3][n_items]
    const uint8_t* form;          // [n_items]
    const uint32_t* index;        // [n_items] the constraint, or the hint
    const uint64_t* hint_param;   // per hint
    const uint32_t* hint_out;     // the hints' output variables, concatenated
    const uint32_t* level_off;    // [levels + 1]
    uint32_t n_items;
    uint64_t* values;             // [n_variables][4]: written and read across levels, never through __restrict__
    uint8_t* state;               // [n_variables]
    uint32_t* report;             // [REP_WORDS]
};

__global__ __launch_bounds__(256) void k_pls_gather(const uint64_t* __restrict__ vals, uint32_t log_n, uint64_t n_public, SolveParams p, uint64_t* __restrict__ q) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_items) return;
    const bool constraint = (p.form[i] & 0x7f) <= SOLVE_O;
    const size_t row = n_public + p.index[i];   // below 2^log_n for a constraint: the setup holds n_public + n_constraints rows
#pragma unroll
    for (int s = 0; s < 5; s++) store(q, (size_t)s * p.n_items + i, constraint ? load<RP>(vals, ((size_t)s << log_n) + row) : zero<RP>());
}

__device__ __forceinline__ size_t divisor_slot(uint32_t form, size_t item, size_t n_items) {
    return (size_t)(form == SOLVE_O ? 3 : form == SOLVE_L ? 0 : 1) * n_items + item;
}
// list[e], e < count: the items whose divisor is a coefficient alone (never 0: a cell counts only where it is not)
__global__ __launch_bounds__(256) void k_pls_invert_const(uint64_t* q, const uint8_t* __restrict__ form, uint32_t n_items, const uint32_t* __restrict__ list, uint32_t count,
                                                          uint64_t* __restrict__ prefix) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lo = t * INV_CHUNK, hi = lo + INV_CHUNK < count ? lo + INV_CHUNK : count;
    if (lo >= count) return;
    Fr run = one<RP>();
#pragma unroll 1
    for (size_t e = lo; e < hi; e++) {
        const uint32_t item = list[e];
        store(prefix, e, run);
        run = mul(run, load<RP>(q, divisor_slot(form[item] & 0x7f, item, n_items)));
    }
    Fr inv = fr_inv(run);
#pragma unroll 1
    for (size_t e = hi; e-- > lo;) {
        const uint32_t item = list[e];
        const size_t slot = divisor_slot(form[item] & 0x7f, item, n_items);
        const Fr d = load<RP>(q, slot);
        store(q, slot, mul(inv, load<RP>(prefix, e)));
        inv = mul(inv, d);
    }
}

__global__ __launch_bounds__(256) void k_pls_init(const uint64_t* __restrict__ inputs, uint64_t n_given, uint64_t n_variables, uint64_t* __restrict__ values,
                                                  uint8_t* __restrict__ state, uint32_t* report) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_variables) return;
    const bool given = v < n_given;
    if (given && !below_mod<RP>(inputs + 4 * v)) atomicMin(&report[REP_BAD_INPUT], (uint32_t)v);
    store(values, v, given ? load<RP>(inputs, v) : zero<RP>());
    state[v] = given ? ASSIGNED : UNASSIGNED;
}

struct Tally {
    uint32_t fail_c, n_fail, n_poison;
};
__device__ __forceinline__ void put(const SolveParams& p, uint32_t v, uint8_t st, const Fr& value, Tally& t) {
    store(p.values, v, st == ASSIGNED ? value : zero<RP>());
    p.state[v] = st;
    t.n_poison += st == POISONED;
}

__device__ __forceinline__ void run_item(const SolveParams& p, size_t i, Tally& t) {
    const uint32_t fb = p.form[i], form = fb & 0x7f;
    const uint32_t x0 = p.x[i], x1 = p.x[(size_t)p.n_items + i], x2 = p.x[2 * (size_t)p.n_items + i];
    if (form == COMMIT) return;   // the host's, between launches
    if (form <= SOLVE_O) {
        Fr q[5];
#pragma unroll
        for (int s = 0; s < 5; s++) q[s] = load<RP>(p.q, (size_t)s * p.n_items + i);
        uint32_t ops = counting(nonzero_bits(q));   // an inverse is nonzero where its divisor was
        if (form != CHECK) ops &= ~(1u << (form - SOLVE_L));
        const uint8_t sl = (ops & CNT_L) ? p.state[x0] : (uint8_t)ASSIGNED, sr = (ops & CNT_R) ? p.state[x1] : (uint8_t)ASSIGNED,
                      so = (ops & CNT_O) ? p.state[x2] : (uint8_t)ASSIGNED;
        const Fr l = (ops & CNT_L) ? load<RP>(p.values, x0) : zero<RP>(), r = (ops & CNT_R) ? load<RP>(p.values, x1) : zero<RP>(),
                 o = (ops & CNT_O) ? load<RP>(p.values, x2) : zero<RP>();
        const bool poisoned = poisoned_operand(form, ops, sl, sr, so);
        Fr out = zero<RP>(), value;
        const uint32_t fail = poisoned ? (uint32_t)OK : solve_item(form, (fb & INVERTED) != 0, q, l, r, o, out, value);
        if (form != CHECK) put(p, form == SOLVE_L ? x0 : form == SOLVE_R ? x1 : x2, state_after(poisoned, fail), out, t);
        if (fail != OK) {
            t.n_fail++;
            const uint32_t c = p.index[i];
            t.fail_c = c < t.fail_c ? c : t.fail_c;
        }
        return;
    }
    // the arithmetic hints: x0 = the input, x1 = the first slot of hint_out, x2 = the outputs
    const uint8_t st = p.state[x0] == POISONED ? (uint8_t)POISONED : (uint8_t)ASSIGNED;
    const Fr x = load<RP>(p.values, x0);
    if (form == INV_ZERO) {
        put(p, p.hint_out[x1], st, st == ASSIGNED ? hint_inv_zero(x) : zero<RP>(), t);
    } else if (form == N_BITS) {
        const Fr c = from_mont(x);
#pragma unroll 1
        for (uint32_t b = 0; b < x2; b++) put(p, p.hint_out[x1 + b], st, hint_bit(c, b), t);
    } else {
        Fr quo = zero<RP>(), rem = zero<RP>();
        if (st == ASSIGNED) hint_quo_rem64(x, p.hint_param[p.index[i]], quo, rem);
        put(p, p.hint_out[x1], st, quo, t);
        put(p, p.hint_out[x1 + 1], st, rem, t);
    }
}

// every lane of the wave arrives: the lowest failing constraint and the two counts, then at most three atomics per wave
__device__ __forceinline__ void join(Tally t, uint32_t* report) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)t.fail_c, d, 64);
        t.fail_c = o < t.fail_c ? o : t.fail_c;
        t.n_fail += (uint32_t)__shfl_xor((int)t.n_fail, d, 64);
        t.n_poison += (uint32_t)__shfl_xor((int)t.n_poison, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (t.n_fail) {
            atomicMin(&report[REP_MIN], t.fail_c);
            atomicAdd(&report[REP_FAILURES], t.n_fail);
        }
        if (t.n_poison) atomicAdd(&report[REP_POISONED], t.n_poison);
    }
}

__global__ __launch_bounds__(256) void k_pls_level(SolveParams p, uint32_t first, uint32_t count) {
    Tally t{NONE, 0, 0};
#pragma unroll 1
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < count; base += (size_t)gridDim.x * blockDim.x)
        if (base + threadIdx.x < count) run_item(p, (size_t)first + base + threadIdx.x, t);
    join(t, p.report);
}

// levels first_level .. first_level + n_levels - 1, one workgroup (the launch is <<<1, 256>>>)
__global__ __launch_bounds__(256) void k_pls_levels_fused(SolveParams p, uint32_t first_level, uint32_t n_levels) {
    Tally t{NONE, 0, 0};
#pragma unroll 1
    for (uint32_t lv = first_level; lv < first_level + n_levels; lv++) {
        const uint32_t lo = p.level_off[lv - 1], hi = p.level_off[lv];
#pragma unroll 1
        for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) run_item(p, i, t);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores have left before it arrives
        __syncthreads();
    }
    join(t, p.report);
}

__global__ __launch_bounds__(256) void k_pls_commit_scatter(const uint32_t* __restrict__ vars, const uint32_t* __restrict__ rows, uint32_t count,
                                                            const uint64_t* __restrict__ values, const uint8_t* __restrict__ state, uint64_t* __restrict__ l,
                                                            uint32_t* __restrict__ poisoned) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = vars[i];
    if (state[v] == POISONED) atomicOr(poisoned, 1u);
    store(l, rows[i], load<RP>(values, v));
}

}  // namespace plsolve
}  // namespace nlx

using namespace nlx;
using plsolve::Fr;

struct Step {
    uint32_t kind;   // 0: one level, 1: a fused run, 2: a commitment's hint
    uint32_t a, b;   // level | first level, levels | commitment
};

struct nlx_bn254_plonk_solver {
    nlx_ctx* ctx = nullptr;
    uint32_t log_n = 0, k = 0;
    uint64_t n_variables = 0, n_given = 0, n_public = 0, n_constraints = 0;
    void* block = nullptr;
    size_t block_bytes = 0;
    plsolve::SolveParams p{};                         // values, state, report: per solve
    uint64_t* d_q = nullptr;
    std::vector<Step> steps;
    std::vector<uint32_t> level_off;
    std::vector<uint32_t> level, form, assigns;       // per constraint
    std::vector<uint32_t> item_of, x[3];              // per constraint: its item (NONE where skipped), its cells
    uint32_t commit_out[NLX_BN254_PLONK_MAX_COMMIT] = {}, commit_count[NLX_BN254_PLONK_MAX_COMMIT] = {}, commit_row[NLX_BN254_PLONK_MAX_COMMIT] = {};
    const uint32_t *d_commit_vars[NLX_BN254_PLONK_MAX_COMMIT] = {}, *d_commit_rows[NLX_BN254_PLONK_MAX_COMMIT] = {};
    uint64_t info[NLX_BN254_PLONK_SOLVER_INFO_WORDS] = {};
};
typedef struct nlx_bn254_plonk_solver PSolver;
typedef struct nlx_bn254_plonk_setup PSetup;   // the plain name is the entry point's

namespace {

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }
constexpr unsigned LEVEL_MAX_BLOCKS = 4096;   // a wider level strides

void solver_free(PSolver* s) {
    if (!s) return;
    if (s->ctx && s->block) {
        (void)hipStreamSynchronize(s->ctx->stream);
        s->ctx->release(s->block);
    }
    delete s;
}

// the descriptor's hints and the setup's commitments as one list in running order; every refusal of the descriptor itself
int32_t merged_hints(nlx_ctx* ctx, const PSetup& su, const nlx_bn254_plonk_solver_desc* d, std::vector<plsolve::Hint>& out) {
    const uint32_t nh = d->n_hints;
    if (nh && (!d->hint_kind || !d->hint_before || !d->hint_param || !d->hint_in_off || !d->hint_out_off || !d->hint_in || !d->hint_out))
        return ctx->fail(NLX_E_INVAL, "NULL argument (the hint arrays)");
    for (const void* ptr : {(const void*)d->hint_kind, (const void*)d->hint_before, (const void*)d->hint_param, (const void*)d->hint_in_off,
                            (const void*)d->hint_out_off, (const void*)d->hint_in, (const void*)d->hint_out})
        if (ptr && is_device_ptr(ptr)) return ctx->fail(NLX_E_INVAL, "the hint arrays are host arrays");
    // commitment j's hint: in front of its own constraint, after the listed hints of the same `before`
    std::vector<plsolve::Hint> commits;
    for (uint32_t j = 0; j < su.k; j++) {
        plsolve::Hint h;
        h.id = nh + j, h.kind = plsolve::COMMIT, h.before = su.commit_rows[j] - (uint32_t)su.n_public, h.param = j;
        size_t first = 0;
        for (uint32_t t = 0; t < j; t++) first += (size_t)su.counts[t];
        for (uint64_t i = 0; i < su.counts[j]; i++) h.in.push_back(su.x[0][su.committed_rows[first + i] - (uint32_t)su.n_public]);
        h.out.push_back(su.x[0][h.before]);
        commits.push_back(std::move(h));
    }
    std::stable_sort(commits.begin(), commits.end(), [](const plsolve::Hint& a, const plsolve::Hint& b) { return a.before < b.before; });
    size_t next_commit = 0;
    for (uint32_t i = 0; i < nh; i++) {
        plsolve::Hint h;
        h.id = i, h.kind = d->hint_kind[i], h.before = d->hint_before[i], h.param = d->hint_param[i];
        if (h.kind < plsolve::INV_ZERO || h.kind > plsolve::QUO_REM64) return ctx->fail(NLX_E_RANGE, "hint %u: unknown kind %u", i, h.kind);
        const uint64_t i0 = d->hint_in_off[i], i1 = d->hint_in_off[i + 1], o0 = d->hint_out_off[i], o1 = d->hint_out_off[i + 1];
        if (i1 < i0 || i1 - i0 > 1 || o1 < o0 || o1 - o0 > 256) return ctx->fail(NLX_E_RANGE, "hint %u: takes one input and gives at most 256 outputs", i);
        h.in.assign(d->hint_in + i0, d->hint_in + i1);
        h.out.assign(d->hint_out + o0, d->hint_out + o1);
        for (uint32_t v : h.in)
            if (v >= su.n_variables) return ctx->fail(NLX_E_RANGE, "hint %u: input variable %u of %llu", i, v, (unsigned long long)su.n_variables);
        for (uint32_t v : h.out)
            if (v >= su.n_variables) return ctx->fail(NLX_E_RANGE, "hint %u: output variable %u of %llu", i, v, (unsigned long long)su.n_variables);
        while (next_commit < commits.size() && commits[next_commit].before < h.before) out.push_back(std::move(commits[next_commit++]));
        out.push_back(std::move(h));
    }
    while (next_commit < commits.size()) out.push_back(std::move(commits[next_commit++]));
    return NLX_OK;
}

// the launches of one solve: commitments' hints in front of their level, runs of narrow levels fused
void plan(const plsolve::Schedule& sc, bool fuse, PSolver& s) {
    std::vector<std::vector<uint32_t>> commits_at(sc.levels + 2);
    for (const plsolve::Item& it : sc.items)
        if (it.form == plsolve::COMMIT) commits_at[it.level].push_back(it.x[0]);
    auto width = [&](uint32_t lv) { return (uint32_t)(sc.level_off[lv] - sc.level_off[lv - 1]); };
    uint64_t launches = 0, runs = 0;
    for (uint32_t lv = 1; lv <= sc.levels;) {
        for (uint32_t j : commits_at[lv]) s.steps.push_back({2, j, 0});
        uint32_t n = 1;
        if (fuse && width(lv) <= plsolve::FUSE)
            while (lv + n <= sc.levels && width(lv + n) <= plsolve::FUSE && commits_at[lv + n].empty()) n++;
        if (n > 1) {
            s.steps.push_back({1, lv, n});
            launches++, runs++;
        } else if (width(lv) > commits_at[lv].size()) {   // a level of commitments alone launches nothing
            s.steps.push_back({0, lv, 0});
            launches++;
        }
        lv += n;
    }
    s.info[2] = launches, s.info[3] = runs;
}

template <class T>
T* carve(uint8_t*& at, size_t count) {
    T* p = reinterpret_cast<T*>(at);
    at += (count * sizeof(T) + 255) / 256 * 256;
    return p;
}

int32_t create_body(nlx_ctx* ctx, Scratch& scratch, const PSetup& su, const plsolve::Schedule& sc, const std::vector<plsolve::Hint>& hints, PSolver& s) {
    using namespace plsolve;
    const size_t ni = sc.items.size(), nh = hints.size(), no = sc.hint_out.size();
    size_t n_committed = 0;
    for (uint32_t j = 0; j < s.k; j++) n_committed += (size_t)su.counts[j];
    auto padded = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    s.block_bytes = padded(5 * ni * 32) + 3 * padded(ni * 4) + padded(ni) + padded(ni * 4) + padded(nh * 8) + padded(no * 4) + padded((sc.levels + 1) * 4) +
                    2 * (size_t)s.k * 256 + 2 * padded(n_committed * 4) + padded(REP_WORDS * 4) + 256;
    s.block = ctx->alloc(s.block_bytes);
    if (!s.block) return ctx->fail(NLX_E_NOMEM, "PLONK solver: device memory for %zu items", ni);
    uint8_t* at = (uint8_t*)s.block;
    s.d_q = carve<uint64_t>(at, 5 * ni * 4);
    uint32_t* d_x = carve<uint32_t>(at, 3 * ni);
    uint8_t* d_form = carve<uint8_t>(at, ni);
    uint32_t* d_index = carve<uint32_t>(at, ni);
    uint64_t* d_param = carve<uint64_t>(at, nh);
    uint32_t* d_out = carve<uint32_t>(at, no);
    uint32_t* d_off = carve<uint32_t>(at, sc.levels + 1);
    uint32_t* d_report = carve<uint32_t>(at, REP_WORDS);

    std::vector<uint32_t> hx(3 * ni), hindex(ni), cd_list;
    std::vector<uint8_t> hform(ni);
    std::vector<uint64_t> hparam(nh);
    s.item_of.assign((size_t)s.n_constraints, NONE);
    for (size_t i = 0; i < ni; i++) {
        const Item& it = sc.items[i];
        for (int c = 0; c < 3; c++) hx[c * ni + i] = it.x[c];
        hindex[i] = it.index;
        hform[i] = (uint8_t)(it.form | (it.const_div ? INVERTED : 0));
        if (it.const_div) cd_list.push_back((uint32_t)i);
        if (it.form <= SOLVE_O) s.item_of[it.index] = (uint32_t)i;
        s.info[4 + it.form]++;
        if (it.form >= SOLVE_L && it.form <= SOLVE_O) s.info[it.const_div ? 12 : 13]++;
    }
    for (size_t h = 0; h < nh; h++) hparam[h] = hints[h].param;
    s.level_off.resize(sc.levels + 1);
    for (uint32_t v = 0; v <= sc.levels; v++) s.level_off[v] = (uint32_t)sc.level_off[v];
    hipStream_t st = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    NLX_HIP(ctx, up(d_x, hx.data(), 3 * ni * 4));
    NLX_HIP(ctx, up(d_form, hform.data(), ni));
    NLX_HIP(ctx, up(d_index, hindex.data(), ni * 4));
    NLX_HIP(ctx, up(d_param, hparam.data(), nh * 8));
    NLX_HIP(ctx, up(d_out, sc.hint_out.data(), no * 4));
    NLX_HIP(ctx, up(d_off, s.level_off.data(), s.level_off.size() * 4));
    std::vector<uint32_t> cvars, crows;
    size_t first = 0;
    for (uint32_t j = 0; j < s.k; j++) {
        const size_t count = (size_t)su.counts[j];
        uint32_t* dv = carve<uint32_t>(at, count);
        uint32_t* dr = carve<uint32_t>(at, count);
        s.d_commit_vars[j] = dv, s.d_commit_rows[j] = dr;
        s.commit_count[j] = (uint32_t)count;
        s.commit_row[j] = su.commit_rows[j];
        s.commit_out[j] = su.x[0][su.commit_rows[j] - (uint32_t)su.n_public];
        cvars.clear(), crows.clear();
        for (size_t i = 0; i < count; i++) {
            crows.push_back(su.committed_rows[first + i]);
            cvars.push_back(su.x[0][su.committed_rows[first + i] - (uint32_t)su.n_public]);
        }
        first += count;
        NLX_HIP(ctx, hipMemcpy(dv, cvars.data(), count * 4, hipMemcpyHostToDevice));   // the vectors are reused: not queued
        NLX_HIP(ctx, hipMemcpy(dr, crows.data(), count * 4, hipMemcpyHostToDevice));
    }
    if ((size_t)(at - (uint8_t*)s.block) > s.block_bytes) return ctx->fail(NLX_E_INVAL, "PLONK solver: the block's layout exceeds its size");
    s.p.q = s.d_q, s.p.x = d_x, s.p.form = d_form, s.p.index = d_index, s.p.hint_param = d_param, s.p.hint_out = d_out, s.p.level_off = d_off;
    s.p.n_items = (uint32_t)ni, s.p.report = d_report;
    if (ni) {
        hipLaunchKernelGGL(k_pls_gather, dim3(blocks_of(ni)), dim3(256), 0, st, su.vals, su.log_n, su.n_public, s.p, s.d_q);
        if (!cd_list.empty()) {
            uint32_t* d_list = scratch.alloc_as<uint32_t>(cd_list.size() * 4);
            uint64_t* d_prefix = scratch.alloc_as<uint64_t>(cd_list.size() * 32);
            if (!d_list || !d_prefix) return ctx->fail(NLX_E_NOMEM, "PLONK solver: device memory");
            NLX_HIP(ctx, up(d_list, cd_list.data(), cd_list.size() * 4));
            const size_t lanes = (cd_list.size() + INV_CHUNK - 1) / INV_CHUNK;
            hipLaunchKernelGGL(k_pls_invert_const, dim3(blocks_of(lanes)), dim3(256), 0, st, s.d_q, d_form, (uint32_t)ni, d_list, (uint32_t)cd_list.size(), d_prefix);
        }
    }
    NLX_HIP(ctx, hipStreamSynchronize(st));   // the host vectors above were read
    NLX_HIP(ctx, hipGetLastError());
    uint64_t widest = 0;
    for (uint32_t v = 1; v <= sc.levels; v++) widest = std::max<uint64_t>(widest, sc.level_off[v] - sc.level_off[v - 1]);
    s.info[0] = sc.levels, s.info[1] = widest, s.info[14] = sc.unassigned, s.info[15] = s.block_bytes;
    return NLX_OK;
}

int32_t solve_body(nlx_ctx* ctx, Scratch& scratch, const PSolver& s, const uint64_t* inputs, const nlx_bn254_plonk_key* key, const uint64_t* commit_blinding,
                   uint64_t* values_out, uint64_t* commit_points_out, nlx_bn254_plonk_solve_report* report) {
    using namespace plsolve;
    hipStream_t st = ctx->stream;
    const size_t nv = (size_t)s.n_variables, n = (size_t)1 << s.log_n;
    Staged sin(ctx, inputs, (size_t)s.n_given * 32, true, false);
    if (sin.status) return sin.status;
    uint64_t* d_values = scratch.alloc_as<uint64_t>(nv * 32);
    uint8_t* d_state = scratch.alloc_as<uint8_t>(nv + 16);
    uint64_t* d_l = s.k ? scratch.alloc_as<uint64_t>(n * 32) : nullptr;
    uint32_t* d_flag = scratch.alloc_as<uint32_t>(16);
    if (!d_values || !d_state || (s.k && !d_l) || !d_flag) return ctx->fail(NLX_E_NOMEM, "PLONK solve: device memory for %zu variables", nv);
    SolveParams p = s.p;
    p.values = d_values, p.state = d_state;
    static const uint32_t fresh[REP_WORDS] = {NONE, 0, 0, NONE};
    NLX_HIP(ctx, hipMemcpyAsync(p.report, fresh, sizeof fresh, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pls_init, dim3(blocks_of(nv)), dim3(256), 0, st, sin.as<uint64_t>(), s.n_given, s.n_variables, d_values, d_state, p.report);
    std::vector<uint64_t> cs((size_t)4 * s.k + 4), points((size_t)8 * s.k + 8);   // read by queued copies: they outlive the last synchronise
    uint64_t host_poisoned = 0;
    uint32_t launches = 0;
    for (const Step& step : s.steps) {
        if (step.kind == 0) {
            const uint32_t first = s.level_off[step.a - 1], count = s.level_off[step.a] - first;
            const unsigned blocks = blocks_of(count) < LEVEL_MAX_BLOCKS ? blocks_of(count) : LEVEL_MAX_BLOCKS;
            ctx->begin_kernel("bn254_plonk_solve_levels", 200.0 * count, (double)count);
            hipLaunchKernelGGL(k_pls_level, dim3(blocks), dim3(256), 0, st, p, first, count);
            ctx->end_kernel();
            launches++;
        } else if (step.kind == 1) {
            const double items = (double)(s.level_off[step.a + step.b - 1] - s.level_off[step.a - 1]);
            ctx->begin_kernel("bn254_plonk_solve_fused", 200.0 * items, items);
            hipLaunchKernelGGL(k_pls_levels_fused, dim3(1), dim3(256), 0, st, p, step.a, step.b);
            ctx->end_kernel();
            launches++;
        } else {
            const uint32_t j = step.a, count = s.commit_count[j];
            NLX_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, st));
            if (count) {
                ctx->begin_kernel("bn254_plonk_solve_commit", 72.0 * count, (double)count);
                hipLaunchKernelGGL(k_pls_commit_scatter, dim3(blocks_of(count)), dim3(256), 0, st, s.d_commit_vars[j], s.d_commit_rows[j], count, d_values, d_state, d_l,
                                   d_flag);
                ctx->end_kernel();
            }
            uint32_t poisoned = 0;
            NLX_RC(fetch(ctx, &poisoned, d_flag, 4));
            if (poisoned) {   // skipped: its output is poisoned (the value stays 0)
                NLX_HIP(ctx, hipMemsetAsync(d_state + s.commit_out[j], POISONED, 1, st));
                host_poisoned++;
                continue;
            }
            NLX_RC(nlx_bn254_plonk_commit(ctx, key, j, d_l, commit_blinding + 8 * (size_t)j, &points[8 * (size_t)j], &cs[4 * (size_t)j]));
            NLX_HIP(ctx, hipMemcpyAsync(d_values + 4 * (size_t)s.commit_out[j], &cs[4 * (size_t)j], 32, hipMemcpyHostToDevice, st));
            NLX_HIP(ctx, hipMemsetAsync(d_state + s.commit_out[j], ASSIGNED, 1, st));
        }
    }
    uint32_t rep[REP_WORDS];
    NLX_RC(fetch(ctx, rep, p.report, sizeof rep));
    NLX_HIP(ctx, hipGetLastError());
    if (rep[REP_BAD_INPUT] != NONE) return ctx->fail(NLX_E_RANGE, "input %u is not below r", rep[REP_BAD_INPUT]);
    report->failures = rep[REP_FAILURES];
    report->poisoned_variables = rep[REP_POISONED] + host_poisoned;
    report->levels_run = (uint32_t)s.info[0], report->launches = launches;
    report->solved = rep[REP_FAILURES] == 0;
    if (!report->solved) {
        // the failing constraint of lowest index: its operands are clean and final, so the header's arithmetic gives its kind and
        // value again on the host (a failing item's divisor is never an inverted one: those cannot be 0)
        const uint32_t c = rep[REP_MIN];
        if (c >= s.n_constraints || s.item_of[c] == NONE) return ctx->fail(NLX_E_HIP, "PLONK solve: the report names constraint %u", c);
        const size_t item = s.item_of[c];
        uint64_t w[8][4];
        for (int i = 0; i < 5; i++) NLX_RC(fetch(ctx, w[i], s.d_q + 4 * ((size_t)i * s.p.n_items + item), 32));
        for (int i = 0; i < 3; i++) NLX_RC(fetch(ctx, w[5 + i], d_values + 4 * (size_t)s.x[i][c], 32));
        Fr q[5], op[3], out, value;
        for (int i = 0; i < 5; i++) q[i] = bnf::load_words<bnf::RP>(w[i]);
        uint32_t ops = counting(nonzero_bits(q));
        if (s.form[c] != CHECK) ops &= ~(1u << (s.form[c] - SOLVE_L));
        for (int i = 0; i < 3; i++) op[i] = (ops >> i & 1) ? bnf::load_words<bnf::RP>(w[5 + i]) : bnf::zero<bnf::RP>();
        report->kind = solve_item(s.form[c], false, q, op[0], op[1], op[2], out, value);
        report->constraint = c, report->level = s.level[c];
        bnf::store_words(bnf::from_mont(value), report->value);
        (void)ctx->fail(NLX_OK, "PLONK solve: constraint %u (level %u) %s, %s 0x%016llx%016llx%016llx%016llx; %llu constraints failed, %llu variables poisoned", c,
                        s.level[c], report->kind == DIV_ZERO ? "divides by zero" : "is not satisfied", report->kind == DIV_ZERO ? "numerator" : "value",
                        (unsigned long long)report->value[3], (unsigned long long)report->value[2], (unsigned long long)report->value[1],
                        (unsigned long long)report->value[0], (unsigned long long)report->failures, (unsigned long long)report->poisoned_variables);
    }
    NLX_HIP(ctx, hipMemcpyAsync(values_out, d_values, nv * 32, hipMemcpyDefault, st));
    NLX_HIP(ctx, hipStreamSynchronize(st));
    if (commit_points_out && s.k) memcpy(commit_points_out, points.data(), (size_t)64 * s.k);
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_plonk_solver_create(nlx_ctx* ctx, const struct nlx_bn254_plonk_setup* setup, const nlx_bn254_plonk_solver_desc* desc,
                                                 struct nlx_bn254_plonk_solver** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!setup || !desc || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    if (setup->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the setup belongs to another context");
    if ((desc->flags & ~(uint32_t)NLX_BN254_PLONK_SOLVER_NO_FUSE) != NLX_BN254_MONTGOMERY)
        return ctx->fail(NLX_E_RANGE, "flags: NLX_BN254_MONTGOMERY, optionally | NLX_BN254_PLONK_SOLVER_NO_FUSE");
    const PSetup& su = *setup;
    if (desc->n_secret > su.n_variables || su.n_public + desc->n_secret > su.n_variables)
        return ctx->fail(NLX_E_RANGE, "n_public + n_secret = %llu + %llu inputs exceed the %llu variables", (unsigned long long)su.n_public,
                         (unsigned long long)desc->n_secret, (unsigned long long)su.n_variables);
    (void)hipSetDevice(ctx->device);
    std::vector<plsolve::Hint> hints;
    NLX_RC(merged_hints(ctx, su, desc, hints));
    std::vector<uint8_t> skipped((size_t)su.n_constraints, 0);
    for (uint32_t r : su.committed_rows) skipped[r - (size_t)su.n_public] = 1;
    for (uint32_t r : su.commit_rows) skipped[r - (size_t)su.n_public] = 1;
    const uint32_t* cells[3] = {su.x[0].data(), su.x[1].data(), su.x[2].data()};
    plsolve::Schedule sc;
    std::string err;
    if (!plsolve::make_schedule(su.n_variables, su.n_public + desc->n_secret, su.n_constraints, cells, su.nonzero.data(), skipped.data(), hints, sc, err))
        return ctx->fail(NLX_E_INVAL, "PLONK solver: %s", err.c_str());   // nothing of the device is held yet
    std::unique_ptr<PSolver, void (*)(PSolver*)> s(new PSolver, solver_free);
    s->ctx = ctx, s->log_n = su.log_n, s->k = su.k;
    s->n_variables = su.n_variables, s->n_public = su.n_public, s->n_given = su.n_public + desc->n_secret, s->n_constraints = su.n_constraints;
    s->level = sc.level, s->form = sc.form, s->assigns = sc.assigns;
    for (int i = 0; i < 3; i++) s->x[i] = su.x[i];
    plan(sc, !(desc->flags & NLX_BN254_PLONK_SOLVER_NO_FUSE), *s);
    int32_t rc;
    {
        Scratch scratch(ctx);
        rc = scratch.finish(create_body(ctx, scratch, su, sc, hints, *s));
    }
    if (rc) return rc;
    *out = s.release();
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_plonk_solver_destroy(struct nlx_bn254_plonk_solver* solver) NLX_TRY {
    solver_free(solver);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_plonk_solver_info(const struct nlx_bn254_plonk_solver* solver, uint64_t out[NLX_BN254_PLONK_SOLVER_INFO_WORDS]) NLX_TRY {
    if (!solver || !out) return NLX_E_INVAL;
    memcpy(out, solver->info, sizeof solver->info);
    return NLX_OK;
} NLX_CATCH(nullptr)

extern "C" int32_t nlx_bn254_plonk_solver_read(const struct nlx_bn254_plonk_solver* solver, uint32_t which, void* out) NLX_TRY {
    if (!solver) return NLX_E_INVAL;
    nlx_ctx* ctx = solver->ctx;
    const std::vector<uint32_t>* src = which == NLX_PLONK_SOLVER_LEVEL ? &solver->level : which == NLX_PLONK_SOLVER_FORM ? &solver->form
                                       : which == NLX_PLONK_SOLVER_ASSIGNS ? &solver->assigns : nullptr;
    if (!src) return ctx->fail(NLX_E_RANGE, "unknown array %u", which);
    if (!out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (!src->empty()) memcpy(out, src->data(), src->size() * 4);
    return NLX_OK;
} NLX_CATCH(solver ? solver->ctx : nullptr)

extern "C" int32_t nlx_bn254_plonk_solver_solve(nlx_ctx* ctx, const struct nlx_bn254_plonk_solver* solver, const uint64_t* inputs,
                                                const nlx_bn254_plonk_key* key, const uint64_t* commit_blinding, uint64_t* values_out,
                                                uint64_t* commit_points_out, nlx_bn254_plonk_solve_report* report) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!solver || !values_out || !report) return ctx->fail(NLX_E_INVAL, "NULL argument");
    memset(report, 0, sizeof *report);
    const PSolver& s = *solver;
    if (s.ctx != ctx) return ctx->fail(NLX_E_INVAL, "the solver belongs to another context");
    if (s.n_given && !inputs) return ctx->fail(NLX_E_INVAL, "NULL argument (inputs)");
    if ((s.k > 0) != (key != nullptr)) return ctx->fail(NLX_E_INVAL, "a key is required exactly when the setup carries commitments (k = %u)", s.k);
    if ((s.k > 0) != (commit_blinding != nullptr)) return ctx->fail(NLX_E_INVAL, "commit_blinding: 2 k scalars, NULL exactly when k = 0 (k = %u)", s.k);
    if (key) {
        if (key->ctx != ctx) return ctx->fail(NLX_E_INVAL, "the key belongs to another context");
        if (key->log_n != s.log_n || key->n_commit != s.k) return ctx->fail(NLX_E_INVAL, "the key (2^%u rows, k = %u) is not this setup's (2^%u rows, k = %u)", key->log_n, key->n_commit, s.log_n, s.k);
        for (uint32_t j = 0; j < s.k; j++)
            if (key->commit_rows[j] != s.commit_row[j] || key->seg[j + 1] - key->seg[j] != s.commit_count[j])
                return ctx->fail(NLX_E_INVAL, "the key's commitment %u is not this setup's", j);
        if (is_device_ptr(commit_blinding) || (commit_points_out && is_device_ptr(commit_points_out))) return ctx->fail(NLX_E_INVAL, "commit_blinding and commit_points_out are host arrays");
    }
    (void)hipSetDevice(ctx->device);
    Scratch scratch(ctx);
    return scratch.finish(solve_body(ctx, scratch, s, inputs, key, commit_blinding, values_out, commit_points_out, report));
} NLX_CATCH(ctx)
