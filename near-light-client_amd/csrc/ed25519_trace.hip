// Trace generation for the Ed25519 verification AIR (near-light-client_amd/ed25519_air.py; SURVEY.md §8a row a12 /
// §8f.1: curta_eddsa_verify_sigs_conditional, nearx/src/builder.rs:152).  Two kernels over the row code of
// ed25519_rows.hpp:
//   k_ed_scan4 four lanes per slot walk its 256 rows (the point after each row depends on the one before) and
//              record the input point of every row - the only sequential part, on values only (fe25519_fast.hpp:
//              26-bit limbs, no witness cells; canonical results, so identical to what the row emitter recomputes);
//   k_ed_rows  one lane per row recomputes its 16 units from that input point (results are canonical, so the
//              recomputation is bit-identical) and writes its 1 488 cells; a wave's 64 lanes are 64 consecutive rows,
//              so every column store is 512 contiguous bytes.
#include "bind_round.hpp"
#include "ctx.hpp"
#include "ed25519_rows.hpp"
#include "gl.hpp"
#include "transcript.hpp"
#include <vector>

namespace nlx {

static_assert(ed::N_COLS0 == NLX_ED25519_COLS0, "column map");

// ---- the scan on FOUR lanes per slot ------------------------------------------------------------------------------------
// A row of the double-and-add chain is fifteen field products in four dependent levels (4 squares; 4 products of the
// doubling; 4 products with the addend; 3 products of the addition).  Walked one after the other on one lane per slot (ed::fast_row,
// the form the host runs) that is 128 lanes for the Sync step's 128 slots and 3.7 ms of latency.  Here a quad of lanes owns a slot: lane j computes
// product j of every level (operands picked by lane-index selects, no divergent control flow), the four results travel by
// DPP quad broadcasts (ten 26-bit limbs each), and lanes 0..2 canonicalise and store one coordinate of the row's input point
// each.  The state is replicated in the quad; values are the same residues as ed::fast_row's (canonical after freeze), so the
// trace is bit-identical.
namespace quad {
struct F10 { int32_t l[10]; };   // fe::Fe's limbs after a carry fit 32 bits (|l_0| <= 2^25 + 608, |l_i| <= 2^25: fe::carry10)

template <int SRC>
__device__ __forceinline__ F10 bcast(const F10& v) {   // lane SRC of the quad's value, in every lane of the quad
    F10 r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = __builtin_amdgcn_mov_dpp(v.l[i], SRC * 0x55, 0xF, 0xF, true);
    return r;
}
__device__ __forceinline__ F10 pick(uint32_t j, const F10& a, const F10& b, const F10& c, const F10& d) {
    F10 r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = j == 0 ? a.l[i] : (j == 1 ? b.l[i] : (j == 2 ? c.l[i] : d.l[i]));
    return r;
}
__device__ __forceinline__ F10 add(const F10& a, const F10& b) { F10 r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = a.l[i] + b.l[i]; return r; }
__device__ __forceinline__ F10 sub(const F10& a, const F10& b) { F10 r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = a.l[i] - b.l[i]; return r; }
__device__ __forceinline__ fe::Fe wide(const F10& a) { fe::Fe r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = a.l[i]; return r; }
__device__ __forceinline__ F10 narrow(const fe::Fe& a) { F10 r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.l[i] = (int32_t)a.l[i]; return r; }
// operands: sums of at most four carried values (|l| <= 2^27 + 2432 < 2^28, fe::mul's bound); result carried
__device__ __forceinline__ F10 mul(const F10& a, const F10& b) { return narrow(fe::mul(wide(a), wide(b))); }
}  // namespace quad

// ---- the scan's arithmetic at given values (self-test entry nlx_fe25519_ops): one lane per element, launched in whole quads - the
// DPP moves need all four lanes, so no lane returns before them; lanes past n compute element n - 1 and store nothing, as
// k_ed_scan4's spare quads do.  Per element: freeze(a) | freeze(a b) | a b's ten carried limbs | freeze of the NEXT lane's product,
// fetched the way the scan moves values (quad::mul, the four broadcasts, quad::pick). ----
constexpr uint32_t FE_OPS_WORDS = NLX_FE25519_OPS_WORDS;
static_assert(FE_OPS_WORDS == 16 + 16 + 10 + 16, "output layout");
__global__ __launch_bounds__(64) void k_fe25519_ops(const int32_t* __restrict__ a, const int32_t* __restrict__ b, size_t n,
                                                    uint32_t* __restrict__ out) {
    using quad::F10;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = t < n;
    const size_t e = live ? t : n - 1;
    const uint32_t j = threadIdx.x & 3;
    F10 x, y;
#pragma unroll
    for (int i = 0; i < 10; i++) { x.l[i] = a[e * 10 + i]; y.l[i] = b[e * 10 + i]; }
    const fe::Fe prod = fe::mul(quad::wide(x), quad::wide(y));
    const F10 m = quad::mul(x, y);
    const F10 next = quad::pick((j + 1) & 3, quad::bcast<0>(m), quad::bcast<1>(m), quad::bcast<2>(m), quad::bcast<3>(m));
    if (!live) return;
    uint32_t* o = out + e * FE_OPS_WORDS;
    uint32_t c16[16];
    fe::freeze(quad::wide(x), c16);
#pragma unroll
    for (int i = 0; i < 16; i++) o[i] = c16[i];
    fe::freeze(prod, c16);
#pragma unroll
    for (int i = 0; i < 16; i++) o[16 + i] = c16[i];
#pragma unroll
    for (int i = 0; i < 10; i++) o[32 + i] = (uint32_t)(int32_t)prod.l[i];
    fe::freeze(quad::wide(next), c16);
#pragma unroll
    for (int i = 0; i < 16; i++) o[42 + i] = c16[i];
}

constexpr uint32_t SCAN4_SLOTS_PER_BLOCK = 16;   // 64 lanes
__global__ __launch_bounds__(64) void k_ed_scan4(const uint64_t* __restrict__ words, uint32_t n_slots, ed::Slot* __restrict__ slots,
                                                 ed::Point* __restrict__ in, ed::Point* __restrict__ fin) {
    using quad::F10;
    __shared__ int32_t tab[64][4][10];   // this lane's column of the slot's addend table: [sel][limb]
    const uint32_t k_raw = blockIdx.x * SCAN4_SLOTS_PER_BLOCK + (threadIdx.x >> 2), j = threadIdx.x & 3;
    const bool live = k_raw < n_slots;               // spare quads redo the last slot and store nothing (whole quads: DPP needs its lanes)
    const uint32_t k = live ? k_raw : n_slots - 1;
    ed::Slot s;
    ed::slot_from_words(words + (size_t)k * ed::SLOT_WORDS, s);
    if (live && j == 0) slots[k] = s;
    {
        ed::FastSlot fs;
        ed::fast_slot(s, fs);
        for (int sel = 0; sel < 4; sel++) {
            const fe::Fe& v = j == 0 ? fs.ymx[sel] : (j == 1 ? fs.ypx[sel] : (j == 2 ? fs.t2d[sel] : fs.z2[sel]));
            for (int i = 0; i < 10; i++) tab[threadIdx.x][sel][i] = (int32_t)v.l[i];
        }
    }
    F10 x, y, z;
#pragma unroll
    for (int i = 0; i < 10; i++) { x.l[i] = 0; y.l[i] = i == 0; z.l[i] = i == 0; }
    uint32_t* out_words = reinterpret_cast<uint32_t*>(in + (size_t)k * ed::ROWS) + 16 * j;   // coordinate j of the slot's first row
#pragma unroll 1
    for (int r = 0; r <= ed::ROWS; r++) {
        // the row's input point (after the last row: the slot's final point): lanes 0..2 freeze and store one coordinate each
        if (live && j < 3) {
            uint32_t c16[16];
            fe::freeze(quad::wide(quad::pick(j, x, y, z, z)), c16);
            uint32_t* dst = r < ed::ROWS ? out_words + (size_t)r * 48 : reinterpret_cast<uint32_t*>(fin + k) + 16 * j;
#pragma unroll
            for (int i = 0; i < 16; i += 4) *reinterpret_cast<uint4*>(dst + i) = make_uint4(c16[i], c16[i + 1], c16[i + 2], c16[i + 3]);
        }
        if (r == ed::ROWS) break;
        const int bit = ed::ROWS - 1 - r;
        const uint32_t sel = ((s.sw[bit >> 4] >> (bit & 15)) & 1) + 2 * ((s.hw[bit >> 4] >> (bit & 15)) & 1);
        // level 1: a = x^2, b = y^2, zz = z^2, e1 = (x + y)^2
        const F10 sq_in = quad::pick(j, x, y, z, quad::add(x, y));
        const F10 sq = quad::mul(sq_in, sq_in);
        const F10 a = quad::bcast<0>(sq), b = quad::bcast<1>(sq), zz = quad::bcast<2>(sq), e1 = quad::bcast<3>(sq);
        const F10 e = quad::sub(quad::sub(e1, a), b), g = quad::sub(b, a), f = quad::sub(g, quad::add(zz, zz)), h = quad::sub(quad::sub(g, b), b);   // h = -(a + b)
        // level 2: x2 = e f, y2 = g h, t2 = e h, z2 = f g
        const F10 m2 = quad::mul(quad::pick(j, e, g, e, f), quad::pick(j, f, h, h, g));
        const F10 x2 = quad::bcast<0>(m2), y2 = quad::bcast<1>(m2);
        // level 3: the addend (its four products with the doubled point), sel = 0 being the neutral element's (1, 1, 0, 2)
        F10 t;
#pragma unroll
        for (int i = 0; i < 10; i++) t.l[i] = tab[threadIdx.x][sel][i];
        const F10 m3 = quad::mul(quad::pick(j, quad::sub(y2, x2), quad::add(y2, x2), m2, m2), t);
        const F10 pa = quad::bcast<0>(m3), pb = quad::bcast<1>(m3), pc = quad::bcast<2>(m3), pd = quad::bcast<3>(m3);
        const F10 e_ = quad::sub(pb, pa), f_ = quad::sub(pd, pc), g_ = quad::add(pd, pc), h_ = quad::add(pb, pa);
        // level 4: x = e_ f_, y = g_ h_, z = f_ g_ (lane 3 repeats z)
        const F10 m4 = quad::mul(quad::pick(j, e_, g_, f_, f_), quad::pick(j, f_, h_, g_, g_));
        x = quad::bcast<0>(m4);
        y = quad::bcast<1>(m4);
        z = quad::bcast<2>(m4);
    }
}

struct TracePut {
    uint64_t* trace;
    size_t n, row;
    __device__ __forceinline__ void operator()(uint32_t col, uint64_t v) { trace[(size_t)col * n + row] = v; }
};

__global__ __launch_bounds__(64) void k_ed_rows(const ed::Slot* __restrict__ slots, const ed::Point* __restrict__ in,
                                                const ed::Point* __restrict__ fin, uint32_t n_slots, uint64_t* __restrict__ trace,
                                                uint32_t* __restrict__ bad_slot) {
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)n_slots * ed::ROWS;
    if (row >= n) return;
    const uint32_t k = (uint32_t)(row / ed::ROWS), prev = k ? k - 1 : n_slots - 1;
    const int r = (int)(row % ed::ROWS);
    const ed::Slot s = slots[k];
    const ed::Point p = in[row];
    ed::Point prev_fin;
    uint32_t prev_ry[16];
    bool prev_active = true;
    if (r == ed::STEP_YCMP) {
        prev_fin = fin[prev];
        for (int i = 0; i < 16; i++) prev_ry[i] = slots[prev].ry[i];
        prev_active = slots[prev].active != 0;
    }
    TracePut put{trace, n, row};
    ed::Point o;
    // row 0 checks the previous slot's Y comparison
    if (!ed::emit_row(r, s, p, prev_ry, &prev_fin, prev_active, put, o)) atomicMin(bad_slot, r == ed::STEP_YCMP ? prev : k);
    if (r == 1 && !s.s_in_range) atomicMin(bad_slot, k);   // S >= L: the comparison rows have no witness
}

// ---- binding accumulator (round 1): Horner fingerprint in F_p^2 of every slot's limbs, limb 15 first, in the order
// enc(A), enc(R) (y with the sign bit of x on top of limb 15), S, D low half, D high half, active (a one-limb value) ----
constexpr int ED_BOUND = 6;   // values absorbed per limb index
__device__ __forceinline__ gl::Ext absorb_limb(gl::Ext acc, gl::Ext gamma, const uint64_t* __restrict__ trace, size_t n, size_t row, int j) {
    const uint32_t base[ED_BOUND - 1] = {ed::cAY, ed::cRY, ed::cSW, ed::cDW, ed::cDW + 16};
    const uint32_t sign[2] = {ed::cSGA, ed::cSGR};
#pragma unroll
    for (int k = 0; k < ED_BOUND - 1; k++) {
        acc = gl::mul(acc, gamma);
        uint64_t v = trace[(size_t)(base[k] + j) * n + row];
        if (k < 2 && j == 15) v += trace[(size_t)sign[k] * n + row] << 15;   // both small: no reduction needed before the add
        acc.a = gl::add(acc.a, v);
    }
    acc = gl::mul(acc, gamma);
    if (j == 0) acc.a = gl::add(acc.a, trace[(size_t)ed::cACT * n + row]);
    return acc;
}

// one lane per slot: the slot's own fingerprint (starting from 0)
__global__ __launch_bounds__(64) void k_ed_bind_slot(const uint64_t* __restrict__ trace, uint32_t n_slots, gl::Ext gamma,
                                                     gl::Ext* __restrict__ slot_fp) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_slots) return;
    const size_t n = (size_t)n_slots * ed::ROWS, row = (size_t)k * ed::ROWS;
    gl::Ext acc{0, 0};
    for (int j = 15; j >= 0; j--) acc = absorb_limb(acc, gamma, trace, n, row, j);
    slot_fp[k] = acc;
}

// one lane per slot: the accumulator column from the slot's start value (exclusive: a row holds what was absorbed before it)
__global__ __launch_bounds__(64) void k_ed_bind_rows(const uint64_t* __restrict__ trace, uint32_t n_slots, gl::Ext gamma,
                                                     const gl::Ext* __restrict__ start, uint64_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_slots) return;
    const size_t n = (size_t)n_slots * ed::ROWS, row0 = (size_t)k * ed::ROWS;
    gl::Ext acc = start[k];
    for (int r = 0; r < ed::ROWS; r++) {
        out[row0 + r] = acc.a;
        out[n + row0 + r] = acc.b;
        if ((r & 15) == 15) acc = absorb_limb(acc, gamma, trace, n, row0 + r, 15 - (r >> 4));
    }
}

}  // namespace nlx

using namespace nlx;

extern "C" int32_t nlx_ed25519_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_slots, const uint64_t gamma[2],
                                          uint64_t* acc_out, uint64_t total_out[2]) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!trace || !gamma || !acc_out || !total_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_slots > 16) return ctx->fail(NLX_E_RANGE, "log_slots must be <= 16");
    // a slot absorbs 16 limbs of ED_BOUND values
    return bind_round(ctx, trace, 1u << log_slots, ed::ROWS, ed::N_COLS0, 16 * ED_BOUND, gamma, acc_out, total_out, k_ed_bind_slot,
                      k_ed_bind_rows);
} NLX_CATCH(ctx)


extern "C" int32_t nlx_fe25519_ops(nlx_ctx* ctx, const int32_t* a, const int32_t* b, size_t n, uint32_t* out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!a || !b || !out) return ctx->fail(NLX_E_INVAL, "NULL buffer");
    if (n == 0) return NLX_OK;
    if (n > (size_t)1 << 24) return ctx->fail(NLX_E_RANGE, "n must be <= 2^24");
    (void)hipSetDevice(ctx->device);
    Staged sa(ctx, a, n * 10 * 4, true, false), sb(ctx, b, n * 10 * 4, true, false), so(ctx, out, n * FE_OPS_WORDS * 4, false, true);
    if (sa.status) return sa.status;
    if (sb.status) return sb.status;
    if (so.status) return so.status;
    hipLaunchKernelGGL(k_fe25519_ops, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, sa.as<int32_t>(), sb.as<int32_t>(), n,
                       so.as<uint32_t>());
    int32_t rc = so.finish();
    if (rc) return rc;
    NLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" int32_t nlx_ed25519_trace(nlx_ctx* ctx, const uint64_t* slots, uint32_t log_slots, uint64_t* trace_out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!slots || !trace_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_slots > 16) return ctx->fail(NLX_E_RANGE, "log_slots must be <= 16");
    (void)hipSetDevice(ctx->device);
    const uint32_t n_slots = 1u << log_slots;
    const size_t n = (size_t)n_slots * ed::ROWS;
    Staged sw(ctx, slots, (size_t)n_slots * ed::SLOT_WORDS * 8, true, false);
    if (sw.status) return sw.status;
    Staged st(ctx, trace_out, (size_t)ed::N_COLS0 * n * 8, false, true);
    if (st.status) return st.status;
    const size_t bytes = (size_t)n_slots * sizeof(ed::Slot) + (n + n_slots) * sizeof(ed::Point) + 16;
    uint32_t bad = 0xFFFFFFFFu;   // written by a queued copy: declared before the scratch that drains the stream
    Scratch scratch(ctx);
    char* d = scratch.alloc_as<char>(bytes);
    if (!d) return NLX_E_NOMEM;
    ed::Slot* d_slots = (ed::Slot*)d;
    ed::Point* d_in = (ed::Point*)(d + (size_t)n_slots * sizeof(ed::Slot));
    ed::Point* d_fin = d_in + n;
    uint32_t* d_bad = (uint32_t*)(d_fin + n_slots);
    hipError_t e0 = hipMemcpyAsync(d_bad, &bad, 4, hipMemcpyHostToDevice, ctx->stream);
    if (e0 != hipSuccess) return ctx->hip_fail(e0, "hipMemcpyAsync");
    // four lanes per slot.  What checks k_ed_scan4 is tests/test_gpu_ed25519_aims.py: its trace against the Python reference, cell
    // by cell, on slots aimed at the arithmetic's extremes, from one slot (fifteen spare quads) to two blocks; its arithmetic and
    // lane moves at given values through nlx_fe25519_ops.  The same walk on one lane is ed::fast_row, which only the host runs
    // (tests/native/ed25519_host_check.cpp, against the witness row and the reference): no device kernel launches it.
    hipLaunchKernelGGL(k_ed_scan4, dim3((n_slots + SCAN4_SLOTS_PER_BLOCK - 1) / SCAN4_SLOTS_PER_BLOCK), dim3(64), 0, ctx->stream,
                       sw.as<uint64_t>(), n_slots, d_slots, d_in, d_fin);
    hipLaunchKernelGGL(k_ed_rows, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_slots, d_in, d_fin, n_slots,
                       st.as<uint64_t>(), d_bad);
    e0 = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream);
    int32_t rc = scratch.finish(st.finish());
    if (!rc && e0 != hipSuccess) rc = ctx->hip_fail(e0, "hipMemcpyAsync");
    if (!rc && bad != 0xFFFFFFFFu)
        rc = ctx->fail(NLX_E_INVAL, "slot %u: the statement is false (the signature does not verify, A / R is not on the curve, "
                                    "S >= L or a coordinate >= p); the trace was written but cannot satisfy the AIR", bad);
    return rc;
} NLX_CATCH(ctx)
