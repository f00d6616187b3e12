// PoseidonBN128: the Poseidon permutation over BN254's scalar field r (circomlib: width 4, S-box x^5, 8 full and 56 partial
// rounds), the hash of plonky2x's wrapper config, on the 29-bit-limb Montgomery arithmetic of bn254_f29.hpp (RMod, R' = 2^261).
// Spec and provenance: tools/gen_poseidon_bn128.py (the reference model, which also writes poseidon_bn128_constants.inc) and
// DESIGN.md §16.
//
// The plain form: every round adds four constants, applies the S-box (all four elements in a full round, element 0 in a partial
// one) and multiplies by the MDS matrix.  An MDS row is ONE 4-term dot product with a single Montgomery reduction (dot4): the
// 4 x 81 partial products go into the same 17 fixed columns, so a row costs 324 + 90 multiply-adds instead of four products'
// 4 x 171.  Per permutation: 8 x 12 + 56 x 3 = 264 products and 64 x 4 = 256 dot products (~0.15 M multiply-adds per state).
//
// Bounds (checked by the host test tests/native/poseidon_bn128_check.cpp, driven by tests/test_poseidon_bn128_cpu.py):
//   dot4(i, s)    every s_j < 2^258 (limbs 0..7 < 2^29)  -> a column holds at most 36 + 9 partial products < 2^58 each, plus
//                 carries < 2^35: below 2^63.5; the result (sum_j M_ij s_j + m r) / R' < 4 r 2^258 / 2^261 + r < 2^255
//   round         state < 2^255 on entry; + constant (< r) < 2^256: a valid input of mul (< 2^257.5) and of dot4; the S-box and
//                 dot4 outputs are < 2^255 again, so the state stays below 2^255 round after round with no tightening
//   from_words    any integer < 2^256 -> its Montgomery form, < 2^255 (one product with 2^522 mod r)
//   to_words      any value < 2^258 -> the canonical integer < r
#pragma once
#include "bn254_f29.hpp"
#include "poseidon_bn128_constants.inc"

namespace nlx {
namespace pbn {

using f29::Fe;
using f29::RMod;
using f29::NL;
using f29::LB;
using f29::MASK;

constexpr int T = NLX_PBN_T, RF = NLX_PBN_RF, RP = NLX_PBN_RP, ROUNDS = RF + RP;
constexpr int CHUNK = 9;   // Goldilocks elements absorbed per permutation: three per slot, slots 1..3
static_assert(NLX_PBN_T == 4, "the round below is written out for width 4");

#if defined(__HIP__)
__constant__ static const uint32_t RC_DEV[ROUNDS * T * NL] = NLX_PBN_RC_INIT;
__constant__ static const uint32_t MDS_DEV[T * T * NL] = NLX_PBN_MDS_INIT;   // the lane-split form reads its row per lane
#endif
static const uint32_t RC_HOST[ROUNDS * T * NL] = NLX_PBN_RC_INIT;

F29_HD const uint32_t* rc_table() {
#if defined(__HIP_DEVICE_COMPILE__)
    return RC_DEV;   // indexed by the round: wave-uniform, so the compiler reads it with scalar loads
#else
    return RC_HOST;
#endif
}
// MDS entries and 2^522 mod r as literals (fully unrolled loops fold them to constants, like RMod::p)
F29_HD uint32_t mds(int i, int j, int l) {
    constexpr uint32_t M[T * T * NL] = NLX_PBN_MDS_INIT;
    return M[(i * T + j) * NL + l];
}
F29_HD uint32_t r2(int l) {
    constexpr uint32_t V[NL] = NLX_PBN_R2_INIT;
    return V[l];
}

// the Montgomery reduction of a 17-column product (the tail of f29::mul): (sum col[k] 2^(29 k)) / R' mod r, not tightened
F29_HD Fe mont_reduce(uint64_t (&col)[2 * NL]) {
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const uint32_t m = ((uint32_t)col[i] * RMod::NINV) & MASK;
#pragma unroll
        for (int j = 0; j < NL; j++) col[i + j] += (uint64_t)m * RMod::p(j);
        col[i + 1] += col[i] >> LB;   // the low 29 bits of col[i] are now zero
    }
    Fe r;
#pragma unroll
    for (int i = NL; i < 2 * NL - 1; i++) {
        r.v[i - NL] = (uint32_t)col[i] & MASK;
        col[i + 1] += col[i] >> LB;
    }
    r.v[NL - 1] = (uint32_t)col[2 * NL - 1];
    return r;
}

// row i of the MDS product, sum_j M[i][j] s_j / R' mod r: one reduction for the four products (bounds in the header comment)
F29_HD Fe dot4(int i, const Fe (&s)[T]) {
    uint64_t col[2 * NL];
#pragma unroll
    for (int k = 0; k < 2 * NL; k++) col[k] = 0;
#pragma unroll
    for (int j = 0; j < T; j++) {
#pragma unroll
        for (int a = 0; a < NL; a++) {
            const uint64_t m = mds(i, j, a);
#pragma unroll
            for (int b = 0; b < NL; b++) col[a + b] += m * s[j].v[b];
        }
    }
    return mont_reduce(col);
}

F29_HD Fe sbox(const Fe& x) {   // x^5 in three products; x < 2^257.5, result < 2^255
    const Fe x2 = f29::mul<RMod>(x, x);
    const Fe x4 = f29::mul<RMod>(x2, x2);
    return f29::mul<RMod>(x4, x);
}

F29_HD Fe load_rc(const uint32_t* rc, int round, int i) {
    Fe c;
#pragma unroll
    for (int l = 0; l < NL; l++) c.v[l] = rc[(round * T + i) * NL + l];
    return c;
}

// The points of a round at which permute() hands every value it has just produced to an observer: the host check
// (tests/native/poseidon_bn128_check.cpp, `trace`) asserts the bounds of the header comment there, on this very schedule.  The
// default observer does nothing and compiles to nothing.
enum Stage { ON_ENTRY = 0, AFTER_CONSTANTS = 1, SBOX_OUT = 2, MDS_OUT = 3 };
struct NoObserver {
    F29_HD void operator()(int, const Fe&) const {}
};

// the permutation on Montgomery-form elements (each < 2^255 on entry and on exit).  ONE loop over the 64 rounds: whether the
// other three elements pass the S-box is a wave-uniform branch, so the round's code exists once.
template <class Observer = NoObserver>
F29_HD void permute(Fe (&s)[T], Observer obs = Observer{}) {
    const uint32_t* rc = rc_table();
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
#pragma unroll
        for (int i = 0; i < T; i++) {
            obs(ON_ENTRY, s[i]);
            s[i] = f29::add(s[i], load_rc(rc, round, i));
            obs(AFTER_CONSTANTS, s[i]);
        }
        s[0] = sbox(s[0]);
        obs(SBOX_OUT, s[0]);
        if (round < RF / 2 || round >= RF / 2 + RP) {
            s[1] = sbox(s[1]);
            s[2] = sbox(s[2]);
            s[3] = sbox(s[3]);
            obs(SBOX_OUT, s[1]);
            obs(SBOX_OUT, s[2]);
            obs(SBOX_OUT, s[3]);
        }
        // written out: as a loop the compiler leaves it rolled (too large to unroll) and indexes the rows through scratch
        const Fe t0 = dot4(0, s), t1 = dot4(1, s), t2 = dot4(2, s), t3 = dot4(3, s);
        s[0] = t0;
        s[1] = t1;
        s[2] = t2;
        s[3] = t3;
#pragma unroll
        for (int i = 0; i < T; i++) obs(MDS_OUT, s[i]);
    }
}

#if defined(__HIP__)
// ---- the lane-split form: four adjacent lanes hold one state, lane q = lane & 3 holding element q ----
// For the latency-bound top of a Merkle tree, where a level has fewer parents than the chip has lanes: a round is the lane's own
// constant, the S-box on every lane (kept on lane 0 only in a partial round: a select, no divergent branch), three quad rotations
// of the nine limbs (DPP quad_perm, no LDS) and ONE dot4 per lane with that lane's MDS row - 513 + 414 dependent multiply-adds
// per round where the one-lane form runs 513 + 4 x 414 (partial) or 4 x 513 + 4 x 414 (full).
// Bit-identical to permute(): each lane's dot4 sums the same four products into the same columns (the rotation only reorders
// exact 64-bit additions) and each S-box sees the same operand, so the lazy-reduction bounds of the header comment carry over
// unchanged.  The round-constant index depends on the lane here, so the constant is read per lane (one 36-byte read from the
// 144 contiguous bytes of the round, the same for all 16 quads of a wave) and the NEXT round's read is issued ahead of the S-box.
// All four lanes of a quad must be active.
template <int CTRL>
__device__ __forceinline__ Fe quad_rot(const Fe& x) {   // lane q receives the value of lane (q + k) & 3 of its quad
    Fe r;
#pragma unroll
    for (int l = 0; l < NL; l++) r.v[l] = (uint32_t)__builtin_amdgcn_mov_dpp((int)x.v[l], CTRL, 0xF, 0xF, true);
    return r;
}
constexpr int QUAD_ROT1 = 0x39, QUAD_ROT2 = 0x4E, QUAD_ROT3 = 0x93;   // quad_perm [1,2,3,0], [2,3,0,1], [3,0,1,2]

struct QuadRow {
    uint32_t m[T][NL];   // m[k] = M[q][(q + k) & 3]: the entry that multiplies the value rotated in from k lanes up
};
__device__ __forceinline__ QuadRow quad_row(uint32_t q) {
    QuadRow r;
#pragma unroll
    for (int k = 0; k < T; k++)
#pragma unroll
        for (int l = 0; l < NL; l++) r.m[k][l] = MDS_DEV[(q * T + ((q + k) & 3)) * NL + l];
    return r;
}
__device__ __forceinline__ Fe dot4_quad(const QuadRow& row, const Fe (&t)[T]) {
    uint64_t col[2 * NL];
#pragma unroll
    for (int k = 0; k < 2 * NL; k++) col[k] = 0;
#pragma unroll
    for (int j = 0; j < T; j++) {
#pragma unroll
        for (int a = 0; a < NL; a++) {
            const uint64_t m = row.m[j][a];
#pragma unroll
            for (int b = 0; b < NL; b++) col[a + b] += m * t[j].v[b];
        }
    }
    return mont_reduce(col);
}
// s: this lane's element (Montgomery form, < 2^255 on entry and on exit); q = lane & 3
__device__ __forceinline__ void permute_quad(Fe& s, uint32_t q, const QuadRow& row) {
    Fe c = load_rc(RC_DEV, 0, q);
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
        const Fe x = f29::add(s, c);
        c = load_rc(RC_DEV, round + 1 < ROUNDS ? round + 1 : round, q);
        const bool keep = q == 0 || round < RF / 2 || round >= RF / 2 + RP;
        const Fe y = sbox(x);
        Fe t[T];
#pragma unroll
        for (int l = 0; l < NL; l++) t[0].v[l] = keep ? y.v[l] : x.v[l];
        t[1] = quad_rot<QUAD_ROT1>(t[0]);
        t[2] = quad_rot<QUAD_ROT2>(t[0]);
        t[3] = quad_rot<QUAD_ROT3>(t[0]);
        s = dot4_quad(row, t);
    }
}
#endif

// ---- in and out ----
F29_HD Fe to_mont(const Fe& plain) {   // plain < 2^256 -> plain R' mod r, < 2^255
    Fe c;
#pragma unroll
    for (int l = 0; l < NL; l++) c.v[l] = r2(l);
    return f29::mul<RMod>(plain, c);
}
// four little-endian u64 words (an integer < 2^256) -> Montgomery form
F29_HD Fe from_words(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    const uint32_t w[8] = {(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32),
                           (uint32_t)w2, (uint32_t)(w2 >> 32), (uint32_t)w3, (uint32_t)(w3 >> 32)};
    return to_mont(f29::from_words256(w));
}
// a packed Goldilocks triple e0 + e1 2^64 + e2 2^128 (canonical elements: < 2^192 < r) -> Montgomery form
F29_HD Fe from_gl3(uint64_t e0, uint64_t e1, uint64_t e2) { return from_words(e0, e1, e2, 0); }
// Montgomery form -> the canonical integer < r as four little-endian u64 words
F29_HD void to_words(const Fe& a, uint64_t* out) {
    uint32_t w[8];
    f29::to_canonical256<RMod>(a, w);
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
}
// is the integer of four little-endian words below r (canonical)?
F29_HD bool lt_r(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    const uint64_t w[4] = {w0, w1, w2, w3};
    return bnf::below_mod<bnf::RP>(w);
}

}  // namespace pbn
}  // namespace nlx
