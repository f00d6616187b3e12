// The sub-wave Poseidon of hash_kernels.hip, in a header so that the STARK verifier's path kernel
// (stark_verify.hip) runs the same permutation.
#pragma once
#include <hip/hip_runtime.h>
#include "poseidon.hpp"

// =====================================================================================
// Sub-wave Poseidon for small tree levels, FRI leaves and short traces: one state per quad of lanes
// =====================================================================================
// Lane q of an aligned quad holds state elements q, q + 4 and q + 8 (slot m = element q + 4 m), so a wave holds sixteen
// states and every lane works in the full rounds.  The linear layer out[r] = sum_e C[(e - r) mod 12] s[e] (+ 8 s[0] for r = 0)
// needs all twelve elements in every lane: the three other lanes' slots arrive by DPP quad rotations (18 v_mov_dpp, no LDS, no
// fence, no barrier).  With this split the coefficient of the element that rotation d delivered in slot m, for output slot
// m', depends on (m - m') mod 3 only: C[((q + d) % 4 - q + 4 (m - m')) mod 12] - twelve constants per lane, C rotated by the
// lane's position, kept in registers for the whole kernel (a thirteenth carries the + 8 of the matrix's corner).
// (e = 3 q + m would need twenty: the coefficient depends on m - m' itself there.)
//
// CONTRACT (as for k_ed_scan4): DPP reads its neighbours' registers, so whole quads reach the permutation together - spare
// quads of a wave redo the last item and store nothing, no lane returns before the last permutation; a branch around the
// permutation must be quad-uniform.
namespace nlx {
namespace pquad {

struct Mds {
    uint32_t k[4][3];   // [rotation d][(m - m') mod 3]
    uint32_t k00;       // k[0][0] + 8 in the lane that owns element 0: the coefficient of its own slot 0 for its output slot 0
};

__device__ __forceinline__ Mds mds_table(uint32_t q) {
    constexpr uint32_t C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    Mds t;
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
        for (int m = 0; m < 3; m++) {
            uint32_t v = 0;
#pragma unroll
            for (int qq = 0; qq < 4; qq++)
                if (q == (uint32_t)qq) v = C[(((qq + d) & 3) + 12 - qq + 4 * m) % 12];
            t.k[d][m] = v;
        }
    t.k00 = t.k[0][0] + (q == 0 ? 8u : 0u);
    return t;
}

constexpr int ROT1 = 0x39, ROT2 = 0x4E, ROT3 = 0x93;   // quad_perm [1,2,3,0], [2,3,0,1], [3,0,1,2]: lane q reads lane (q + d) % 4

template <int CTRL>
__device__ __forceinline__ gl32::F rot(gl32::F v) {
    gl32::F r;
    r.lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.lo, CTRL, 0xF, 0xF, true);
    r.hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.hi, CTRL, 0xF, 0xF, true);
    return r;
}

// One round without its constants: S-boxes (all three slots in a full round, element 0's lane alone in a partial one), then the
// linear layer.  `cn` (SEED): this lane's three constants of the NEXT round, which seed the accumulators as in gl32::mds_layer,
// so that adding them costs no instruction of its own.  The accumulators of an output are exact integer sums below 2^42 (the
// coefficients of a row add up to 264, a constant's limb is one more term), whatever the order of the terms.
template <bool SEED>
__device__ __forceinline__ void round(gl32::F (&x)[3], uint32_t q, const Mds& mds, bool full, const uint64_t (&cn)[3]) {
    if (full || q == 0) x[0] = gl32::sbox7(x[0]);
    if (full) {
        x[1] = gl32::sbox7(x[1]);
        x[2] = gl32::sbox7(x[2]);
    }
    gl32::F v[4][3];
#pragma unroll
    for (int m = 0; m < 3; m++) {
        v[0][m] = x[m];
        v[1][m] = rot<ROT1>(x[m]);
        v[2][m] = rot<ROT2>(x[m]);
        v[3][m] = rot<ROT3>(x[m]);
    }
#pragma unroll
    for (int mo = 0; mo < 3; mo++) {
        uint64_t al = SEED ? (uint32_t)cn[mo] : 0, ah = SEED ? cn[mo] >> 32 : 0;
#pragma unroll
        for (int d = 0; d < 4; d++)
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const uint32_t k = (d == 0 && m == 0 && mo == 0) ? mds.k00 : mds.k[d][(m - mo + 3) % 3];
                al += (uint64_t)v[d][m].lo * k;
                ah += (uint64_t)v[d][m].hi * k;
            }
        x[mo] = gl32::fold_acc(al, ah);
    }
}

// The plain thirty-round schedule on gl32's primitives; x[m] = element q + 4 m, loose in, loose out (the same field elements
// as poseidon::permute_loose's: callers canonicalise what they store).
__device__ __forceinline__ void permute(gl32::F (&x)[3], uint32_t q, const Mds& mds) {
    const uint64_t* rc = poseidon::RC_DEV + q;
#pragma unroll
    for (int m = 0; m < 3; m++) x[m] = gl32::add_const_v(x[m], rc[4 * m]);
#pragma unroll 1
    for (int r = 0; r < 29; r++) {
        const uint64_t* rn = rc + (r + 1) * 12;   // loaded first: they travel while the S-boxes compute
        const uint64_t cn[3] = {rn[0], rn[4], rn[8]};
        round<true>(x, q, mds, (r < 4) || (r >= 26), cn);
    }
    const uint64_t none[3] = {0, 0, 0};
    round<false>(x, q, mds, true, none);
}

}  // namespace pquad
}  // namespace nlx
