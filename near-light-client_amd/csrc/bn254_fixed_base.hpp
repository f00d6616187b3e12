// Fixed-base batch scalar multiplication over BN254 G1 / G2 (bn254_fixed_base.hip) as phases of their
// own - what the Groth16 setup (bn254_groth16_setup.hip) schedules: ONE table per group serves every array of the key.
#pragma once
#include <cstddef>
#include <cstdint>
#include "ctx.hpp"

namespace nlx {
namespace fixed_base {

constexpr int WINDOW_BITS = 8;                                          // why 8: DESIGN.md section 36
constexpr int N_WINDOWS = (254 + WINDOW_BITS - 1) / WINDOW_BITS;        // scalars are below r < 2^254
constexpr int N_DIGITS = (1 << WINDOW_BITS) - 1;                        // table entries per window: d = 1 .. 2^w - 1
constexpr uint64_t MAX_SCALARS = (uint64_t)1 << 27;

// the generators the setups multiply (gnark-crypto's words, Montgomery): G1 = (1, 2), G2 = g2Gen
inline constexpr uint64_t G1_GEN[8] = {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full,
                                       0xa6ba871b8b1e1b3aull, 0x14f1d651eb8e167bull, 0xccdd46def0f28c58ull, 0x1c14ef83340fbe5eull};
inline constexpr uint64_t G2_GEN[16] = {0x8e83b5d102bc2026ull, 0xdceb1935497b0172ull, 0xfbb8264797811adfull, 0x19573841af96503bull,
                                        0xafb4737da84c6140ull, 0x6043dd5a5802d8c4ull, 0x09e950fc52a02f86ull, 0x14fef0833aea7b6bull,
                                        0x619dfa9d886be9f6ull, 0xfe7fd297f59e9b78ull, 0xff9e1a62231b7dfeull, 0x28fd7eebae9e4206ull,
                                        0x64095b56c71856eeull, 0xdc57f922327d3cbbull, 0x55f935be33351076ull, 0x0da4a0e693fd6482ull};

// g2 = 0: G1 (64-byte table entries), 1: G2 (128 bytes)
size_t table_bytes(int g2);
// The base on the host, as nlx_bn254_g1_lincomb / nlx_bn254_pairing check a point: NLX_E_RANGE (a coordinate not below q, off the
// curve, G2: outside the subgroup), NLX_E_INVAL (the point at infinity), the error text set
int32_t check_base(nlx_ctx* ctx, const uint64_t* base, int g2);
// table[j][d - 1] = d * 2^(WINDOW_BITS j) * base in the MSM's packed affine form (enqueues; `base`: host words, checked)
int32_t build_table(nlx_ctx* ctx, Scratch& scratch, const uint64_t* base, int g2, void* d_table);
// the first scalar that is not below r into *d_first_bad (0xFFFFFFFF: none); enqueues
void check_scalars(nlx_ctx* ctx, const uint64_t* d_scalars, size_t n, uint32_t* d_first_bad);
// out[i] = scalars[i] * base through the table (enqueues; scalars below r; scratch from `scratch`)
int32_t run(nlx_ctx* ctx, Scratch& scratch, const void* d_table, const uint64_t* d_scalars, size_t n, int montgomery, int g2, uint64_t* d_out);

}  // namespace fixed_base
}  // namespace nlx
