// The resident PLONK key over BN254 and the prover's host helpers that the witness checker shares (bn254_plonk_prove.hip owns
// the definitions; bn254_plonk_check.hip is the second user - DESIGN.md sections 23 and 35).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "bn254_fp.hpp"
#include "ctx.hpp"
#include "../../include/nlx.h"

struct nlx_bn254_plonk_key {
    nlx_ctx* ctx = nullptr;
    uint32_t log_n = 0, n_commit = 0;
    bool coset = false;
    uint64_t* coeffs = nullptr;   // [8 + k][n + 3] natural order, zero above n: ql qr qm qo qk s1 s2 s3 qcp_0 ..
    uint64_t* sigma = nullptr;    // [3][n] s1 s2 s3 by values on H
    uint64_t* coset_ev = nullptr; // [8 + k][4 n] with NLX_BN254_PLONK_KEY_COSET
    void* srs = nullptr;          // n + 3 points, the bucket kernels' form
    uint32_t* rows = nullptr;     // the committed rows, concatenated
    uint32_t seg[NLX_BN254_PLONK_MAX_COMMIT + 1] = {};
    uint32_t commit_rows[NLX_BN254_PLONK_MAX_COMMIT] = {};
    uint32_t last_row = 0;
    uint64_t k1[4], k2[4], shift[4];
    uint64_t commitments[(8 + NLX_BN254_PLONK_MAX_COMMIT) * 8];   // s1 s2 s3 ql qr qm qo qk qcp_0 ..
    std::vector<void*> blocks;
    uint64_t info[NLX_BN254_PLONK_KEY_INFO_WORDS] = {};
    // the witness checker's: s1 s2 s3 decoded to cells, [3][n] words wire << 30 | row; made by the first NLX_BN254_PLONK_CHECK_COPIES
    // of the key, null in a key never checked, released with the key (not counted in info[0]: key_info keeps its five words)
    uint32_t* sigma_cells = nullptr;
};

namespace nlx {
namespace ppk {

// position of ql qr qm qo qk s1 s2 s3 in the key's arrays
enum { QL = 0, QR, QM, QO, QK, S1, S2, S3 };

// The MSM over the resident SRS: sum_i scalars[i] srs[i], i < count <= n + 3.  buckets / wsum: the call's scratch.
struct MsmScratch {
    void* buckets = nullptr;
    void* wsum = nullptr;
};
int32_t msm_scratch(nlx_ctx* ctx, Scratch& scratch, MsmScratch* ms);
int32_t commit(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const MsmScratch& ms, const uint64_t* d_scalars, size_t count, uint64_t out[8]);
// pi2_j on H from the L wire into d_col (n elements)
int32_t build_pi2(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, uint32_t j, const uint64_t* d_l, const uint64_t* d_b2, uint64_t* d_col);
// round 0 for commitment j: pi2_j's coefficients in d_col, [PI2_j] (G1Affine words) and c_j = hash_to_field([PI2_j].Marshal(),
// "BSB22-Plonk") as Montgomery words
int32_t commit_pi2(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const MsmScratch& ms, uint32_t j, const uint64_t* d_l, const uint64_t* d_b2,
                   uint64_t* d_col, uint64_t point_out[8], uint64_t c_out[4]);
// host scalars below r
int32_t check_scalars(nlx_ctx* ctx, const uint64_t* w, size_t count, const char* what);

}  // namespace ppk
}  // namespace nlx
