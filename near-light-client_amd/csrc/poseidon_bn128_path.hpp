// One Merkle path under PoseidonBN128 on a quad of lanes (plonky2's verify_merkle_proof_to_cap, hash side): the leaf digest of
// an opened row, then one two_to_one per sibling, on the lane-split permutation of poseidon_bn128.hpp (lane q holds element q
// of the width-4 state).  The one piece of device code behind the path kernel of the proof verifier (fri_verify.hip,
// k_fri_paths_bn128) and the public primitive nlx_poseidon_bn128_merkle_verify_batch (poseidon_bn128.hip).
#pragma once
#include "gl.hpp"
#include "poseidon_bn128.hpp"

namespace nlx {
namespace pbn {

#if defined(__HIP__)
constexpr int QUAD_BCAST0 = 0x00;   // quad_perm [0,0,0,0]: every lane of a quad receives lane 0's value

// s: the state before the first permutation - zero for a row that is hashed (width > 4), and for a row that is its own digest
// (hash_or_noop's no-op branch: the caller passes width = 0) the digest on lane 0.  row: `width` words, taken mod p.
// idx: the leaf's index, path: path_len siblings of four canonical words (each digest below r: the caller has checked).
// width, idx and path_len are quad-uniform, and all four lanes of the quad are active.  Returns the state after the last
// permutation: lane 0 holds the digest that the cap must hold at idx >> path_len, in Montgomery form.
//
// ONE loop and one call site of the permutation: step i < ceil(width / 9) absorbs chunk i by pbn_absorb's rule
// (poseidon_bn128.hip) - lane q >= 1 packs group q - 1 of at most three words into its slot, lane 0 keeps the capacity slot, and
// a slot that a short last chunk does not reach keeps its value; every later step is two_to_one(l, r) = permute([0, 0, l, r])[0]
// with the running digest broadcast from lane 0 to lane 2 or 3 and the sibling converted on the lane that takes it.
// Bounds: the running digest is never brought out of Montgomery form between levels.  permute_quad leaves every lane below 2^255,
// which is its own entry bound (header of poseidon_bn128.hpp: "state < 2^255 on entry ... below 2^255 round after round"), and
// from_words turns any integer below 2^256 - a packed group below 2^192, a sibling below r - into a value below 2^255 as well.
__device__ __forceinline__ Fe quad_merkle_path(Fe s, const uint64_t* __restrict__ row, uint32_t width, uint32_t idx,
                                               const uint64_t* __restrict__ path, uint32_t path_len, uint32_t q, const QuadRow& qrow) {
    const uint32_t g3 = 3 * ((q + 3) & 3);   // first word of this lane's group within a chunk (lane 0: past every chunk)
    const uint32_t n_chunks = (width + CHUNK - 1) / CHUNK;
#pragma unroll 1
    for (uint32_t i = 0; i < n_chunks + path_len; i++) {
        const bool leaf = i < n_chunks;   // quad-uniform
        uint64_t w[4] = {0, 0, 0, 0};
        bool take;
        if (leaf) {
            const uint32_t c = i * CHUNK, rem = width - c;
            take = q != 0 && g3 < rem;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (take && g3 + j < rem) w[j] = gl::canon(row[c + g3 + j]);
        } else {
            const uint32_t k = i - n_chunks;
            take = q == (((idx >> k) & 1) ? 2u : 3u);   // the running digest is the right child when the bit is set
            if (take) {
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = path[4 * (size_t)k + j];
            }
        }
        const Fe in = from_words(w[0], w[1], w[2], w[3]);
        const Fe cur = quad_rot<QUAD_BCAST0>(s);
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const uint32_t keep = leaf ? s.v[l] : (q >= 2 ? cur.v[l] : 0u);   // lanes 0 and 1 of a two_to_one state are zero
            s.v[l] = take ? in.v[l] : keep;
        }
        permute_quad(s, q, qrow);
    }
    return s;
}
#endif

}  // namespace pbn
}  // namespace nlx
