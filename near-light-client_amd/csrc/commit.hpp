// Device-resident polynomial batch commitment (plonky2::fri::oracle::PolynomialBatch).
#pragma once
#include <memory>
#include "ctx.hpp"

struct nlx_commit {
    nlx_ctx* ctx = nullptr;
    uint32_t n_cols = 0;
    uint32_t log_n = 0;
    uint32_t rate_bits = 0;
    uint32_t cap_height = 0;
    uint64_t* coeffs_br = nullptr;  // [col][n], coefficient i at position bitrev(i)
    uint64_t* lde = nullptr;        // [col][r][k] = p_col(g * w_L^(8k + r)), L = n << rate_bits
    uint64_t* digests = nullptr;    // level-major; level 0 in plonky2 leaf order
    const uint64_t* cap = nullptr;  // inside digests
    uint64_t* group_digests = nullptr;  // grouped leaves only: the runs' digests, [4 K][L]
    // Batches (STARK commitment rounds, nlx_stark_desc.batch_cols): the columns are n_trees PolynomialBatches of batch_cols columns
    // (the last one what is left), transformed together but each with its OWN Merkle tree (hash_or_noop leaves over its
    // columns) and cap: tree k's level-major digests start tree_words * k words into `digests`.  n_trees = 1: one batch.
    uint32_t n_trees = 1, batch_cols = 0;
    size_t tree_words = 0;
    bool owner = true;                  // false: a view of one batch (commit_view), nothing to free
    uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS;   // the Merkle tree's hash (include/nlx.h NLX_HASHER_*)
    size_t n() const { return (size_t)1 << log_n; }
    size_t L() const { return (size_t)1 << (log_n + rate_bits); }
    unsigned log_L() const { return log_n + rate_bits; }
};

namespace nlx {
size_t merkle_digest_words(size_t n_leaves, uint32_t cap_height);
// Input kinds for commit_build
enum class CommitInput { ValuesNatural, CoeffsNatural, CoeffsBitrev };
// d_in: device pointer, [col][n] with column stride in_stride.  Enqueues all work on ctx->stream;
// no synchronisation.  On success *out owns coeffs_br / lde / digests.
// leaf_group: 0 = plonky2 leaves (hash_or_noop of the whole LDE row); G > 0 and n_cols > G: grouped leaves (launch.hpp)
// batch_cols: 0 = one batch; B > 0 and n_cols > B: ceil(n_cols / B) batches with a tree each (see nlx_commit)
// hasher: NLX_HASHER_POSEIDON_BN128 hashes leaves and nodes with PoseidonBN128 (poseidon_bn128.hip; no grouped leaves, no
// batches); d_bad then is a zeroed device word the leaf kernel sets when a <= 4-column row packs to a value >= r (RangeFlag)
int32_t commit_build(nlx_ctx* ctx, const uint64_t* d_in, size_t in_stride, CommitInput kind, uint32_t n_cols,
                     uint32_t log_n, uint32_t rate_bits, uint32_t cap_height, nlx_commit** out, uint32_t leaf_group = 0,
                     uint32_t batch_cols = 0, uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS, uint32_t* d_bad = nullptr);
// A commitment one call owns.  nlx_commit_destroy only hands the tables back to the allocator: an owner is declared BEFORE the
// call's Scratch, so that the stream is drained first (destruction runs in reverse order).
struct CommitDeleter { void operator()(nlx_commit* c) const { nlx_commit_destroy(c); } };
using CommitPtr = std::unique_ptr<nlx_commit, CommitDeleter>;
inline int32_t commit_build(nlx_ctx* ctx, const uint64_t* d_in, size_t in_stride, CommitInput kind, uint32_t n_cols, uint32_t log_n,
                            uint32_t rate_bits, uint32_t cap_height, CommitPtr& out, uint32_t leaf_group = 0, uint32_t batch_cols = 0,
                            uint32_t hasher = NLX_HASHER_POSEIDON_GOLDILOCKS, uint32_t* d_bad = nullptr) {
    nlx_commit* c = nullptr;
    const int32_t rc = commit_build(ctx, d_in, in_stride, kind, n_cols, log_n, rate_bits, cap_height, &c, leaf_group, batch_cols, hasher, d_bad);
    out.reset(c);
    return rc;
}
// batch k of a commitment as a commitment of its own (non-owning): its columns of the shared tables, its tree, its cap
nlx_commit commit_view(const nlx_commit* c, uint32_t k);

// ---- PoseidonBN128 (poseidon_bn128.hip) ----
// leaf digests of an LDE table (the row -> tree position map of launch_hash_lde_leaves), hash_or_noop over BN254 Fr
void launch_pbn_hash_lde_leaves(hipStream_t st, const uint64_t* d_lde, size_t col_stride, uint32_t n_cols, unsigned log_n,
                                unsigned rate_bits, uint64_t* d_digests, uint32_t* d_bad);
// levels down to the cap with two_to_one; returns the cap level inside d_digests
// (levels of at most quad_max_parents parents through the lane-split kernel)
const uint64_t* launch_pbn_merkle_levels(hipStream_t st, uint64_t* d_digests, size_t n_leaves, unsigned cap_height,
                                         size_t quad_max_parents);
// commit-phase leaf digests of a FRI layer (launch_fri_leaves' index map and layout), hash_no_pad of the 2 arity words of a coset
void launch_pbn_fri_leaves(hipStream_t st, const uint64_t* d_values, unsigned log_n, unsigned rate_bits, unsigned arity_bits,
                           uint64_t* d_digests, size_t quad_max_leaves);
// a zeroed device word for the BN128 kernels' range flag, and its read-back once the stream has run (synchronises)
struct RangeFlag {
    nlx_ctx* ctx;
    uint32_t* d = nullptr;
    explicit RangeFlag(nlx_ctx* c) : ctx(c) {
        d = (uint32_t*)ctx->alloc(256);
        if (d) (void)hipMemsetAsync(d, 0, 4, ctx->stream);
    }
    ~RangeFlag() { ctx->release(d); }
    RangeFlag(const RangeFlag&) = delete;
    RangeFlag& operator=(const RangeFlag&) = delete;
    // NLX_OK, NLX_E_RANGE (an input had no digest) or the synchronisation's error
    int32_t check(const char* what) {
        uint32_t h = 0;
        hipError_t e = hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return ctx->hip_fail(e, what);
        if (h) return ctx->fail(NLX_E_RANGE, "%s: an input is not a canonical BN254 Fr element, or a row of <= 4 elements packs to a value >= r", what);
        return NLX_OK;
    }
};
}  // namespace nlx
