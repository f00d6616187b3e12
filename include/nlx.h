/* nlx.h - C ABI of the MI355X-native prover backend for the nearx plonky2x circuits.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the reference has no FFI seam for its
 * prover, so the seam is cut one layer below nearx (nearx/src/test_utils.rs:29,62,66 call
 * CircuitBuilder::build / CircuitBuild::prove / verify; those reach the plonky2 functions
 * named on each entry point below, crates pinned at /root/reference/Cargo.lock:4864-4866,
 * 4912-4974, 4977-4979, 6515-6517).  INTEGRATION.md shows the Rust `extern "C"` stubs a
 * maintainer adds to the patched plonky2 / starkyx / plonky2x crates.
 *
 * Conventions
 *  - Field elements are canonical (< p = 2^64 - 2^32 + 1) little-endian u64.  Inputs that are
 *    not canonical are rejected only where stated; outputs are always canonical.
 *  - Matrices of polynomials are column-major: cols[c * n + i].
 *  - Every data pointer may be a HOST pointer or a HIP DEVICE pointer (e.g. a torch tensor's
 *    data_ptr()); the library inspects it with hipPointerGetAttributes.  Host buffers are
 *    copied over PCIe inside the call; device buffers are used in place.  Output buffers are
 *    caller-owned.  Handles (nlx_ctx, nlx_commit, nlx_circuit) are library-owned and freed
 *    only by their *_destroy call.
 *  - Every call returns 0 on success or a negative NLX_E_* code and never throws or aborts;
 *    nlx_last_error(ctx) describes the most recent failure on that context.
 *  - A context is bound to one HIP device and is NOT thread-safe (one host thread per
 *    context); different contexts are independent.  Calls are synchronous on return.
 *  - Results are deterministic: identical inputs give identical outputs on any device count
 *    or occupancy; the proof-of-work grind returns the SMALLEST valid nonce.
 *  - There is no CPU fallback: if no gfx950 device is usable nlx_ctx_create fails.
 */
#ifndef NLX_H
#define NLX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLX_OK 0
#define NLX_E_INVAL (-1)
#define NLX_E_NOMEM (-2)
#define NLX_E_HIP (-3)
#define NLX_E_RANGE (-4)
#define NLX_E_UNSUPPORTED (-5)

typedef struct nlx_ctx nlx_ctx;
typedef struct nlx_commit nlx_commit;

/* library / ABI version (major << 16 | minor) */
uint32_t nlx_version(void);
const char* nlx_strerror(int32_t code);
/* The Goldilocks generator pair this library was built with (include/nlx_field.h):
 * out[0] = MULTIPLICATIVE_GROUP_GENERATOR (coset shift, k_i base), out[1] = POWER_OF_TWO_GENERATOR (order 2^32).
 * plonky2_field::goldilocks_field::GoldilocksField::{MULTIPLICATIVE_GROUP_GENERATOR, POWER_OF_TWO_GENERATOR}
 * (crate pinned at /root/reference/Cargo.lock:4912-4914); a caller checks it against its own constants once. */
void nlx_field_generators(uint64_t out[2]);
/* Self-test of the "never throws" rule on the caller's platform: raises a C++ exception INSIDE the library - kind 0: a
 * real failed host allocation (a std::vector larger than the address space), 1: std::runtime_error, 2: a non-standard
 * object - and returns what the entry points' guard makes of it: NLX_E_NOMEM for kind 0, NLX_E_INVAL otherwise
 * (NLX_E_RANGE for an unknown kind).  Kinds 3 / 4 / 5 arm / disarm a fault in nlx_batch_prove's start-up (3: starting the
 * second worker thread fails, 4: the first, 5: off; they return NLX_OK): the batch must still return a code, with the
 * workers that did start joined and every job proved (tests/test_gpu_mapreduce.py).  Needs no context and no GPU.  Every extern "C" definition of the library is a
 * function-try-block with this guard (csrc/ctx.hpp NLX_TRY / NLX_CATCH), so a std::bad_alloc in the host-side
 * orchestration reaches a Rust / Go caller as a return code (crates/protocol/src/prelude.rs:1 maps
 * such codes to anyhow::Error at the caller), never as an unwind through foreign frames. */
int32_t nlx_abi_selftest(int32_t kind);

/* ---- context ---- */
int32_t nlx_ctx_create(int device, nlx_ctx** out);
void nlx_ctx_destroy(nlx_ctx* ctx);
const char* nlx_last_error(const nlx_ctx* ctx);
/* Use an existing HIP stream (e.g. torch's current stream) for all work of this context;
 * NULL restores the context's own stream.  The caller keeps ownership of the stream. */
int32_t nlx_ctx_set_stream(nlx_ctx* ctx, void* hip_stream);
int32_t nlx_ctx_synchronize(nlx_ctx* ctx);
/* Scheduling priority of the context's own stream: high = 1 puts its kernels ahead of other streams' when workgroup slots
 * free up.  For small latency-bound proofs (the curta STARKs of a Sync step) sharing a GPU with a large throughput-bound one
 * (the outer proof): the short kernels no longer queue behind the long ones.  Call it before queuing work. */
int32_t nlx_ctx_set_priority(nlx_ctx* ctx, int high);
/* Restrict the context's own stream to a subset of the device's compute units (bit i of the mask = CU i; MI355X has 256).
 * Two contexts with disjoint masks partition the chip: a chain of short latency-bound kernels (a small STARK) then runs
 * beside a long throughput-bound proof instead of queueing behind its millisecond-long workgroups.  Call it before queuing
 * work; a later nlx_ctx_set_priority undoes it. */
int32_t nlx_ctx_set_cu_mask(nlx_ctx* ctx, const uint32_t* mask, uint32_t n_words);
/* Device buffers for callers without HIP bindings of their own (SURVEY.md §8b `nlx_buf`): every entry point that
 * takes a "host or device" pointer accepts nlx_buf_device_ptr(buf) (+ an offset).  A buffer belongs to its context
 * and must be destroyed before it; upload / download are synchronous. */
typedef struct nlx_buf nlx_buf;
int32_t nlx_buf_create(nlx_ctx* ctx, size_t bytes, nlx_buf** out);
void nlx_buf_destroy(nlx_buf* buf);
void* nlx_buf_device_ptr(const nlx_buf* buf);
size_t nlx_buf_size(const nlx_buf* buf);
int32_t nlx_buf_upload(nlx_buf* buf, size_t offset, const void* src, size_t bytes);
int32_t nlx_buf_download(nlx_buf* buf, size_t offset, void* dst, size_t bytes);
/* The context keeps freed device blocks for reuse (hipMalloc / hipFree synchronise the device).
 * nlx_ctx_memory reports the bytes it holds from the driver and the part currently in use by live handles and
 * tables; nlx_ctx_trim returns the unused part to the driver (it synchronises the stream first). */
int32_t nlx_ctx_memory(const nlx_ctx* ctx, size_t* reserved_bytes, size_t* in_use_bytes);
int32_t nlx_ctx_trim(nlx_ctx* ctx);
/* Per-kernel device timing for measurement (bench.py's roofline): when enabled, the library brackets
 * its main kernels ("intt", "lde", "hash_lde_leaves", "merkle_levels", "quotient", "air_quotient", "fri_combine"; nlx_ntt_batch:
 * "ntt_transform", "ntt_reorder")
 * with HIP events on the context's stream.  nlx_ctx_kernel_timing(ctx, x) also clears the samples. */
int32_t nlx_ctx_kernel_timing(nlx_ctx* ctx, int enable);
int32_t nlx_ctx_kernel_stats(nlx_ctx* ctx, const char* name, uint64_t* calls, double* total_ms, double* alg_bytes);
/* work units of the same samples that are not bytes: Poseidon permutations for "hash_lde_leaves" and "merkle_levels"
 * (the kernels whose bound is the integer-VALU issue rate, not HBM); 0 for the others */
int32_t nlx_ctx_kernel_units(nlx_ctx* ctx, const char* name, double* units);

/* ---- a1: GoldilocksField arithmetic, element-wise (device self-test of the field core) ----
 * a, b: n arbitrary u64 (values >= p are reduced first, except for row 4).  out: 5 x n:
 * row 0 a*b, row 1 a+b, row 2 a-b, row 3 a^-1 (0 if a = 0), row 4 the raw multiply path applied to
 * the UNREDUCED inputs (carry/borrow edges), all canonical. */
int32_t nlx_field_ops(nlx_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* The lazily reduced forms (one reduction per sum of products).  a, b: n pairs of arbitrary u64, NOT reduced first.
 * out: 8 x n, all canonical: rows 0-1 the extension product (a[2i] + a[2i+1] X)(b[2i] + b[2i+1] X), X^2 = 7; rows 2-3
 * (a[2i] + a[2i+1] X) b[2i]; row 4 the 160-bit integer with 32-bit limbs (a[2i] lo, a[2i] hi, a[2i+1] lo, a[2i+1] hi,
 * b[2i+1] lo), lowest first, reduced mod p; rows 5-6 and row 7 the LOOSE device forms of the extension product and of that
 * reduction (any u64 congruent to the value), made canonical afterwards: equal to rows 0-1 and row 4. */
int32_t nlx_ext_ops(nlx_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);

/* ---- a5: plonky2::hash::poseidon::Poseidon::poseidon ----
 * states: n x 12 u64, row-major, permuted in place. */
int32_t nlx_poseidon_permute_batch(nlx_ctx* ctx, uint64_t* states, size_t n);

/* ---- a5/a6: PoseidonHash::hash_or_noop over the rows of a row-major matrix ----
 * (the per-leaf step of MerkleTree::new).  digests_out: n_rows x 4. */
int32_t nlx_hash_rows(nlx_ctx* ctx, const uint64_t* rows, size_t n_rows, size_t row_len, uint64_t* digests_out);

/* ---- a6: plonky2::hash::merkle_tree::MerkleTree::new(leaves, cap_height) ----
 * leaves: row-major n_leaves x leaf_len, n_leaves a power of two >= 2^cap_height.
 * digests_out (optional, may be NULL): level-major digests, level 0 = leaf digests
 * (n_leaves x 4), then n_leaves/2, ... down to and including the cap level;
 * nlx_merkle_digest_words() gives its length.  cap_out: 2^cap_height x 4. */
size_t nlx_merkle_digest_words(size_t n_leaves, uint32_t cap_height);
int32_t nlx_merkle_build(nlx_ctx* ctx, const uint64_t* leaves, size_t n_leaves, size_t leaf_len,
                         uint32_t cap_height, uint64_t* digests_out, uint64_t* cap_out);

/* ---- PoseidonBN128: Poseidon over BN254's scalar field r (circomlib t = 4, x^5, 8 full + 56 partial rounds), the hash of
 * plonky2x's PoseidonBN128GoldilocksConfig (the permutation is pinned by known answers, the hash family is
 * recalled).  A digest is ONE Fr element, written as 4 little-endian u64 words, canonical (not Montgomery): the shape of a
 * Goldilocks HashOut, so digest, cap and path buffers keep their sizes.
 * permute_batch: states n x 16 words (4 elements x 4 words), permuted in place; an element >= r -> NLX_E_RANGE.
 * hash_rows: hash_or_noop of every row (inputs taken mod p): <= 4 elements are the digest sum x_i 2^(64 i) itself (NLX_E_RANGE
 * if that is >= r), longer rows hash_no_pad (9 elements per permutation, three per slot 1..3, the slots overwritten).
 * merkle_build: nlx_merkle_build with these leaves and two_to_one(a, b) = permute([0, 0, a, b])[0] for the nodes.
 * merkle_verify_batch: plonky2's verify_merkle_proof_to_cap for n (leaf, index, path) triples against one cap, one byte each
 * (ok_out[i] = 1: the path reaches cap[indices[i] >> path_len]).  Host arrays in merkle_build's layouts: leaves n x leaf_len
 * (taken mod p; leaf_len <= 4: hash_rows' no-op rule, NLX_E_RANGE if a packed leaf is >= r), indices n u64 (NLX_E_RANGE unless
 * below 2^(path_len + cap_height)), siblings n x path_len x 4 bottom-up, cap 2^cap_height x 4.  A sibling or cap entry is a
 * digest: one integer below r, whatever its words are against p (NLX_E_RANGE otherwise).  One quad of lanes per triple, the
 * device code of the proof verifier's path kernel. */
int32_t nlx_poseidon_bn128_permute_batch(nlx_ctx* ctx, uint64_t* states, size_t n);
int32_t nlx_poseidon_bn128_hash_rows(nlx_ctx* ctx, const uint64_t* rows, size_t n_rows, size_t row_len, uint64_t* digests_out);
int32_t nlx_poseidon_bn128_merkle_build(nlx_ctx* ctx, const uint64_t* leaves, size_t n_leaves, size_t leaf_len, uint32_t cap_height,
                                        uint64_t* digests_out, uint64_t* cap_out);
int32_t nlx_poseidon_bn128_merkle_verify_batch(nlx_ctx* ctx, const uint64_t* leaves, size_t n, size_t leaf_len, const uint64_t* indices,
                                               const uint64_t* siblings, uint32_t path_len, const uint64_t* cap, uint32_t cap_height,
                                               uint8_t* ok_out);

/* ---- a2: plonky2_field::fft::{fft, ifft}, PolynomialCoeffs::coset_fft, PolynomialValues::coset_ifft ----
 * cols: n_cols x 2^log_n, column-major, transformed in place, natural order in and out.
 * inverse = 0: coefficients -> values on shift*<w>;  inverse = 1: values on shift*<w> -> coefficients.
 * coset_shift = 1 (or 0) means the plain subgroup. */
int32_t nlx_ntt_batch(nlx_ctx* ctx, uint64_t* cols, size_t n_cols, uint32_t log_n, int inverse,
                      uint64_t coset_shift);

/* cfg5 / SURVEY 8e: ONE forward transform of 2^log_n points per column split over G = 2^world_log GPUs.  Rank r holds the
 * contiguous slice [r m, (r + 1) m), m = 2^log_n / G, of every column (n_cols x m, column-major, device memory).  The first
 * world_log levels of a decimation in frequency pair element j with j + n / 2^(level + 1) - on another rank: for level =
 * 0 .. world_log - 1 the caller exchanges slices with rank r XOR (G >> (level + 1)) (RCCL send / recv) and this call computes
 * the rank's half of the level in place on `mine` from the partner's slice `theirs`.  After the last cross level every slice
 * is an independent transform of m points: nlx_ntt_batch(mine, n_cols, log_n - world_log, 0, 1) leaves rank r holding
 * X[k] for k = bitrev_G(r) (mod G) at local index k div G.  (near-light-client_amd/split_ntt.py drives it.) */
int32_t nlx_ntt_split_level(nlx_ctx* ctx, uint64_t* mine, const uint64_t* theirs, size_t n_cols, uint32_t log_n, uint32_t world_log,
                            uint32_t rank, uint32_t level);

/* ---- f.4 (first piece): the BN254 scalar-field NTT of the recursive wrap (gnark-crypto ecc/bn254/fr/fft Domain.FFT /
 * FFTInverse; the wrap itself is not in /root/reference - succinct.json:7-8 names the entry point that can run it).
 * cols: n_cols x 2^log_n elements, column-major, transformed in place, natural order in and out; an element is 32 bytes =
 * four little-endian 64-bit words.  flags = NLX_BN254_MONTGOMERY: elements are in Montgomery form (R = 2^256), i.e.
 * gnark-crypto's fr.Element exactly as it lies in memory; flags = 0: canonical integers < r.  log_n <= 28 (Fr's 2-adicity);
 * the root of unity is gnark-crypto's (5^((r-1)/2^28)).  inverse = 1 also multiplies by 1/n. */
#define NLX_BN254_MONTGOMERY 1u
int32_t nlx_bn254_ntt_batch(nlx_ctx* ctx, uint64_t* cols, size_t n_cols, uint32_t log_n, int inverse, uint32_t flags);
/* The same with gnark-crypto's two FFT options.  coset_shift != NULL (four words in the form of the data): the transform on
 * the coset shift * <w> - fft.OnCoset() with the domain's FrMultiplicativeGen: forward evaluates on shift w^k (coefficient j
 * is multiplied by shift^j first), inverse interpolates from there (coefficient j is multiplied by shift^-j last).
 * NLX_BN254_BITREV_OUT: natural order in, bit-reversed order out - what fft.DIF leaves; NLX_BN254_BITREV_IN: bit-reversed
 * order in, natural order out - fft.DIT (decimation in time).  Neither has a reordering pass: a prover that alternates
 * them (FFTInverse(DIF) -> pointwise work -> FFT(DIT, OnCoset)), as gnark's does, never reorders.  Not both at once.
 * coset_shift is read on the HOST (a device pointer is refused); with flags = 0 it must be a canonical integer below r. */
#define NLX_BN254_BITREV_OUT 2u
#define NLX_BN254_BITREV_IN 4u
int32_t nlx_bn254_ntt_batch_coset(nlx_ctx* ctx, uint64_t* cols, size_t n_cols, uint32_t log_n, int inverse, uint32_t flags,
                                  const uint64_t* coset_shift);
/* ---- f.4 (second piece): the G1 multi-scalar multiplication of the wrap's KZG commitments (gnark-crypto ecc/bn254
 * G1Affine.MultiExp(points, scalars, config)).  points: n x 8 little-endian 64-bit words = gnark-crypto's G1Affine as it lies in
 * memory (X then Y, each an fp.Element in Montgomery form, R = 2^256; the point at infinity is (0, 0)); scalars: n x 4 words,
 * fr.Element in Montgomery form with flags = NLX_BN254_MONTGOMERY, canonical integers < r with flags = 0.  out: sum_i
 * scalars[i] * points[i] as a G1Affine (8 words, Montgomery; (0, 0) for the point at infinity).  points / scalars may be host
 * or device pointers; n <= 2^27.  Points are taken to be on the curve (as MultiExp does). */
int32_t nlx_bn254_msm_g1(nlx_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint32_t flags, uint64_t out[8]);
/* The same over G2 (Groth16's B query): points n x 16 words = gnark-crypto's G2Affine (X then Y, each an E2{A0, A1} of two
 * fp.Element, Montgomery; infinity = all zero), the coordinates in Fq2 = Fq[u] / (u^2 + 1); out: a G2Affine, 16 words. */
int32_t nlx_bn254_msm_g2(nlx_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint32_t flags, uint64_t out[16]);
/* The sum of n G1Affine points (same layout; host pointers, computed on the host): joins the partial results of an MSM whose
 * points were split over several GPUs - one addition per rank. */
int32_t nlx_bn254_g1_sum(const uint64_t* points, uint64_t n, uint64_t out[8]);
int32_t nlx_bn254_g2_sum(const uint64_t* points, uint64_t n, uint64_t out[16]);   /* the same for G2Affine points */
/* Segmented G1 linear combinations on the device: out[s] = sum of scalars[t] * points[t] over first[s] <= t < first[s + 1] -
 * many short sums at once (a verifier's digests, one segment per proof and digest), one wave per segment.
 * points: n_terms x 8 words (G1Affine, Montgomery), scalars: n_terms x 4 words, canonical integers below r - both host or
 * device; first: HOST, n_segments + 1 ascending offsets from 0, n_terms = first[n_segments]; out: n_segments x 8 G1Affine words,
 * host or device.  The all-zero words stand for the point at infinity on input and output; a scalar of 0 and an empty segment
 * give it.  Points are checked as nlx_bn254_pairing checks its G1 points: a coordinate not below q, a point off the curve or a
 * scalar not below r gives NLX_E_RANGE, the message names the term ("term t: ...") and nothing is written.  At most 2^20 segments
 * and 2^24 terms.  Kernel-timing names "bn254_g1_lincomb_check", "bn254_g1_lincomb". */
int32_t nlx_bn254_g1_lincomb(nlx_ctx* ctx, const uint64_t* points, const uint64_t* scalars, const uint32_t* first, size_t n_segments,
                             uint64_t* out);
/* Test / bench data on the device: out[i] = (i + 1) * base for i < n as G1Affine words - n distinct curve points (an SRS's
 * worth of gather targets for the MSM; a big-integer model makes a few thousand per second).  out: host or device, n x 8
 * words; n <= 2^27; base must not be the point at infinity. */
int32_t nlx_bn254_g1_multiples(nlx_ctx* ctx, const uint64_t base[8], uint64_t n, uint64_t* out);
/* Fixed-base batch scalar multiplication (csrc/bn254_fixed_base.hip): out[i] = scalars[i] * base for
 * i < n - what an SRS [tau^i]_1, a Groth16 setup and every honest test key are made of.  base: HOST, 8 (G1Affine) or 16
 * (G2Affine) Montgomery words; scalars: n x 4 words, fr.Element in Montgomery form with flags = NLX_BN254_MONTGOMERY, canonical
 * integers with flags = 0, host or device; out: n x 8 (G1) or n x 16 (G2) words, Montgomery, host or device; the all-zero words
 * stand for the point at infinity (a scalar of 0).  n <= 2^27.  NLX_E_RANGE: a scalar not below r (the message names its
 * index), a base with a coordinate not below q, off its curve or (G2) outside the subgroup of order r - the checks
 * nlx_bn254_g1_lincomb and nlx_bn254_pairing apply; NLX_E_INVAL: the base is the point at infinity.  Nothing is written on a
 * refusal.  A table of d * 2^(8 j) * base (d < 256, j < 32) is built per call in HBM; then 32 mixed additions per scalar and
 * one inversion per lane.  Kernel-timing names "bn254_fixed_base_table", "bn254_fixed_base_g1", "bn254_fixed_base_g2". */
int32_t nlx_bn254_g1_scalar_muls(nlx_ctx* ctx, const uint64_t base[8], const uint64_t* scalars, uint64_t n, uint32_t flags, uint64_t* out);
int32_t nlx_bn254_g2_scalar_muls(nlx_ctx* ctx, const uint64_t base[16], const uint64_t* scalars, uint64_t n, uint32_t flags, uint64_t* out);

/* ---- f.4 (third piece): the PLONK prover's quotient chain and a KZG opening on those kernels.  What the wrap's prover
 * (gnark backend/plonk/bn254 Prove; Go, not in /root/reference - succinct.json:7-8 names the entry point that runs it) does
 * between its commitments, restated from the published protocol (three-wire PLONK as gnark arithmetises it), not from
 * gnark's source: no blinding terms, no gnark byte format.  Every element is an fr.Element as it lies in memory (four words,
 * Montgomery): flags must be NLX_BN254_MONTGOMERY.
 *
 * nlx_bn254_plonk_quotient: the thirteen polynomials given by their values on H = <w_n> (host or device pointers, n x 4 words
 * each, natural order; pi may be NULL) -> coefficients (FFTInverse, DIF) -> values on the coset coset_shift * <w_4n> (FFT,
 * DIT, OnCoset) -> there, pointwise,
 *     t = [ ql l + qr r + qm l r + qo o + qk + pi
 *           + alpha ( (l + beta x + gamma)(r + beta k1 x + gamma)(o + beta k2 x + gamma) z
 *                     - (l + beta s1 + gamma)(r + beta s2 + gamma)(o + beta s3 + gamma) z(w_n x) )
 *           + alpha^2 L1(x) (z - 1) ] / (x^n - 1),           L1(x) = (x^n - 1) / (n (x - 1))
 * -> coefficients (FFTInverse, OnCoset).  t_out: the three chunks t_lo, t_mid, t_hi of n coefficients each (3 n x 4 words,
 * natural order, host or device).  *high_chunk_is_zero (may be NULL): 1 if coefficients 3n .. 4n-1 all vanish - they do
 * exactly when the witness satisfies gates and copy constraints, and a prover must not commit to t otherwise.
 * coset_shift, k1, k2, alpha, beta, gamma: host, four words each, in the form of the data.  2 <= log_n <= 26. */
typedef struct {
    uint32_t log_n;
    uint32_t flags;                       /* NLX_BN254_MONTGOMERY */
    const uint64_t *ql, *qr, *qm, *qo, *qk;   /* selectors */
    const uint64_t *s1, *s2, *s3;             /* the permutation, as polynomials: s_j(w^i) = the point of H, k1 H or k2 H that wire j of gate i maps to */
    const uint64_t *l, *r, *o;                /* wires */
    const uint64_t *z;                        /* the permutation's grand product, z(w^0) = 1 */
    const uint64_t *pi;                       /* public-input polynomial (values on H) or NULL */
    const uint64_t *coset_shift, *k1, *k2;    /* gnark: the domain's FrMultiplicativeGen u, then k1 = u, k2 = u^2 */
    const uint64_t *alpha, *beta, *gamma;
    /* Blinding (flags |= NLX_BN254_PLONK_BLINDED; gnark: getBlindedPolynomial, order 1 for l, r, o and order 2 for z): host, nine
     * elements of four words in the form of the data - b[0], b[1] for l, b[2], b[3] for r, b[4], b[5] for o, b[6], b[7], b[8] for
     * z: the polynomial that enters the quotient is l(X) + (b[0] + b[1] X)(X^n - 1) ... z(X) + (b[6] + b[7] X + b[8] X^2)(X^n - 1)
     * (same values on H; the caller commits to and opens the blinded polynomials).  The quotient then has 3 n + 6 coefficients:
     * t_out receives ALL 4 n of them (4 n x 4 words) and *high_chunk_is_zero tells whether coefficients 3 n + 6 .. 4 n - 1 vanish;
     * gnark's h1, h2, h3 are t[0 : n + 2], t[n + 2 : 2 n + 4], t[2 n + 4 : 3 n + 6].  log_n >= 3.  NULL / flag clear: as before. */
    const uint64_t *blinding;
    /* Bsb22 commitments (flags |= NLX_BN254_PLONK_COMMIT; gnark: api.Commit, the selectors Qcp and the polynomials PI2 of its
     * proving key and proof).  The gate identity gains sum_j qcp[j] pi2[j], j < n_commit: qcp[j] is 1 on the rows whose L wire
     * commitment j covers and 0 elsewhere; pi2[j] holds those L values, two blinding values on rows where qcp[j] is 0, and 0
     * elsewhere.  qcp and pi2 are HOST arrays of n_commit pointers, each to n x 4 words on H (host or device) like the other
     * polynomials; pi2 is not blinded by (X^n - 1) multiples.  The degree bound and t_out are as without commitments, and
     * *high_chunk_is_zero also turns 0 when a pi2 does not close its rows.  May be combined with NLX_BN254_PLONK_BLINDED.
     * These three fields are read ONLY when the flag is set: a caller compiled against the struct that ended at `blinding`
     * keeps working.  With the flag set: n_commit outside 1 .. NLX_BN254_PLONK_MAX_COMMIT -> NLX_E_RANGE; a NULL array or a
     * NULL entry -> NLX_E_INVAL. */
    uint32_t n_commit;
    const uint64_t *const *qcp;
    const uint64_t *const *pi2;
} nlx_bn254_plonk_quotient_args;
#define NLX_BN254_PLONK_BLINDED 0x100u
#define NLX_BN254_PLONK_COMMIT 0x200u
#define NLX_BN254_PLONK_MAX_COMMIT 4u
int32_t nlx_bn254_plonk_quotient(nlx_ctx* ctx, const nlx_bn254_plonk_quotient_args* args, uint64_t* t_out, int32_t* high_chunk_is_zero);
/* The permutation's grand product (gnark computeZ / the paper's round 2): z(w^0) = 1,
 * z(w^(i+1)) = z(w^i) prod_j (w_j(i) + beta id_j(i) + gamma) / (w_j(i) + beta s_j(i) + gamma), id = (w^i, k1 w^i, k2 w^i).
 * One inversion per 64 rows (batch inversion), the running product as a multi-level scan.  All inputs n x 4 words on H in
 * natural order, host or device; beta, gamma, k1, k2 host; z_out: n x 4 words, host or device.  *closes (may be NULL): 1 if
 * the product returns to 1 after the last row - it does exactly when the wires respect the permutation.
 * 1 / 0 := 0, as gnark's BatchInvert has it: a row whose denominator vanishes contributes the ratio 0 and nothing else, so z is
 * exact up to and including that row, 0 after it, and *closes is 0.  beta, gamma, k1, k2 are fr.Element words: one that is not
 * below r -> NLX_E_RANGE, as for nlx_bn254_plonk_quotient. */
int32_t nlx_bn254_plonk_grand_product(nlx_ctx* ctx, uint32_t log_n, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                                      const uint64_t* s1, const uint64_t* s2, const uint64_t* s3, const uint64_t beta[4],
                                      const uint64_t gamma[4], const uint64_t k1[4], const uint64_t k2[4], uint64_t* z_out,
                                      int32_t* closes);
/* out[i] = sum_t scalars[t] * polys[t][i], i < m: the linearisation polynomial and the batched opening polynomial of the last
 * round.  polys: host array of n_terms (<= 16) pointers, each to m x 4 words (host or device); scalars: host, n_terms x 4 words;
 * out: m x 4 words, host or device (may alias one of the inputs). */
int32_t nlx_bn254_fr_lincomb(nlx_ctx* ctx, uint64_t m, uint32_t n_terms, const uint64_t* const* polys, const uint64_t* scalars,
                             uint64_t* out);
/* Groth16's quotient (gnark backend/groth16/bn254 computeH): a, b, c = the values of A w, B w, C w on H (n x 4 words each,
 * natural order, host or device) -> h = (a b - c) / (x^n - 1) as n coefficients (the top one is zero): three FFTInverse(DIF),
 * three FFT(DIT, OnCoset) on the coset of the SAME size, one pointwise pass (the divisor is one constant there), one
 * FFTInverse(OnCoset).  The proof's points are then nlx_bn254_msm_g1 / _g2 over the proving key's queries. */
int32_t nlx_bn254_groth16_quotient(nlx_ctx* ctx, uint32_t log_n, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                                   const uint64_t coset_shift[4], uint64_t* h_out);
/* One KZG opening (gnark-crypto kzg.Open): coeffs = m coefficients (natural order, host or device), zeta = the point (host).
 * y_out = p(zeta); quotient_out (may be NULL; host or device, m - 1 coefficients) = (p(X) - p(zeta)) / (X - zeta) - the
 * running Horner values, computed as a parallel scan; proof_out (may be NULL) = its commitment sum_i q_i srs[i] over the first
 * m - 1 points of the SRS (G1Affine words as for nlx_bn254_msm_g1; host or device).  2 <= m <= 2^28. */
int32_t nlx_bn254_kzg_open(nlx_ctx* ctx, const uint64_t* coeffs, uint64_t m, const uint64_t zeta[4], const uint64_t* srs,
                           uint64_t y_out[4], uint64_t* quotient_out, uint64_t proof_out[8]);
/* Self-test entry for the nine-limb loose field every BN254 kernel computes on (csrc/bn254_f29.hpp), one lane per case.
 * modulus: the base field q or the scalar field r.  a, b: n x 9 u32 raw limbs of 29 bits (value = sum l_i 2^(29 i)), host or
 * device; limbs 0 .. 7 below 2^29, limb 8 takes what is left of a value below 2^261 - NOT reduced first, so the operand limits
 * the header states can be reached.  out: n x NLX_BN254_F29_OPS_WORDS u32 (host or device), per case eleven results of nine
 * limbs each, in this order: mul(a, b), add(a, b), sub<4>(a, b), sub<8>(a, b), tighten(a), canonical(a), is_zero_mod(a) (0 or 1
 * in limb 0), from_mont256(to_words256(a)), from_words256(to_words256(a)), to_canonical256(a) (its words re-sliced), x32(a).
 * A result is meaningful where the case's operands lie inside that function's bounds. */
#define NLX_BN254_MODULUS_Q 0u
#define NLX_BN254_MODULUS_R 1u
#define NLX_BN254_F29_OPS_WORDS 99
int32_t nlx_bn254_f29_ops(nlx_ctx* ctx, uint32_t modulus, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);

/* ---- f.4, the Groth16 half: whole proofs from a proving key resident in HBM (gnark backend/groth16/bn254 ProvingKey and Prove;
 * Go, not in the reference: the layout and the rules are recalled from gnark v0.9, parity with gnark-produced bytes unpinned -
 * DESIGN.md section 19).  The descriptor carries gnark's ProvingKey as it lies in memory; every pointer may be host or device.
 *   g1_a / g1_b / g2_b  G1.A, G1.B, G2.B: the queries FILTERED of their points at infinity (G1Affine: 8 words, G2Affine: 16 words,
 *                       Montgomery) with their counts; infinity_a / infinity_b: InfinityA / InfinityB, one byte per wire (Go's
 *                       []bool), non-zero = that wire's point was filtered out.  G2.B is filtered by InfinityB.
 *   g1_k                G1.K, one point per private wire (n_wires - n_public of them)
 *   g1_z                G1.Z, 2^log_n - 1 points
 *   g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta   the five single points
 *   log_n               the domain's size; n_constraints <= 2^log_n; n_public counts the constant wire (wire 0, value 1);
 *                       wire order: ONE, public, secret, internal
 *   the R1CS (optional; all of it or none): three CSR matrices of n_constraints rows - x_row_ptr: n_constraints + 1 offsets,
 *                       x_wire / x_coeff_id: one wire id and one index into `coeffs` per term - and the coefficient table
 *                       (n_coeffs x 4 words, fr.Element Montgomery).  Without it nlx_bn254_r1cs_eval and a prove call that
 *                       does not bring a, b, c return NLX_E_INVAL.
 *   n_commitments       Bsb22 / Pedersen commitments (Proof.Commitments, CommitmentPok): must be 0 here, else NLX_E_UNSUPPORTED -
 *                       a key with commitments brings its Pedersen bases through nlx_bn254_groth16_key_create_committed.
 * Creation uploads once, converts every query to the bucket kernels' form once (the three wire queries and G1.K expanded to the
 * wires' index space, the point at infinity at masked and public positions, so that one set of sorted digits serves all four),
 * and classifies the R1CS: coefficients equal to 1 or -1 are marked (added or subtracted, no product), rows of more than 64
 * terms go to a wave-per-row list.  NLX_E_RANGE: flags other than NLX_BN254_MONTGOMERY, log_n outside 1 .. 26, n_constraints >
 * 2^log_n, a mask whose count of clear entries disagrees with its query's count, counts of G1.K / G1.Z / G2.B that disagree
 * with the sizes, a wire id >= n_wires, a coefficient id outside the table, row pointers that decrease.  The key belongs to
 * its context and must be destroyed before it. */
typedef struct nlx_bn254_groth16_key nlx_bn254_groth16_key;
typedef struct {
    uint32_t log_n;
    uint32_t flags;                     /* NLX_BN254_MONTGOMERY */
    uint64_t n_wires, n_public, n_constraints;
    const uint64_t* g1_a; uint64_t n_g1_a;
    const uint64_t* g1_b; uint64_t n_g1_b;
    const uint64_t* g2_b; uint64_t n_g2_b;
    const uint64_t* g1_k; uint64_t n_g1_k;
    const uint64_t* g1_z; uint64_t n_g1_z;
    const uint8_t *infinity_a, *infinity_b;
    const uint64_t *g1_alpha, *g1_beta, *g1_delta, *g2_beta, *g2_delta;
    const uint64_t *a_row_ptr, *b_row_ptr, *c_row_ptr;
    const uint32_t *a_wire, *b_wire, *c_wire;
    const uint32_t *a_coeff_id, *b_coeff_id, *c_coeff_id;
    const uint64_t* coeffs; uint64_t n_coeffs;
    uint32_t n_commitments;
} nlx_bn254_groth16_key_desc;
int32_t nlx_bn254_groth16_key_create(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* desc, nlx_bn254_groth16_key** out);
void nlx_bn254_groth16_key_destroy(nlx_bn254_groth16_key* key);
/* A key with k = 1 .. NLX_BN254_GROTH16_MAX_COMMITMENTS Bsb22 / Pedersen commitments (gnark's ProvingKey.CommitmentKeys and the
 * R1CS's CommitmentInfo; rules recalled and unpinned like the rest: tools/groth16_commit_model.py).  Every
 * pointer may be host or device.
 *   n_commitments       k; desc->n_commitments must equal it
 *   n_private           k counts: |PrivateCommitted_j|; M = their sum
 *   private_wires       the k sets concatenated, M wire ids: private wires, ascending inside a set, the sets pairwise disjoint
 *   basis, basis_exp_sigma   the k Pedersen keys' Basis and BasisExpSigma concatenated, M G1Affine points each (8 words,
 *                       Montgomery; (0, 0) = the point at infinity is allowed)
 *   commitment_wires    k wire ids (CommitmentIndex_j): private, not committed, distinct
 * desc->g1_k then holds n_wires - n_public - M - k points: the private wires that are neither committed nor a commitment's, in
 * ascending order.  NLX_E_RANGE: k outside 1 .. 8, desc->n_commitments != k, an id below n_public or >= n_wires, ids that do not
 * ascend inside a set, sets that overlap, a commitment wire that is committed or listed twice, a G1.K count that disagrees -
 * and everything nlx_bn254_groth16_key_create refuses.  The two bases are converted once and stay compact (M points each) next
 * to the wire ids; the committed and the commitment wires hold the point at infinity in the expanded G1.K. */
#define NLX_BN254_GROTH16_MAX_COMMITMENTS 8
typedef struct {
    uint32_t n_commitments;
    const uint64_t* n_private;
    const uint32_t* private_wires;
    const uint64_t *basis, *basis_exp_sigma;
    const uint32_t* commitment_wires;
} nlx_bn254_groth16_commit_desc;
int32_t nlx_bn254_groth16_key_create_committed(nlx_ctx* ctx, const nlx_bn254_groth16_key_desc* desc,
                                               const nlx_bn254_groth16_commit_desc* commit_desc, nlx_bn254_groth16_key** out);
/* out[0] = bytes the key keeps resident in HBM (the Pedersen bases and the committed wire ids included), out[1] = R1CS rows run
 * one per lane, out[2] = rows run one per wave, out[3] = terms of the three matrices, out[4] = terms whose coefficient is 1 or
 * -1, out[5] = the row-length threshold, out[6] = M, the committed wires, out[7] = k, the commitments (both 0 on a key without). */
#define NLX_BN254_GROTH16_KEY_INFO_WORDS 8
int32_t nlx_bn254_groth16_key_info(const nlx_bn254_groth16_key* key, uint64_t out[NLX_BN254_GROTH16_KEY_INFO_WORDS]);
/* a = A w, b = B w, c = C w: three sparse matrix-vector products over Fr.  witness: n_wires x 4 words (Montgomery), host or
 * device; a_out, b_out, c_out: 2^log_n x 4 words each, host or device, rows past n_constraints zero.  Kernel-timing name
 * "bn254_r1cs_eval", units terms. */
int32_t nlx_bn254_r1cs_eval(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, uint64_t* a_out, uint64_t* b_out,
                            uint64_t* c_out);
/* One proof.  a, b, c: the solver's values of A w, B w, C w on H (2^log_n x 4 words, host or device; gnark: solution.A/B/C), or
 * all three NULL: computed from the key's matrices.  r, s: the blinding scalars, host, four Montgomery words each, below r.
 * Before anything is committed: w[0] must be 1 and a_i b_i = c_i must hold on every row - otherwise NLX_E_INVAL (the message
 * names the first failing row) and no output is written.  Then h = (a b - c) / Z_H on the device (coset shift 5, gnark's
 * domain generator), the four MSMs over the wire vector on one digit decomposition and one set of sorted indices, G1.Z over h,
 * and on the host Ar = sum w_i A_i + alpha + r delta, Bs = sum w_i B_i + beta + s delta (G2; Bs1 the same in G1),
 * Krs = sum_private w_i K_i + sum_(i < n-1) h_i Z_i + s Ar + r Bs1 - r s delta.
 * ar_out, krs_out: G1Affine words; bs_out: G2Affine words.  Kernel-timing name "bn254_groth16_msms".  A key with commitments:
 * NLX_E_INVAL (its proofs come from nlx_bn254_groth16_prove_committed). */
int32_t nlx_bn254_groth16_prove(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, const uint64_t* a,
                                const uint64_t* b, const uint64_t* c, const uint64_t r[4], const uint64_t s[4], uint64_t ar_out[8],
                                uint64_t bs_out[16], uint64_t krs_out[8]);
/* C_j = sum_i w[PrivateCommitted_j[i]] Basis_j[i] of commitment j < k: the call a solver's hint makes while the witness is still
 * being solved - of `witness` (n_wires x 4 words, Montgomery, host or device) only the wires of PrivateCommitted_j are read.
 * out: G1Affine words, (0, 0) for the point at infinity (an empty set, or values that are all zero).  The hash that turns C_j
 * into the commitment wire's value is the caller's here (nlx_bn254_hash_to_field is the library's, for the PLONK prover).  NLX_E_INVAL on a key without commitments,
 * NLX_E_RANGE for j >= k.  Kernel-timing name "bn254_groth16_commit", units committed wires. */
int32_t nlx_bn254_groth16_commit(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, uint32_t j, const uint64_t* witness, uint64_t out[8]);
/* One proof on a key with commitments: everything nlx_bn254_groth16_prove does (the same guards first, the same a, b, c, r, s;
 * Krs sums G1.K over the private wires that are left: the prover does not add C_j to it), and all k commitments recomputed from
 * the finished witness with their proof of knowledge (pedersen.BatchProve):
 *   commitments_out     k x 8 words: C_j, G1Affine
 *   pok_out             Pok = sum_j rho^j sum_i w[PrivateCommitted_j[i]] BasisExpSigma_j[i]: one gather of the M committed values
 *                       into a plain and a rho^j-scaled compact vector, k MSMs over slices of the first, ONE over the second
 *   rho                 the folding challenge, host, four Montgomery words, below r (else NLX_E_RANGE); the caller's hash of
 *                       the k commitment-wire values; not used when k = 1
 * The library does not check that the witness's commitment wires hold the challenges of the C_j it returns: the caller does (the
 * Python binding's prove_committed).  A key without commitments: NLX_E_INVAL.  No output is written before the end. */
int32_t nlx_bn254_groth16_prove_committed(nlx_ctx* ctx, const nlx_bn254_groth16_key* key, const uint64_t* witness, const uint64_t* a,
                                          const uint64_t* b, const uint64_t* c, const uint64_t r[4], const uint64_t s[4],
                                          const uint64_t rho[4], uint64_t ar_out[8], uint64_t bs_out[16], uint64_t krs_out[8],
                                          uint64_t* commitments_out, uint64_t pok_out[8]);

/* gnark's groth16.Setup(r1cs) from a trapdoor, on the device (csrc/bn254_groth16_setup.hip).  The rules are
 * rule 3 of tools/groth16_model.py and rule 1 of tools/groth16_commit_model.py - recalled from gnark v0.9, UNPINNED like the
 * rest of the Groth16 half.  The descriptor:
 *   log_n, n_wires, n_public, n_constraints, the R1CS (required) and n_commitments / n_private / private_wires /
 *                       commitment_wires: as in nlx_bn254_groth16_key_desc and nlx_bn254_groth16_commit_desc (host or device)
 *   tau, alpha, beta, gamma, delta    the trapdoor: HOST, four Montgomery words each
 *   sigma               the Pedersen trapdoor: HOST, four Montgomery words; read only for n_commitments > 0
 * On the device: L_j(tau) for j < 2^log_n with one batched inversion; A_i(tau), B_i(tau), C_i(tau) as the transposed products
 * of the three matrices (terms sorted by wire id; a lane per wire, a wave per wire above 64 terms); the scalars of every key
 * array; ONE fixed-base launch over G1 and one over G2.  InfinityA[i] / InfinityB[i] are set exactly when A_i(tau) / B_i(tau) is
 * zero, whether the wire is absent from the matrix or its terms cancel.
 * NLX_E_RANGE, the message naming the cause: flags other than NLX_BN254_MONTGOMERY, a trapdoor value that is zero or not
 * below r, tau^(2^log_n) = 1, and everything nlx_bn254_groth16_key_create[_committed] refuses about sizes, ids and sets.
 * Nothing is left allocated on a refusal.  The result belongs to its context and must be destroyed before it.
 * The Pedersen verifying key is ([1]_2, [-sigma]_2): the model's rule takes BasisExpSigma = sigma Basis, under which
 * e(C, [-sigma]_2) e(Pok, [1]_2) = 1 (a setup that takes BasisExpSigma = (1 / sigma') Basis writes the same key as [-1 / sigma']_2).
 * (The type is known by its struct tag only: the name is the entry point's.) */
struct nlx_bn254_groth16_setup;
typedef struct {
    uint32_t log_n;
    uint32_t flags;                     /* NLX_BN254_MONTGOMERY */
    uint64_t n_wires, n_public, n_constraints;
    const uint64_t *a_row_ptr, *b_row_ptr, *c_row_ptr;
    const uint32_t *a_wire, *b_wire, *c_wire;
    const uint32_t *a_coeff_id, *b_coeff_id, *c_coeff_id;
    const uint64_t* coeffs; uint64_t n_coeffs;
    const uint64_t *tau, *alpha, *beta, *gamma, *delta;
    uint32_t n_commitments;
    const uint64_t* n_private;
    const uint32_t* private_wires;
    const uint32_t* commitment_wires;
    const uint64_t* sigma;
} nlx_bn254_groth16_setup_desc;
int32_t nlx_bn254_groth16_setup(nlx_ctx* ctx, const nlx_bn254_groth16_setup_desc* desc, struct nlx_bn254_groth16_setup** out);
void nlx_bn254_groth16_setup_destroy(struct nlx_bn254_groth16_setup* setup);
/* out[0..3] = the points of G1.A, G1.B (= G2.B), G1.K, G1.Z; out[4] = M, the committed wires; out[5] = k; out[6] = the points of
 * ic (n_public + k); out[7] = the wires whose sums ran one per wave (over the three matrices). */
#define NLX_BN254_GROTH16_SETUP_INFO_WORDS 8
int32_t nlx_bn254_groth16_setup_info(const struct nlx_bn254_groth16_setup* setup, uint64_t out[NLX_BN254_GROTH16_SETUP_INFO_WORDS]);
/* One array of the result copied to `out` (host or device), in gnark-crypto's layout: G1Affine 8 words, G2Affine 16 words,
 * Montgomery; the masks one byte per wire.  The counts are nlx_bn254_groth16_setup_info's; basis and basis_exp_sigma hold the k
 * Pedersen keys' points concatenated (M each).  An array of no points writes nothing.  NLX_E_RANGE: an unknown `which`; the
 * two Pedersen G2 points on a result without commitments. */
enum {
    NLX_G16_SETUP_G1_A = 0, NLX_G16_SETUP_G1_B = 1, NLX_G16_SETUP_G2_B = 2, NLX_G16_SETUP_G1_K = 3, NLX_G16_SETUP_G1_Z = 4,
    NLX_G16_SETUP_INFINITY_A = 5, NLX_G16_SETUP_INFINITY_B = 6,
    NLX_G16_SETUP_G1_ALPHA = 7, NLX_G16_SETUP_G1_BETA = 8, NLX_G16_SETUP_G1_DELTA = 9, NLX_G16_SETUP_G2_BETA = 10, NLX_G16_SETUP_G2_DELTA = 11,
    NLX_G16_SETUP_BASIS = 12, NLX_G16_SETUP_BASIS_EXP_SIGMA = 13,
    NLX_G16_SETUP_G2_GAMMA = 14, NLX_G16_SETUP_IC = 15, NLX_G16_SETUP_PEDERSEN_G = 16, NLX_G16_SETUP_PEDERSEN_G_ROOT_SIGMA_NEG = 17
};
int32_t nlx_bn254_groth16_setup_read(const struct nlx_bn254_groth16_setup* setup, uint32_t which, void* out);
/* The resident proving key of this setup (with its R1CS, and its Pedersen bases for k > 0), built from the device arrays by
 * nlx_bn254_groth16_key_create[_committed]: the points never visit the host.  The key is the caller's, independent of `setup`. */
int32_t nlx_bn254_groth16_setup_key(const struct nlx_bn254_groth16_setup* setup, nlx_bn254_groth16_key** out);

/* ---- f.4, the PLONK half: whole gnark-shaped proofs from a proving key resident in HBM (gnark backend/plonk/bn254 ProvingKey and
 * Prove; Go, not in the reference: the protocol is restated from its published structure, parity with gnark-produced bytes
 * unpinned - DESIGN.md section 23).  Every element is an fr.Element / G1Affine as it lies in memory (Montgomery words).
 *   log_n               3 .. 26; flags: NLX_BN254_MONTGOMERY, optionally | NLX_BN254_PLONK_KEY_COSET
 *   ql qr qm qo qk s1 s2 s3   the fixed polynomials by values on H (n x 4 words each, host or device), as gnark's trace holds them
 *   k1, k2, coset_shift host, four words each, below r
 *   srs, n_srs          G1Affine points (8 words each, host or device); n_srs >= n + 3, the first n + 3 are used
 *   n_commit            k = 0 .. NLX_BN254_PLONK_MAX_COMMIT Bsb22 commitments; with k > 0:
 *   qcp                 HOST array of k pointers, qcp[j] = the selector of commitment j by values on H (host or device)
 *   n_committed         k counts (host or device): the rows whose L wire commitment j covers
 *   committed_rows      the k sets concatenated (host or device), ascending inside a set, each row < n
 *   commit_rows         k rows (host or device): commitment j's own row i_j, whose L wire must hold c_j
 *   last_row            the key-wide second blinding row (gnark: the last constraint)
 * Creation computes the 8 + k coefficient forms once (kept padded to n + 3), converts the first n + 3 SRS points to the bucket
 * kernels' form once, computes the 8 + k KZG commitments, and checks on the device that each qcp[j] is 1 exactly on its rows.
 * With NLX_BN254_PLONK_KEY_COSET the key also keeps the fixed polynomials' values on the coset coset_shift * <w_4n>
 * ((8 + k) * 4 n * 32 bytes): a proof then transforms only l r o z (pi, pi2_j); without it they are recomputed per proof from
 * the resident coefficients.  The two settings give the same bytes.
 * NLX_E_RANGE: log_n, unknown flags, n_commit, n_srs < n + 3, a scalar not below r, a row outside H, rows that do not ascend;
 * NLX_E_INVAL: a NULL pointer, a selector that disagrees with its rows.  The key belongs to its context and must be destroyed
 * before it. */
typedef struct nlx_bn254_plonk_key nlx_bn254_plonk_key;
typedef struct {
    uint32_t log_n;
    uint32_t flags;
    const uint64_t *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;
    const uint64_t *k1, *k2, *coset_shift;
    const uint64_t* srs; uint64_t n_srs;
    uint32_t n_commit;
    const uint64_t *const *qcp;
    const uint64_t* n_committed;
    const uint32_t* committed_rows;
    const uint32_t* commit_rows;
    uint32_t last_row;
} nlx_bn254_plonk_key_desc;
#define NLX_BN254_PLONK_KEY_COSET 0x400u
int32_t nlx_bn254_plonk_key_create(nlx_ctx* ctx, const nlx_bn254_plonk_key_desc* desc, nlx_bn254_plonk_key** out);
void nlx_bn254_plonk_key_destroy(nlx_bn254_plonk_key* key);
/* out[0] = bytes the key keeps resident in HBM, out[1] = n, out[2] = k, out[3] = the committed rows of all sets, out[4] = 1 if
 * the coset values are resident. */
#define NLX_BN254_PLONK_KEY_INFO_WORDS 5
int32_t nlx_bn254_plonk_key_info(const nlx_bn254_plonk_key* key, uint64_t out[NLX_BN254_PLONK_KEY_INFO_WORDS]);
/* The verifying key's points: (8 + k) x 8 words in the order the transcript binds them: s1 s2 s3 ql qr qm qo qk qcp_0 .. */
int32_t nlx_bn254_plonk_key_commitments(const nlx_bn254_plonk_key* key, uint64_t* out);
size_t nlx_bn254_plonk_proof_bytes(const nlx_bn254_plonk_key* key);   /* 552 + 64 k */
/* The solver's hint of commitment j < k, while the witness is still being solved: of l (n x 4 words, host or device) only the
 * committed rows of set j are read.  pi2_j on H = those L values, then blinding[0] on the commitment row, THEN blinding[1] on
 * last_row (the second write stands where the two coincide); point_out = [PI2_j] (G1Affine words), c_out =
 * hash_to_field([PI2_j].Marshal(), "BSB22-Plonk") (Montgomery words): the value the circuit expects on the L wire of row i_j.
 * blinding: host, two elements.  NLX_E_INVAL on a key without commitments, NLX_E_RANGE for j >= k. */
int32_t nlx_bn254_plonk_commit(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, uint32_t j, const uint64_t* l, const uint64_t* blinding,
                               uint64_t point_out[8], uint64_t c_out[4]);
/* One proof in gnark's Proof.WriteTo bytes (552 + 64 k of them).  l, r, o: the wires on H, n x 4 words each, host or device.
 * public_inputs: host, n_public x 4 words.  blinding: host, nine elements (l 2, r 2, o 2, z 3); commit_blinding: host, 2 k
 * elements (commitment j: [2 j] on its row, [2 j + 1] on last_row), NULL exactly when k = 0.  The library draws no randomness.
 * Every pi2_j is recomputed from the finished wires.  NLX_E_INVAL with a message, nothing written: l[commit_rows[j]] != c_j (also
 * what a committed value changed after the hint gives), a grand product that does not close, a quotient whose coefficients
 * from 3 n + 6 up do not vanish.  NLX_E_RANGE: proof_cap too small, a scalar not below r.  Kernel-timing names, one per round:
 * bn254_plonk_prove_commit, _wires, _z, _quotient, _evals, _open. */
int32_t nlx_bn254_plonk_prove(nlx_ctx* ctx, const nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                              const uint64_t* public_inputs, uint64_t n_public, const uint64_t* blinding, const uint64_t* commit_blinding,
                              uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
/* The witness checker of the resident prover: which row, which copy or which commitment a witness breaks (DESIGN.md section 35;
 * the counterpart of nlx_circuit_check_witness over BN254 Fr).  Exact on the rows of H - no challenge, no random combination:
 *   GATES    row i is bad iff ql l + qr r + qm l r + qo o + qk + PI_i + m_i l != 0 with the selectors at w^i, PI_i =
 *            public_inputs[i] for i < n_public, c_j on commitment row i_j, 0 elsewhere, m_i = the number of commitment sets whose
 *            committed rows contain i.  The c_j are known only when COMMITS runs in the same call: without it the k commitment
 *            rows are left out and counted in gate_rows_skipped.  "First" = the lowest row.
 *   COPIES   cell (wire, row) is bad iff its value differs from the value at sigma(wire, row); both ends of a broken copy are
 *            bad cells.  "First" = the lowest row, then the lowest wire (0 = L, 1 = R, 2 = O); copy_to_* is the decoded partner.
 *   COMMITS  per commitment j, as the prover's round 0: pi2_j from l and commit_blinding, [PI2_j] by the key's MSM, c_j =
 *            hash_to_field([PI2_j].Marshal(), "BSB22-Plonk"), compared with l[i_j].  Dropped from `checked` on a key with k = 0.
 * NLX_BN254_PLONK_CHECK_ALL reports satisfied exactly when nlx_bn254_plonk_prove accepts the same arguments; where the prover
 * refuses, the first finding of the corresponding kind exists (grand product <-> copies, quotient degree <-> gates, commitment
 * message <-> commits).  Field elements of the report are four CANONICAL words (not Montgomery). */
#define NLX_BN254_PLONK_CHECK_GATES   1u
#define NLX_BN254_PLONK_CHECK_COPIES  2u
#define NLX_BN254_PLONK_CHECK_COMMITS 4u   /* keys with k > 0 */
#define NLX_BN254_PLONK_CHECK_ALL     7u
typedef struct {
    uint32_t checked;      /* the NLX_BN254_PLONK_CHECK_* bits that ran */
    uint32_t satisfied;    /* 1: nothing found by any check that ran */
    uint64_t gate_rows_bad;
    uint32_t gate_rows_skipped, gate_row;
    uint64_t gate_value[4];            /* the constraint's value on gate_row */
    uint64_t copy_cells_bad;
    uint32_t copy_row, copy_wire, copy_to_row, copy_to_wire;
    uint64_t copy_value[4], copy_to_value[4];
    uint32_t commits_bad, commit_index, commit_row, commit_pad_;
    uint64_t commit_have[4] /* l[i_j] */, commit_want[4] /* c_j */;
    uint64_t cache_bytes;              /* what the key now keeps for later checks */
} nlx_bn254_plonk_witness_report;
/* l, r, o, public_inputs, commit_blinding: as nlx_bn254_plonk_prove takes them; never written.  The wires' words must be
 * reduced Montgomery values (below r), as every fr.Element is: they are not range-checked, here or in the prover, and the copy
 * pass compares words, so x and x + r would count as different values.  what: a non-empty set of
 * NLX_BN254_PLONK_CHECK_* bits.  Returns NLX_OK whenever the check ran - the verdict is in *report, which is zero-filled before
 * anything else happens; when report->satisfied == 0, nlx_last_error holds one line naming the row and value, the two cells of
 * the copy and their values, or the commitment.  NLX_E_INVAL: a NULL argument, `what` outside 1 .. 7, COMMITS on a key with
 * k > 0 without commit_blinding, a sigma value that lies in no coset {1, k1, k2} H (its position is in the message, nothing is
 * cached), 1, k1^n, k2^n not pairwise distinct.  NLX_E_RANGE: a scalar not below r, more public inputs than rows.
 * The selectors' values on H are made per check in the call's scratch (five forward transforms of size n) and not kept; the
 * first COPIES check of a key decodes s1 s2 s3 into one 32-bit word per cell (12 n bytes), which the key keeps until
 * nlx_bn254_plonk_key_destroy - hence the non-const key. */
int32_t nlx_bn254_plonk_check_witness(nlx_ctx* ctx, nlx_bn254_plonk_key* key, const uint64_t* l, const uint64_t* r, const uint64_t* o,
                                      const uint64_t* public_inputs, uint64_t n_public, const uint64_t* commit_blinding, uint32_t what,
                                      nlx_bn254_plonk_witness_report* report);
/* gnark's plonk.Setup(spr, srs) on the device, from the constraints (csrc/bn254_plonk_setup.hip).  The
 * rules are those of tools/gnark_plonk_setup_model.py, the place of record - recalled from gnark v0.9 backend/plonk/bn254
 * setup.go, UNPINNED like the rest of the PLONK half: parity with gnark-produced keys is not claimed.  With N = n_public +
 * n_constraints and n = 2^log_n >= N:
 *   rows         row i < n_public: ql = -1, the other selectors 0, cells L = variable i, R = O = variable 0; row n_public + c is
 *                constraint c: selectors coeffs[ql[c]] .., cells (xa[c], xb[c], xc[c]); rows N .. n - 1: selectors 0, cells variable 0.
 *                qk holds the constraints' constants only: public inputs enter at proof time.
 *   commitments  commitment j names committed CONSTRAINT indices (ascending) and one commitment constraint; the key's rows are
 *                those indices + n_public, qcp_j is 1 on j's committed rows, last_row = N - 1.  The constraints' own selectors
 *                (ql = -1 on those rows) are the circuit's business.
 *   permutation  over positions p = col * n + row (col 0 1 2 = L R O): walking p upward, perm[p] = the previous position holding
 *                the same variable; a variable's first position takes its last one; a variable seen once maps to itself.
 *   sigma        s_col(w^row) = id[perm[col * n + row]], id[c * n + i] = (1, k1, k2)[c] * w^i (gnark: k1 = u, k2 = u^2).
 * The descriptor:
 *   log_n        0: the smallest log_n >= 3 with 2^log_n >= N; else 3 .. 26
 *   xa xb xc     n_constraints variable ids each; ql qr qm qo qk: n_constraints coefficient ids each (host or device)
 *   coeffs       n_coeffs x 4 Montgomery words (host or device); k1, k2, coset_shift: HOST, four Montgomery words each
 *   n_commit     k <= NLX_BN254_PLONK_MAX_COMMIT; n_committed: k counts, committed: the k sets of constraint indices
 *                concatenated, commit_constraint: k constraint indices (host or device)
 * Refused on the host before anything is allocated on the device, the message naming the cause and the index - NLX_E_RANGE:
 * flags other than NLX_BN254_MONTGOMERY, log_n outside 3 .. 26 or too small for N, n_variables = 0 or < n_public, a variable id
 * >= n_variables, a coefficient id >= n_coeffs, a coefficient, k1, k2 or coset_shift not below r, n_commit > 4, a committed or
 * commitment constraint index >= n_constraints, a set that does not ascend; NLX_E_INVAL: a NULL array that is needed.
 * The result keeps on the device the trace on H (ql qr qm qo qk s1 s2 s3 qcp_j by values), the 3 n cells as variable ids and
 * the permutation; it belongs to its context and must be destroyed before it.  Kernel-timing names: bn254_plonk_setup_rows,
 * _sort, _perm, _sigma; bn254_plonk_setup_wires; bn254_kzg_srs_powers.
 * (The type is known by its struct tag only: the name is the entry point's.) */
struct nlx_bn254_plonk_setup;
typedef struct {
    uint32_t log_n;
    uint32_t flags;                     /* NLX_BN254_MONTGOMERY */
    uint64_t n_variables, n_public, n_constraints;
    const uint32_t *xa, *xb, *xc;
    const uint32_t *ql, *qr, *qm, *qo, *qk;
    const uint64_t* coeffs; uint64_t n_coeffs;
    const uint64_t *k1, *k2, *coset_shift;
    uint32_t n_commit;
    const uint64_t* n_committed;
    const uint32_t* committed;
    const uint32_t* commit_constraint;
} nlx_bn254_plonk_setup_desc;
int32_t nlx_bn254_plonk_setup(nlx_ctx* ctx, const nlx_bn254_plonk_setup_desc* desc, struct nlx_bn254_plonk_setup** out);
void nlx_bn254_plonk_setup_destroy(struct nlx_bn254_plonk_setup* setup);
/* out[0] = n, out[1] = log_n, out[2] = k, out[3] = N, out[4] = the variables that occur in a cell, out[5] = the cells of the
 * variable that occurs most often (the longest cycle of the permutation). */
#define NLX_BN254_PLONK_SETUP_INFO_WORDS 6
int32_t nlx_bn254_plonk_setup_info(const struct nlx_bn254_plonk_setup* setup, uint64_t out[NLX_BN254_PLONK_SETUP_INFO_WORDS]);
/* One array of the result copied to `out` (host or device).  The polynomials: n x 4 Montgomery words, NLX_PLONK_SETUP_QCP0 + j
 * for j < k; CELLS: 3 n variable ids (uint32, L then R then O); PERMUTATION: 3 n positions; SIGMA_CELLS: the permutation in the
 * witness checker's encoding, col << 30 | row.  NLX_E_RANGE: an unknown `which`. */
enum {
    NLX_PLONK_SETUP_QL = 0, NLX_PLONK_SETUP_QR = 1, NLX_PLONK_SETUP_QM = 2, NLX_PLONK_SETUP_QO = 3, NLX_PLONK_SETUP_QK = 4,
    NLX_PLONK_SETUP_S1 = 5, NLX_PLONK_SETUP_S2 = 6, NLX_PLONK_SETUP_S3 = 7, NLX_PLONK_SETUP_QCP0 = 8,
    NLX_PLONK_SETUP_CELLS = 12, NLX_PLONK_SETUP_PERMUTATION = 13, NLX_PLONK_SETUP_SIGMA_CELLS = 14
};
int32_t nlx_bn254_plonk_setup_read(const struct nlx_bn254_plonk_setup* setup, uint32_t which, void* out);
/* The resident proving key of this setup: a nlx_bn254_plonk_key_desc of device pointers through nlx_bn254_plonk_key_create (the
 * one creation path; srs, n_srs and what it refuses as there), key_flags = 0 or NLX_BN254_PLONK_KEY_COSET.  The key then receives
 * the decoded permutation: its first NLX_BN254_PLONK_CHECK_COPIES reports cache_bytes = 12 n and runs no decode.  The key is the
 * caller's, independent of `setup`. */
int32_t nlx_bn254_plonk_setup_key(const struct nlx_bn254_plonk_setup* setup, const uint64_t* srs, uint64_t n_srs, uint32_t key_flags,
                                  nlx_bn254_plonk_key** out);
/* The solver's last step: l[row] = values[cell of (L, row)], r and o likewise.  values: n_variables x 4 words (host or device;
 * the public inputs are the first n_public); l, r, o: n x 4 words each, host or device.  A `values` shorter than n_variables
 * cannot be detected: only NULL is refused (NLX_E_INVAL). */
int32_t nlx_bn254_plonk_setup_wires(nlx_ctx* ctx, const struct nlx_bn254_plonk_setup* setup, const uint64_t* values, uint64_t* l, uint64_t* r,
                                    uint64_t* o);
/* gnark's witness solver on the device, by levels (csrc/bn254_plonk_solve.hpp and .hip): from the public
 * and secret inputs of a setup's constraint system to the whole variable vector that nlx_bn254_plonk_setup_wires takes.  The
 * rules are those of tools/gnark_plonk_solve_model.py, the place of record - recalled from gnark v0.9 (constraint/bn254/solver.go)
 * and UNPINNED: parity with gnark's solver is not claimed.
 *   given        variables [0, n_public + n_secret)
 *   counting     a cell counts only where its coefficient can determine it: L when ql != 0 or qm != 0, R when qr != 0 or
 *                qm != 0, O when qo != 0
 *   skipped      the committed constraints of every commitment and each commitment's own constraint
 *   constraints  in index order: with no unassigned counting variable a check (ql l + qr r + qm l r + qo o + qk == 0), with one
 *                (in one cell) it is solved: l = -(qr r + qo o + qk) / (ql + qm r), r likewise, o = -(ql l + qr r + qm l r + qk) / qo
 *   hints        hint i runs in front of constraint hint_before[i] (non-descending); inputs hint_in[hint_in_off[i] ..
 *                hint_in_off[i + 1]), outputs hint_out[hint_out_off[i] .. hint_out_off[i + 1]) (variable ids; the offset arrays hold
 *                n_hints + 1 entries).  NLX_PLONK_HINT_INV_ZERO: 1 in, 1 out, x^-1 or 0 for 0.  _N_BITS: 1 in, 1 .. 256 outs, out
 *                i = bit i of the canonical integer.  _QUO_REM64: 1 in, hint_param[i] = m in [1, 2^64), outs q, r with
 *                canonical(x) = q m + r, 0 <= r < m.  The commitments' hints (c_j onto the L variable of commitment j's own
 *                constraint, in front of that constraint) are implied by the setup and are not listed.
 * Create makes the schedule on the host - per constraint its form (NLX_PLONK_SOLVE_FORM_*), its level (1 + the highest level
 * among the assigners of its operands; inputs are level 0) and the variable it assigns - and refuses, before anything is
 * allocated on the device, NLX_E_INVAL with a message naming the constraint or hint: two unassigned counting variables in one
 * constraint; the unassigned variable in two counting cells; a hint input not assigned by `before`; a hint output that is given
 * or assigned twice; `before` descending or > n_constraints; NLX_E_RANGE: flags other than NLX_BN254_MONTGOMERY, n_public +
 * n_secret > n_variables, an unknown hint kind or a variable id out of range.  A variable nothing assigns stays 0 and is counted.
 * All arrays of the descriptor are HOST arrays.  The solver keeps its own copies of all it needs: it is independent of `setup`
 * once created, belongs to the setup's context and must be destroyed before it.  NLX_BN254_PLONK_SOLVER_NO_FUSE: one launch per
 * level (the A/B run and the parity test); by default a run of consecutive levels of at most NLX_BN254_PLONK_SOLVER_FUSE items
 * each executes in one launch of one workgroup, with a workgroup barrier between levels. */
struct nlx_bn254_plonk_solver;
#define NLX_PLONK_HINT_INV_ZERO 4u
#define NLX_PLONK_HINT_N_BITS 5u
#define NLX_PLONK_HINT_QUO_REM64 6u
#define NLX_PLONK_SOLVE_FORM_CHECK 0u
#define NLX_PLONK_SOLVE_FORM_L 1u
#define NLX_PLONK_SOLVE_FORM_R 2u
#define NLX_PLONK_SOLVE_FORM_O 3u
#define NLX_PLONK_SOLVE_FORM_SKIPPED 8u
#define NLX_BN254_PLONK_SOLVER_NO_FUSE 0x800u
#define NLX_BN254_PLONK_SOLVER_FUSE 1024u
typedef struct {
    uint64_t n_secret;
    uint32_t flags, n_hints;            /* NLX_BN254_MONTGOMERY, optionally | NLX_BN254_PLONK_SOLVER_NO_FUSE */
    const uint32_t *hint_kind, *hint_before;
    const uint64_t *hint_param;
    const uint64_t *hint_in_off, *hint_out_off;
    const uint32_t *hint_in, *hint_out;
} nlx_bn254_plonk_solver_desc;
int32_t nlx_bn254_plonk_solver_create(nlx_ctx* ctx, const struct nlx_bn254_plonk_setup* setup, const nlx_bn254_plonk_solver_desc* desc,
                                      struct nlx_bn254_plonk_solver** out);
void nlx_bn254_plonk_solver_destroy(struct nlx_bn254_plonk_solver* solver);
/* out[0] = levels, [1] = the widest level's items, [2] = launches per solve (level and fused kernels; a commitment's hint adds
 * its scatter and the commit call), [3] = fused runs, [4 .. 11] = items per form (check, solve L, R, O, INV_ZERO, N_BITS,
 * QUO_REM64, COMMIT), [12] = constant divisors (inverted once, at creation), [13] = value-dependent divisors (inverted in-lane,
 * per solve), [14] = variables left unassigned, [15] = resident bytes. */
#define NLX_BN254_PLONK_SOLVER_INFO_WORDS 16
int32_t nlx_bn254_plonk_solver_info(const struct nlx_bn254_plonk_solver* solver, uint64_t out[NLX_BN254_PLONK_SOLVER_INFO_WORDS]);
/* The schedule per constraint, n_constraints uint32 to a HOST array: the level (0 where skipped), the form, or the variable it
 * assigns (0xFFFFFFFF where none).  NLX_E_RANGE: an unknown `which`. */
enum { NLX_PLONK_SOLVER_LEVEL = 0, NLX_PLONK_SOLVER_FORM = 1, NLX_PLONK_SOLVER_ASSIGNS = 2 };
int32_t nlx_bn254_plonk_solver_read(const struct nlx_bn254_plonk_solver* solver, uint32_t which, void* out);
#define NLX_PLONK_SOLVE_DIV_ZERO 1u      /* the divisor of a solving constraint is 0, whatever the numerator */
#define NLX_PLONK_SOLVE_UNSATISFIED 2u   /* a check-only constraint is nonzero */
typedef struct {
    uint32_t solved;               /* 1: every item ran and nothing failed */
    uint32_t kind;                 /* 0, or NLX_PLONK_SOLVE_* of the failing constraint of lowest index */
    uint32_t constraint, level;    /* that constraint and its level */
    uint64_t value[4];             /* the numerator (DIV_ZERO) or the constraint's value (UNSATISFIED), CANONICAL words */
    uint64_t failures;             /* constraints that failed on clean operands */
    uint64_t poisoned_variables;   /* variables downstream of a failure: not computed */
    uint32_t levels_run, launches;
} nlx_bn254_plonk_solve_report;
/* One solve.  inputs: (n_public + n_secret) x 4 Montgomery words, host or device, each below r (else NLX_E_RANGE, nothing
 * written).  key: the setup's resident key, required exactly when the setup carries commitments (k > 0), else NLX_E_INVAL; it
 * must belong to the same n.  commit_blinding: HOST, 2 k elements (commitment j: [2 j] on its row, [2 j + 1] on last_row), the
 * ones the proof will use; NULL exactly when k = 0.  values_out: n_variables x 4 words, host or device - what
 * nlx_bn254_plonk_setup_wires takes; poisoned and unassigned variables come as 0.  commit_points_out: HOST, k x 8 words, the
 * [PI2_j] (may be NULL).  Nothing in the call draws randomness.
 * A failing constraint poisons the variable it would assign; an item with a poisoned operand fails nothing and poisons what it
 * would assign (a commitment with a poisoned input is skipped), so the reported failure is the one a sequential solver stops
 * at, however the levels interleave.  Returns NLX_OK whenever the solve ran - the verdict is in *report (zero-filled first);
 * with report->solved == 0 nlx_last_error holds one line naming the constraint.  Kernel-timing names:
 * bn254_plonk_solve_levels, _fused, _commit. */
int32_t nlx_bn254_plonk_solver_solve(nlx_ctx* ctx, const struct nlx_bn254_plonk_solver* solver, const uint64_t* inputs,
                                     const nlx_bn254_plonk_key* key, const uint64_t* commit_blinding, uint64_t* values_out,
                                     uint64_t* commit_points_out, nlx_bn254_plonk_solve_report* report);
/* A TEST SRS from its trapdoor (gnark-crypto kzg.NewSRS(size, tau); whoever knows tau forges openings): g1_out[i] = [tau^i]_1 for
 * i < n (n x 8 words, host or device), g2_out = [1]_2, [tau]_2 (2 x 16 words, HOST, may be NULL).  tau: HOST, four Montgomery
 * words.  The powers are computed on the device (lane i from a table of tau^(2^b)), then one fixed-base pass per group.
 * NLX_E_RANGE: tau = 0, tau not below r, n = 0 or n > 2^27. */
int32_t nlx_bn254_kzg_srs(nlx_ctx* ctx, const uint64_t* tau, uint64_t n, uint64_t* g1_out, uint64_t* g2_out);
/* n_polys <= 16 polynomials at ONE point in one pass: polys = host array of pointers to lens[i] x 4 words (coefficients, natural
 * order, host or device; 1 <= lens[i] <= 2^28, the lengths may differ), point: host; out: host, n_polys x 4 words.  Kernel-timing
 * name "bn254_fr_eval_many". */
int32_t nlx_bn254_fr_eval_many(nlx_ctx* ctx, uint32_t n_polys, const uint64_t* const* polys, const uint64_t* lens, const uint64_t point[4],
                               uint64_t* out);
/* gnark-crypto fr.Hash(msg, dst, 1)[0] as Montgomery words: RFC 9380 expand_message_xmd over SHA-256 to 48 bytes, read
 * big-endian, mod r.  Host only, needs no context; dst_len <= 255. */
int32_t nlx_bn254_hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint64_t out[4]);

/* ---- f.4: the optimal ate pairing on BN254 and the Groth16 verifier that stands on it (csrc/bn254_pairing.hpp / .hip; DESIGN.md
 * section 30; the big-integer model is tools/bn254_pairing_model.py).
 * The n reduced pairings e(g1[i], g2[i]).  g1: n x 8 words (G1Affine), g2: n x 16 words (G2Affine), Montgomery as for the MSM, (0, 0)
 * = the point at infinity (the pairing is then 1, as in gnark-crypto); host or device.  gt_out: n x 48 words, host or device:
 * twelve Fq elements in gnark-crypto's E12 order (C0.B0.A0, C0.B0.A1, C0.B1.A0, ... C1.B2.A1), four words each - Montgomery with
 * flags = NLX_BN254_MONTGOMERY, canonical integers with flags = 0.  Every coordinate must be below q, every point on its curve and
 * every G2 point in the subgroup of order r: otherwise NLX_E_RANGE, the message naming the first offending pair, and nothing is
 * written.  n <= 2^20.  Kernel-timing names "bn254_pairing_points", "bn254_pairing_miller", "bn254_pairing_final_exp". */
int32_t nlx_bn254_pairing(nlx_ctx* ctx, const uint64_t* g1, const uint64_t* g2, size_t n, uint32_t flags, uint64_t* gt_out);
/* n_checks product checks: ok_out[c] = 1 if prod_i e(P_i, Q_i) = 1 over check c's n_pairs[c] pairs, else 0.  g1 / g2 hold the
 * pairs of all checks back to back (host or device); n_pairs and ok_out are host arrays.  One Miller launch over all pairs and one
 * final exponentiation per check, whatever the number of pairs; a check of no pairs, or of pairs at infinity, gives 1.  The
 * points are checked as for nlx_bn254_pairing.  flags must be 0; at most 2^20 pairs in all. */
int32_t nlx_bn254_pairing_check(nlx_ctx* ctx, const uint64_t* g1, const uint64_t* g2, const uint32_t* n_pairs, size_t n_checks, uint32_t flags,
                                uint8_t* ok_out);
/* gnark's groth16 VerifyingKey resident on the device.  All points are gnark-crypto's words (Montgomery), all arrays host.
 *   n_public        the public wires, the constant wire ONE included (>= 1)
 *   n_commitments   k <= NLX_BN254_GROTH16_MAX_COMMITMENTS Bsb22 / Pedersen commitments
 *   ic, n_ic        G1.K: n_public points for the public wires, then one per commitment wire; n_ic = n_public + k
 *   n_hashed, hashed   PublicAndCommitmentCommitted: k counts, then the sets concatenated - ids into ic's index space (an id
 *                   n_public + i names commitment i's wire and must have i < the commitment that hashes it)
 *   pedersen_g, pedersen_g_root_sigma_neg   the Pedersen verifying key, e(C, GRootSigmaNeg) e(Pok, G) = 1 ([1]_2 and [-1 / sigma]_2 in gnark's setup); read only for k > 0
 * Creation checks every point as nlx_bn254_pairing does, computes e(alpha, beta) once on the device (gnark's Precompute) and keeps
 * it resident next to -gamma, -delta and ic.  NLX_E_RANGE: a point that fails its checks, n_public = 0, k out of range, n_ic that
 * disagrees, an id out of range.  The key belongs to its context and must be destroyed before it. */
typedef struct nlx_bn254_groth16_vk nlx_bn254_groth16_vk;
typedef struct {
    const uint64_t *g1_alpha, *g2_beta, *g2_gamma, *g2_delta;
    const uint64_t* ic; uint64_t n_ic;
    uint32_t n_public, n_commitments;
    const uint32_t* n_hashed;
    const uint32_t* hashed;
    const uint64_t *pedersen_g, *pedersen_g_root_sigma_neg;
} nlx_bn254_groth16_vk_desc;
int32_t nlx_bn254_groth16_vk_create(nlx_ctx* ctx, const nlx_bn254_groth16_vk_desc* desc, nlx_bn254_groth16_vk** out);
void nlx_bn254_groth16_vk_destroy(nlx_bn254_groth16_vk* vk);
/* gnark's groth16.Verify on the bytes of Proof.WriteTo (164 + 32 k; what bn254_groth16.proof_bytes writes).  public_inputs:
 * (n_public - 1) x 4 words per proof (wires 1 .. n_public - 1, Montgomery, host), the proofs' back to back in the batch call;
 * proofs / lens: host.  The return value says whether the check RAN (conventions of nlx_verify): NLX_OK with the answer in the
 * verdict (zero-filled first), and on a rejection nlx_last_error holds one line naming the first rejected proof; NLX_E_INVAL for
 * NULL arguments, NLX_E_RANGE for a public input that is not below r.  A proof gets the first reason that applies, in gnark's
 * order:
 *   NLX_BN254_VERIFY_MALFORMED  a wrong length or commitment count, a bad flag byte, a coordinate >= q, an x with no y on the
 *                               curve, Bs outside the subgroup; index = 0 Ar, 1 Bs, 2 Krs, 3 + j C_j, 3 + k Pok (0 for the length)
 *   NLX_BN254_VERIFY_PEDERSEN   e(sum_j rho^j C_j, GRootSigmaNeg) e(Pok, G) != 1
 *   NLX_BN254_VERIFY_PAIRING    e(Ar, Bs) e(IC_0 + sum w_i IC_i + sum C_j, -gamma) e(Krs, -delta) != e(alpha, beta)
 * Host: decoding, the square roots, the commitment challenges and rho.  Device: the subgroup test of Bs, the public sum, 3 (+ 2)
 * Miller loops per proof and the final exponentiations - the same five launches for one proof and for a batch (kernel-timing
 * names "bn254_groth16_ksum", "bn254_pairing_points", "bn254_pairing_miller", "bn254_pairing_final_exp"). */
#define NLX_BN254_VERIFY_ACCEPT 0u
#define NLX_BN254_VERIFY_MALFORMED 1u
#define NLX_BN254_VERIFY_PEDERSEN 2u
#define NLX_BN254_VERIFY_PAIRING 3u
typedef struct { uint32_t accepted, reason, index; } nlx_bn254_verdict;
int32_t nlx_bn254_groth16_verify(const nlx_bn254_groth16_vk* vk, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                                 nlx_bn254_verdict* verdict);
int32_t nlx_bn254_groth16_verify_batch(const nlx_bn254_groth16_vk* vk, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                                       const uint64_t* public_inputs, nlx_bn254_verdict* verdicts);

/* gnark's plonk VerifyingKey resident on the device and gnark v0.9 plonk.Verify on the bytes of Proof.WriteTo (552 + 64 k; what
 * nlx_bn254_plonk_prove writes) - csrc/bn254_plonk_verify.hip, DESIGN.md section 32.  The specification of every byte and formula
 * is tools/gnark_bsb22_model.py; parity with gnark's own Verify is UNPINNED like the rest of f.4.  All arrays host.
 *   log_n 3 .. 26, n_public <= n, n_commit = k <= NLX_BN254_PLONK_MAX_COMMIT
 *   k1, k2          four Montgomery words each, below r (as in nlx_bn254_plonk_key_desc)
 *   commitments     (8 + k) x 8 words in nlx_bn254_plonk_key_commitments' order: s1 s2 s3 ql qr qm qo qk qcp_0 ..
 *   commit_rows     k rows i_j < n; read only for k > 0
 *   g1              the SRS's first point (gnark vk.Kzg.G1); g2, g2_tau: [1]_2 and [tau]_2, 16 words each
 * Creation checks every point as nlx_bn254_groth16_vk_create does (the two G2 points in the subgroup) and keeps the points
 * resident.  NLX_E_RANGE: a point that fails (the message names it), log_n, k, a row not below n, n_public > n, k1 / k2 not below
 * r; NLX_E_INVAL: a NULL pointer.  The key belongs to its context and must be destroyed before it. */
typedef struct nlx_bn254_plonk_vk nlx_bn254_plonk_vk;
typedef struct {
    uint32_t log_n, n_public, n_commit;
    const uint64_t *k1, *k2;
    const uint64_t* commitments;
    const uint32_t* commit_rows;
    const uint64_t *g1;
    const uint64_t *g2, *g2_tau;
} nlx_bn254_plonk_vk_desc;
int32_t nlx_bn254_plonk_vk_create(nlx_ctx* ctx, const nlx_bn254_plonk_vk_desc* desc, nlx_bn254_plonk_vk** out);
void nlx_bn254_plonk_vk_destroy(nlx_bn254_plonk_vk* vk);
/* The calling conventions are nlx_bn254_groth16_verify's: the return value says whether the check RAN, the verdict is zero-filled
 * first, on a rejection nlx_last_error holds one line naming the first rejected proof; NLX_E_INVAL for NULL arguments, NLX_E_RANGE
 * for a public input not below r (naming the proof and the input).  public_inputs: n_public x 4 Montgomery words per proof, the
 * proofs' back to back.  A proof gets the first reason that applies:
 *   NLX_BN254_VERIFY_MALFORMED  index 0: the length, or a count that does not fit (commitment count != k, claimed-value count
 *                               != 7 + k); after the length the fields are judged in byte order.  Points (a bad flag byte, a
 *                               coordinate >= q, an x with no y; a compressed point at infinity is a valid point): 0 L, 1 R, 2 O,
 *                               3 Z, 4 .. 6 H1 .. H3, 7 + j PI2_j, 7 + k the batched opening's H, 8 + k the shifted opening's H.
 *                               Values not below r: 9 + k + i claimed value i, 16 + 2 k the shifted value
 *   NLX_BN254_VERIFY_ALGEBRAIC  gnark's "algebraic relation does not hold": lin(zeta) + PI(zeta) - alpha b (o + gamma) z_w -
 *                               alpha^2 L_1(zeta) != folded_h(zeta) (zeta^n - 1), PI with the Bsb22 terms; an inverse of 0 is 0
 *   NLX_BN254_VERIFY_PAIRING    the two openings folded into one check of two pairs fail:
 *                               e(D_f + lambda Z - (v_f + lambda z_w) G + zeta H_b + lambda zeta w H_z, [1]_2)
 *                               e(-(H_b + lambda H_z), [tau]_2) != 1
 * The lambda rule.  gnark's kzg.BatchVerifyMultiPoints draws lambda from crypto/rand; this library draws no randomness: lambda =
 * nlx_bn254_hash_to_field(zeta || gamma' || Z.Marshal() || H_b.Marshal() || H_z.Marshal() || v_f || z_w, dst
 * "nlx-plonk-kzg-fold") with the scalars as 32 big-endian bytes, 1 in place of 0.  gamma' (FoldProof's challenge) stands in the
 * message for the folded digest D_f = sum gamma'^i D_i: it is itself a hash over zeta, every D_i and every claimed value, and D_f is
 * never computed on its own - it is spelled out inside the one combination of the left point.  Any nonzero lambda is a valid run of
 * gnark's verifier, so acceptance equals gnark's up to a probability of 1 / r.
 * Host: decoding, square roots, the transcript, the Bsb22 hashes, every scalar (one inversion per proof), the relation.  Device:
 * two launches of the segmented combination (two segments a proof each), the Miller loops of two pairs a proof, one final
 * exponentiation a proof - the same launches for one proof and for a batch of up to 2^17 (kernel-timing names
 * "bn254_plonk_verify_lincomb_a", "bn254_plonk_verify_lincomb_b", "bn254_pairing_miller", "bn254_pairing_final_exp"). */
#define NLX_BN254_VERIFY_ALGEBRAIC 4u
int32_t nlx_bn254_plonk_verify(const nlx_bn254_plonk_vk* vk, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                               nlx_bn254_verdict* verdict);
int32_t nlx_bn254_plonk_verify_batch(const nlx_bn254_plonk_vk* vk, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                                     const uint64_t* public_inputs, nlx_bn254_verdict* verdicts);

/* ---- f.4: gnark-crypto's point bytes, decoded and encoded on the device (csrc/bn254_codec.hpp / .hip).
 * What kzg.SRS.WriteTo and groth16.ProvingKey.WriteTo / WriteRawTo are made of: G1Affine.Bytes() (32 bytes) and G2Affine.Bytes()
 * (64) with flags = NLX_BN254_POINTS_COMPRESSED, RawBytes() (64 and 128) with NLX_BN254_POINTS_RAW; exactly one of the two must
 * be set, else NLX_E_RANGE.  The place of record for every byte rule is tools/gnark_bytes_model.py; the rules are recalled from
 * gnark v0.9 / gnark-crypto and UNPINNED like the rest of f.4.  In short: coordinates are big-endian canonical integers below q,
 * G2 as X.A1 || X.A0 (|| Y.A1 || Y.A0); the top two bits of the first byte are 00 (raw), 10 / 11 (compressed, the smaller / larger
 * y: y > (q - 1) / 2, over Fq2 decided on A1, on A0 when A1 is zero) or 01: the point at infinity, 0x40 and zeros in both modes
 * and (0, 0) in words.  Words are G1Affine (8) / G2Affine (16: X.A0 X.A1 Y.A0 Y.A1), Montgomery.
 * Pointers may be host or device; input and output must not overlap (NLX_E_INVAL).  n = 0: NLX_OK, nothing is written; n <= 2^28.
 * Decode: one lane per point - the flag for the mode, every coordinate below q, compressed: y = (x^3 + b)^((q + 1) / 4) and its
 * check (over Fq2 two such chains), raw: the curve equation; G2: the subgroup test of nlx_bn254_pairing unless
 * NLX_BN254_POINTS_NO_SUBGROUP.  A point gets the first status that applies (NLX_BN254_POINT_*: BAD_INFINITY = flag 01 with any
 * other bit set; OFF_CURVE = no square root, or a raw point off the curve) and a bad point all-zero words.  If any point is bad
 * the call returns NLX_E_INVAL, the message naming the lowest bad index and its reason; points_out and status_out (n words, may
 * be NULL) are written all the same.
 * Encode: does not test the curve (gnark does not); a coordinate that is not below q: NLX_E_RANGE naming the lowest such index
 * (its bytes are zero).
 * Kernel-timing names "bn254_g1_decode", "bn254_g2_decode", "bn254_g1_encode", "bn254_g2_encode"; units: points. */
#define NLX_BN254_POINTS_COMPRESSED 1u
#define NLX_BN254_POINTS_RAW 2u
#define NLX_BN254_POINTS_NO_SUBGROUP 4u /* nlx_bn254_g2_decode only */
#define NLX_BN254_POINT_OK 0u
#define NLX_BN254_POINT_BAD_FLAG 1u
#define NLX_BN254_POINT_RANGE 2u
#define NLX_BN254_POINT_BAD_INFINITY 3u
#define NLX_BN254_POINT_OFF_CURVE 4u
#define NLX_BN254_POINT_NOT_IN_SUBGROUP 5u
int32_t nlx_bn254_g1_decode(nlx_ctx* ctx, const uint8_t* bytes, uint64_t n, uint32_t flags, uint64_t* points_out, uint32_t* status_out);
int32_t nlx_bn254_g2_decode(nlx_ctx* ctx, const uint8_t* bytes, uint64_t n, uint32_t flags, uint64_t* points_out, uint32_t* status_out);
int32_t nlx_bn254_g1_encode(nlx_ctx* ctx, const uint64_t* points, uint64_t n, uint32_t flags, uint8_t* bytes_out);
int32_t nlx_bn254_g2_encode(nlx_ctx* ctx, const uint64_t* points, uint64_t n, uint32_t flags, uint8_t* bytes_out);

/* ---- a3: plonky2::fri::oracle::PolynomialBatch::{from_values, from_coeffs} ----
 * values / coeffs: n_cols x 2^log_n column-major, natural order.  The coset shift is the
 * field's multiplicative generator (plonky2 F::coset_shift()).  blinding / salting is not
 * supported (zero_knowledge = false in the standard recursion config).
 * cap_out: 2^cap_height x 4 words.  *out receives a handle that keeps coefficients, the LDE
 * table and all Merkle digests resident in HBM. */
int32_t nlx_commit_from_values(nlx_ctx* ctx, const uint64_t* values, size_t n_cols, uint32_t log_n,
                               uint32_t rate_bits, uint32_t cap_height, uint64_t* cap_out, nlx_commit** out);
int32_t nlx_commit_from_coeffs(nlx_ctx* ctx, const uint64_t* coeffs, size_t n_cols, uint32_t log_n,
                               uint32_t rate_bits, uint32_t cap_height, uint64_t* cap_out, nlx_commit** out);
/* The same with the Merkle tree's hasher chosen: NLX_HASHER_POSEIDON_GOLDILOCKS is exactly the entries above,
 * NLX_HASHER_POSEIDON_BN128 hashes leaves (hash_or_noop of the LDE row) and nodes with PoseidonBN128; its digests have the
 * Goldilocks layout, so nlx_commit_get_* / open_rows / eval_at work unchanged.  Any other value: NLX_E_RANGE.  A BN128
 * commitment cannot feed a Goldilocks transcript: nlx_quotient_eval on a Goldilocks circuit and nlx_fri_prove return
 * NLX_E_UNSUPPORTED for it (a BN128 circuit, nlx_circuit_build_hasher, and nlx_fri_prove_hasher take it).
 * Merkle levels of at most T parents run a lane-split kernel (four lanes per permutation; same digests): T is a constant of the
 * library that the environment variable NLX_PBN_QUAD_MAX_PARENTS, read at nlx_ctx_create, overrides (0 = never).
 * Kernel-timing names: "hash_lde_leaves_bn128" and "merkle_levels_bn128", units BN128 permutations. */
#define NLX_HASHER_POSEIDON_GOLDILOCKS 0
#define NLX_HASHER_POSEIDON_BN128 1
int32_t nlx_commit_from_values_hasher(nlx_ctx* ctx, const uint64_t* values, size_t n_cols, uint32_t log_n, uint32_t rate_bits,
                                      uint32_t cap_height, uint32_t hasher, uint64_t* cap_out, nlx_commit** out);
int32_t nlx_commit_from_coeffs_hasher(nlx_ctx* ctx, const uint64_t* coeffs, size_t n_cols, uint32_t log_n, uint32_t rate_bits,
                                      uint32_t cap_height, uint32_t hasher, uint64_t* cap_out, nlx_commit** out);
/* the commitment's NLX_HASHER_* (NLX_E_INVAL for NULL) */
int32_t nlx_commit_hasher(const nlx_commit* c);
void nlx_commit_destroy(nlx_commit* c);

/* PolynomialBatch.polynomials: coefficients, natural order, n_cols x n column-major. */
int32_t nlx_commit_get_coeffs(nlx_commit* c, uint64_t* coeffs_out);
/* MerkleTree.cap */
int32_t nlx_commit_get_cap(nlx_commit* c, uint64_t* cap_out);
/* MerkleTree.leaves[idx[j]] (row of the bit-reversed LDE table, n_cols words) and
 * MerkleTree::prove(idx[j]) (log2(n << rate_bits) - cap_height sibling digests, bottom-up).
 * rows_out: k x n_cols;  paths_out (may be NULL): k x path_len x 4. */
int32_t nlx_commit_open_rows(nlx_commit* c, const uint64_t* idx, size_t k, uint64_t* rows_out,
                             uint64_t* paths_out);
/* a10: PolynomialBatch polynomials evaluated at zeta in the quadratic extension
 * (OpeningSet::new's eval_commitment).  zeta: 2 words; out_ext: n_cols x 2 words. */
int32_t nlx_commit_eval_at(nlx_commit* c, const uint64_t zeta[2], uint64_t* out_ext);
/* whole LDE table in plonky2's leaf order: (n << rate_bits) x n_cols row-major (debug / tests) */
int32_t nlx_commit_get_leaves(nlx_commit* c, uint64_t* leaves_out);
/* level-major digests as in nlx_merkle_build */
int32_t nlx_commit_get_digests(nlx_commit* c, uint64_t* digests_out);

/* ===================================================================================
 * Whole-proof interface: plonky2::plonk::circuit_data / prover (a14) and its stages
 * (a8 partial products, a9 quotient, a10 openings, a11 FRI), SURVEY.md §3.4.
 * =================================================================================== */

/* gate kinds understood by the constraint combiner (plonky2::gates::*) */
#define NLX_GATE_NOOP 0          /* gates::noop::NoopGate */
#define NLX_GATE_CONSTANT 1      /* gates::constant::ConstantGate { num_consts = param0 } */
#define NLX_GATE_PUBLIC_INPUT 2  /* gates::public_input::PublicInputGate */
#define NLX_GATE_ARITHMETIC 3    /* gates::arithmetic_base::ArithmeticGate { num_ops = param0 } */
#define NLX_GATE_BASE_SUM 4      /* gates::base_sum::BaseSumGate<B = param0> { num_limbs = param1 } */
#define NLX_GATE_POSEIDON 5      /* gates::poseidon::PoseidonGate */
#define NLX_GATE_ARITHMETIC_EXT 6 /* gates::arithmetic_extension::ArithmeticExtensionGate<2> { num_ops = param0 } */
#define NLX_GATE_MUL_EXT 7        /* gates::multiplication_extension::MulExtensionGate<2> { num_ops = param0 } */
#define NLX_GATE_REDUCING 8       /* gates::reducing::ReducingGate<2> { num_coeffs = param0 } */
#define NLX_GATE_REDUCING_EXT 9   /* gates::reducing_extension::ReducingExtensionGate<2> { num_coeffs = param0 } */
#define NLX_GATE_POSEIDON_MDS 10   /* gates::poseidon_mds::PoseidonMdsGate */
#define NLX_GATE_EXPONENTIATION 11 /* gates::exponentiation::ExponentiationGate { num_power_bits = param0 } */
#define NLX_GATE_RANDOM_ACCESS 12  /* gates::random_access::RandomAccessGate { bits = param0, num_copies = param1 & 0xFFFF,
                                      num_extra_constants = param1 >> 16 } */
#define NLX_GATE_COSET_INTERPOLATION 13 /* gates::coset_interpolation::CosetInterpolationGate<2> { subgroup_bits = param0,
                                           degree = param1 } - the FRI-verifier gate of every recursive (reduce) proof */
/* plonky2x frontend::num::u32::gates (from plonky2-u32), 2-bit range-check limbs: the u32 / u64 arithmetic and
 * comparisons of nearx's header, height and stake logic (nearx/src/builder.rs ensure_height / ensure_stake ...) */
#define NLX_GATE_U32_ADD_MANY 14    /* U32AddManyGate { num_addends = param0, num_ops = param1 } */
#define NLX_GATE_U32_ARITHMETIC 15  /* U32ArithmeticGate { num_ops = param0 } */
#define NLX_GATE_U32_SUBTRACTION 16 /* U32SubtractionGate { num_ops = param0 } */
#define NLX_GATE_U32_RANGE_CHECK 17 /* U32RangeCheckGate { num_input_limbs = param0 } */
#define NLX_GATE_COMPARISON 18      /* ComparisonGate { num_bits = param0, num_chunks = param1 } */
/* gates::lookup::LookupGate / gates::lookup_table::LookupTableGate of table param0: no gate constraints; their wires feed
 * the lookup argument (vanishing_poly::check_lookup_constraints).  LookupGate slot i = wires (2i, 2i+1) = (input, output),
 * num_routed_wires / 2 slots; LookupTableGate slot i = wires (3i, 3i+1, 3i+2) = (input, output, multiplicity),
 * num_routed_wires / 3 slots. */
#define NLX_GATE_LOOKUP 19
#define NLX_GATE_LOOKUP_TABLE 20
#define NLX_GATE_KIND_MAX 20

typedef struct {
    uint32_t kind;
    uint32_t selector_index; /* selector polynomial used by this gate (gates::selectors::SelectorsInfo) */
    uint32_t group_start;    /* gate-index range [start, end) that shares the selector */
    uint32_t group_end;
    uint32_t index;          /* position in the sorted gate list = selector value on the gate's rows */
    uint32_t param0, param1;
} nlx_gate_desc;

/* CommonCircuitData + CircuitConfig + FriParams, flattened (standard_recursion_config values in
 * comments).  Same field order as the oracle's orc_circuit_desc. */
typedef struct {
    uint32_t degree_bits;
    uint32_t num_wires;              /* 135 */
    uint32_t num_routed_wires;       /* 80 */
    uint32_t num_constants;          /* 2 (gate constants per row, selectors excluded) */
    uint32_t num_challenges;         /* 2 */
    uint32_t rate_bits;              /* 3 */
    uint32_t cap_height;             /* 4 */
    uint32_t quotient_degree_factor; /* 8 */
    uint32_t num_partial_products;   /* 9 */
    uint32_t fri_pow_bits;           /* 16 */
    uint32_t fri_num_queries;        /* 28 */
    uint32_t fri_arity_bits;         /* 4 */
    uint32_t fri_final_poly_bits;    /* 5 */
    uint32_t num_selectors;
    uint32_t num_gates;
    uint32_t num_public_inputs;
    const nlx_gate_desc* gates;
    const uint64_t* k_is;            /* num_routed_wires coset shifts (host pointer) */
    uint64_t circuit_digest[4];      /* all zero: computed by nlx_circuit_build as plonky2 does */
    /* ---- lookup tables (CommonCircuitData::luts, ProverOnlyCircuitData::{lookup_rows, lut_to_lookups}) ----
     * num_luts == 0 (a zero-initialised tail): no lookup argument, the rest is ignored.  With tables:
     *  - the constants matrix carries 4 + num_luts lookup selector columns between the gate selectors and the gate
     *    constants (gates::selectors::selectors_lookup: TransSre, TransLdc, InitSre, LastLdc; selector_ends_lookups);
     *  - nlx_prove first does prover::set_lookup_wires ON THE DEVICE WITNESS IT IS HANDED (multiplicity wires of the
     *    LookupTableGate rows, padding slots of each table's last LookupGate row - the caller's buffer is written);
     *  - 2 * num_challenges more challenges are drawn after the gammas, the Zs commitment carries the
     *    num_challenges * (1 + S) lookup polynomials (RE, SLDC_0..S-1; S = ceil(num_routed_wires / 2 / (qdf - 1)))
     *    after the partial products, they are opened at zeta and g * zeta, and the vanishing polynomial carries
     *    check_lookup_constraints' 4 + num_luts + 2 S terms per challenge between the permutation and the gate terms.
     * All four arrays are host pointers, copied by nlx_circuit_build. */
    uint32_t num_luts;               /* 0 .. 16 */
    uint32_t pad_;
    const uint32_t* lut_sizes;       /* num_luts: entries per table (1 .. 65536) */
    const uint16_t* lut_pairs;       /* the tables' (input, output) pairs, table after table, 2 x u16 per entry */
    const uint32_t* lookup_rows;     /* 3 per table: last_lu_row, last_lut_row, first_lut_row (LookupWire); the LookupGate rows
                                        are [last_lu_row, last_lut_row), the LookupTableGate rows [last_lut_row, first_lut_row],
                                        row first_lut_row + 1 is a NoopGate row */
    const uint32_t* lut_num_lookups; /* num_luts: lookups made into each table (lut_to_lookups[t].len()) */
} nlx_circuit_desc;

typedef struct nlx_circuit nlx_circuit;

/* CircuitBuilder::build's prover data: commits the constants (selectors first, then gate
 * constants; (num_selectors + num_constants) x n) and the sigma polynomials (num_routed_wires x n),
 * both column-major subgroup evaluations, and keeps everything the prover needs resident in HBM. */
int32_t nlx_circuit_build(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants,
                          const uint64_t* sigmas, nlx_circuit** out);
/* The same with the config's Hasher chosen (NLX_HASHER_*): NLX_HASHER_POSEIDON_GOLDILOCKS is the entry above.
 * NLX_HASHER_POSEIDON_BN128 is plonky2x's PoseidonBN128GoldilocksConfig (the wrapper circuit's config; rules recalled, not pinned
 * against Rust output - tools/bn128_config_model.py): every Merkle tree of the proof hashes with
 * PoseidonBN128, a digest enters the transcript as five Goldilocks limbs (7, 7, 7, 7, 4 little-endian bytes), the challenger's
 * sponge, the public-inputs hash and the proof of work stay Goldilocks Poseidon, the circuit digest is a BN128 digest, and the
 * proof bytes keep their layout (a digest = four little-endian words).  Such a circuit goes through the prove, batch-prove,
 * digest, cap and stage entries like any other; its stage commitments are BN128 commitments.
 * Any other hasher: NLX_E_RANGE.  NLX_E_UNSUPPORTED under BN128 for circuits with lookup tables and for shapes with an oracle of
 * 4 columns or fewer (num_challenges * quotient_degree_factor <= 4: such a leaf is its own digest and has none when >= r). */
int32_t nlx_circuit_build_hasher(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants,
                                 const uint64_t* sigmas, uint32_t hasher, nlx_circuit** out);
/* the circuit's NLX_HASHER_* (NLX_E_INVAL for NULL) */
int32_t nlx_circuit_hasher(const nlx_circuit* c);
void nlx_circuit_destroy(nlx_circuit* c);
int32_t nlx_circuit_digest(const nlx_circuit* c, uint64_t out[4]);
int32_t nlx_circuit_constants_sigmas_cap(const nlx_circuit* c, uint64_t* cap_out);
size_t nlx_proof_max_bytes(const nlx_circuit* c);

/* prove_with_partition_witness + ProofWithPublicInputs::to_bytes.
 * wires: num_wires x n column-major (host or device).  proof_out: host buffer of proof_cap bytes.
 * Under NLX_HASHER_POSEIDON_GOLDILOCKS the witness is not checked against the circuit (with quotient_degree_factor = 2^rate_bits
 * plonky2's quotient degree check is vacuous): an unsatisfied witness yields a proof that a verifier rejects.  A circuit built
 * with NLX_HASHER_POSEIDON_BN128 fails with NLX_E_INVAL instead, here and in nlx_quotient_eval, when the top
 * quotient_degree_factor coefficients of a quotient polynomial are not zero: a check against wrong
 * witnesses, not a verifier. */
int32_t nlx_prove(nlx_circuit* c, const uint64_t* wires, const uint64_t* public_inputs, uint8_t* proof_out,
                  size_t proof_cap, size_t* proof_len);

/* ---- witness checker: which row, gate and constraint a witness breaks ----
 * Evaluates the circuit on the TRACE ROWS of a witness (no LDE, no random combination: a row is bad iff one of its own gate's
 * constraints is non-zero) and names the first thing that does not hold.  Call it when a proof does not verify. */
#define NLX_CHECK_GATES   1u   /* every row's gate constraints (Gate::eval_unfiltered_base of the row's own gate) */
#define NLX_CHECK_COPIES  2u   /* w[x] == w[sigma(x)] for every routed cell */
#define NLX_CHECK_LOOKUPS 4u   /* circuits with tables: real LookupGate slots and LookupTableGate entries */
#define NLX_CHECK_ALL     7u

typedef struct {
    uint32_t checked;      /* the NLX_CHECK_* bits that ran (LOOKUPS is dropped for a circuit without tables) */
    uint32_t satisfied;    /* 1: nothing found by any check that ran */
    /* gates: "first" = lowest row, then lowest constraint index (plonky2's order of the gate's constraints) */
    uint64_t gate_rows_bad;            /* rows with at least one non-zero constraint */
    uint32_t gate_row, gate_index /* into desc.gates */, gate_kind /* NLX_GATE_* */, gate_constraint;
    uint64_t gate_value;               /* that constraint's canonical value */
    /* copies: "first" = lowest row, then lowest column */
    uint64_t copy_cells_bad;           /* routed cells x with w[x] != w[sigma(x)] */
    uint32_t copy_row, copy_col, copy_to_row, copy_to_col;
    uint64_t copy_value, copy_to_value;
    /* lookups: "first" = lowest row, then lowest slot */
    uint64_t lookup_slots_bad;
    uint32_t lookup_row, lookup_slot, lookup_table, lookup_pad_;
    uint64_t lookup_input, lookup_output;
} nlx_witness_report;

/* wires: num_wires x n column-major, host or device, as nlx_prove takes them; never written (unlike nlx_prove on a circuit with
 * tables: the padding slots and multiplicity wires that nlx_prove fills are left alone and are not checked).  public_inputs feed
 * PublicInputGate through hash_no_pad, as in nlx_prove.  what: a non-empty set of NLX_CHECK_* bits.
 * Returns NLX_OK whenever the check ran - the verdict is in *report, which is zero-filled before anything else happens; when
 * report->satisfied == 0, nlx_last_error holds one line naming the row, the gate's plonky2 name, the constraint index and its
 * value, or the two cells of the copy, or the lookup slot.  NLX_E_INVAL: a NULL argument, `what` outside 1 .. 7, or a sigma
 * value that lies in no coset k_i H (its position is in the message).  Works the same under both hashers: nothing here hashes
 * except the host hash_no_pad of the public inputs.
 * The first check of a circuit builds what later checks reuse and the circuit keeps until nlx_circuit_destroy: for
 * NLX_CHECK_GATES the constants' values on H (one forward transform of the constants commitment's coefficients), for
 * NLX_CHECK_COPIES the sigma values decoded to (row, column).  A circuit that is never checked pays neither time nor memory for
 * them at nlx_circuit_build. */
int32_t nlx_circuit_check_witness(nlx_circuit* c, const uint64_t* wires, const uint64_t* public_inputs, uint32_t what,
                                  nlx_witness_report* report);

/* ---- stage-level entry points: the fine seam for callers that keep plonky2's own
 * prove_with_partition_witness loop and replace it stage by stage (SURVEY.md §8b call list) ---- */

/* The circuit's constants + sigmas commitment (FRI oracle 0), borrowed: owned by the circuit, do not destroy. */
const nlx_commit* nlx_circuit_constants_sigmas(const nlx_circuit* c);
/* a8 wires_permutation_partial_products_and_zs + PolynomialBatch::from_values: wires = num_wires x n subgroup
 * values (host or device); the commitment holds num_challenges Z columns followed by the partial products. */
int32_t nlx_partial_products_and_zs(nlx_circuit* c, const uint64_t* wires, const uint64_t betas[2], const uint64_t gammas[2],
                                    nlx_commit** zs_out);
/* a9 compute_quotient_polys + PolynomialBatch::from_coeffs: the num_challenges * quotient_degree_factor quotient
 * chunks, committed.  public_inputs_hash = hash_no_pad(public inputs) (nlx_hash_no_pad). */
int32_t nlx_quotient_eval(nlx_circuit* c, const nlx_commit* wires, const nlx_commit* zs, const uint64_t betas[2],
                          const uint64_t gammas[2], const uint64_t alphas[2], const uint64_t public_inputs_hash[4],
                          nlx_commit** quotient_out);

/* plonky2::iop::challenger::Challenger state: sponge_state, input_buffer, output_buffer (popped from the end). */
typedef struct {
    uint64_t state[12];
    uint64_t input[8];
    uint32_t n_input;
    uint32_t pad0;
    uint64_t output[8];
    uint32_t n_output;
    uint32_t pad1;
} nlx_challenger;
void nlx_challenger_init(nlx_challenger* c);
int32_t nlx_challenger_observe(nlx_challenger* c, const uint64_t* elements, size_t n);
int32_t nlx_challenger_challenge(nlx_challenger* c, uint64_t* out, size_t n);
/* Challenger::observe_hash / observe_cap (host only): n_digests digests of four words each.  NLX_HASHER_POSEIDON_GOLDILOCKS: the
 * four words are the elements.  NLX_HASHER_POSEIDON_BN128: each digest enters as five Goldilocks elements, its 32 little-endian
 * bytes cut into chunks of 7, 7, 7, 7 and 4; a digest >= r: NLX_E_RANGE, nothing observed.  Other hashers: NLX_E_RANGE. */
int32_t nlx_challenger_observe_hash(nlx_challenger* c, const uint64_t* digests, size_t n_digests, uint32_t hasher);
/* PoseidonHash::hash_no_pad on the host (public-inputs hash, circuit digest) */
int32_t nlx_hash_no_pad(const uint64_t* elements, size_t n, uint64_t out[4]);

typedef struct {
    uint32_t arity_bits;       /* FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) */
    uint32_t final_poly_bits;
    uint32_t pow_bits;         /* proof_of_work_bits */
    uint32_t num_queries;      /* num_query_rounds */
} nlx_fri_params;
/* a11 PolynomialBatch::prove_openings / fri_proof for an instance of the shape every caller on this path has:
 * batch 0 = every column of every oracle (in order) opened at zeta, batch 1 = the first n_next[o] columns of
 * every oracle o (in order) opened at g * zeta (plonky2: oracles = constants_sigmas, wires, zs_partial_products,
 * quotient and n_next = {0, 0, num_challenges, 0}; a STARK: n_next = all columns of every trace oracle).  openings_* are the extension values (2 words each)
 * already observed by the caller's challenger; the challenger is advanced exactly as upstream's
 * (fri alpha, commit-phase caps and betas, final polynomial, proof of work, query indices).  Writes the FriProof
 * bytes: commit_phase_merkle_caps, query_round_proofs, final_poly, pow_witness. */
int32_t nlx_fri_prove(nlx_ctx* ctx, const nlx_commit* const* oracles, uint32_t n_oracles, const uint32_t* n_next,
                      const uint64_t zeta[2], const uint64_t* openings_zeta, const uint64_t* openings_next,
                      const nlx_fri_params* params, nlx_challenger* challenger, uint8_t* proof_out, size_t proof_cap,
                      size_t* proof_len);

/* The same with the hasher of the commit-phase Merkle trees and of cap observation chosen; every oracle must carry that hasher
 * (NLX_E_UNSUPPORTED otherwise; an unknown hasher: NLX_E_RANGE).  Hasher 0 is the entry above.  Kernel-timing names of the BN128
 * commit phase: "fri_leaves_bn128" and "fri_merkle_levels_bn128", units BN128 permutations. */
int32_t nlx_fri_prove_hasher(nlx_ctx* ctx, const nlx_commit* const* oracles, uint32_t n_oracles, const uint32_t* n_next,
                             const uint64_t zeta[2], const uint64_t* openings_zeta, const uint64_t* openings_next,
                             const nlx_fri_params* params, uint32_t hasher, nlx_challenger* challenger, uint8_t* proof_out,
                             size_t proof_cap, size_t* proof_len);

/* a13: plonky2x LocalProver::batch_prove.  Proves n_jobs independent jobs with n_workers concurrent
 * workers.  workers[i] are circuits built from the SAME description on DISTINCT contexts (one stream +
 * one host thread each; contexts may be on the same GPU - overlapping one proof's latency-bound phases
 * with another's throughput-bound kernels - or on different GPUs).  Jobs are taken in order by whichever
 * worker is free; each job's outcome is written to its own status / proof_len.  Returns NLX_OK if every
 * job succeeded, else the first failing job's code. */
typedef struct {
    const uint64_t* wires;          /* num_wires x n column-major, host or device (device of the worker that runs it) */
    const uint64_t* public_inputs;
    uint8_t* proof_out;             /* host buffer */
    size_t proof_cap;
    size_t proof_len;               /* out */
    int32_t status;                 /* out */
} nlx_prove_job;
int32_t nlx_batch_prove(nlx_circuit* const* workers, uint32_t n_workers, nlx_prove_job* jobs, size_t n_jobs);

/* Per-stage device time of the most recent nlx_prove on this circuit, in milliseconds
 * (HIP events on the context's stream).  names_out receives static strings. */
#define NLX_MAX_STAGES 24
int32_t nlx_prove_stage_times(const nlx_circuit* c, uint32_t* n_stages, const char** names_out, float* ms_out);

/* a11 fri_proof_of_work: smallest nonce w such that the Poseidon duplex of `state` with w written
 * at `pos` has at least `bits` leading zero bits in output word 7. */
int32_t nlx_pow_grind(nlx_ctx* ctx, const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t* nonce_out);

/* ---- a12: starky-style STARK prover ----
 * Replaces starky::prover::prove / compute_quotient_polys / StarkOpeningSet::new / Stark::fri_instance -
 * the public ancestor of the un-vendored starkyx (curta) prover that plonky2x runs for nearx's
 * curta_eddsa_verify / curta_sha256 calls (nearx/src/builder.rs; Cargo.lock:6515).  The AIR is data: a
 * register program replacing Stark::eval_packed_generic + ConstraintConsumer, interpreted per point of
 * the quotient coset.  Words are op | dst << 8 | a << 24 | b << 40 (16-bit fields); NLX_AIR_CONST is
 * followed by one immediate word.  Registers r0 .. r63; a register must be written before it is read.
 * Each EMIT feeds every challenge's accumulator: acc_j = acc_j * alpha_j + c. */
#define NLX_AIR_LOCAL 0            /* r[dst] = local_values[a] */
#define NLX_AIR_NEXT 1             /* r[dst] = next_values[a] */
#define NLX_AIR_PUBLIC 2           /* r[dst] = public_inputs[a] */
#define NLX_AIR_CONST 3            /* r[dst] = immediate (next word) */
#define NLX_AIR_ADD 4              /* r[dst] = r[a] + r[b] * 2^sh, sh = word bits 56..61 (0 = plain add) */
#define NLX_AIR_SUB 5              /* r[dst] = r[a] - r[b] * 2^sh */
#define NLX_AIR_MUL 6
#define NLX_AIR_EMIT_TRANSITION 7  /* ConstraintConsumer::constraint_transition(r[a]): times (x - g^-1) */
#define NLX_AIR_EMIT_FIRST 8       /* constraint_first_row(r[a]): times L_0(x) */
#define NLX_AIR_EMIT_LAST 9        /* constraint_last_row(r[a]): times L_{n-1}(x) */
#define NLX_AIR_EMIT 10            /* constraint(r[a]) on every row */
#define NLX_AIR_PERIODIC 11        /* r[dst] = periodic column a at this row (values[a][row mod period]) */
#define NLX_AIR_PACK_LOCAL 12      /* r[dst] = sum_{i<b} 2^i local_values[a+i], 1 <= b <= 32 (bits -> word) */
#define NLX_AIR_PACK_NEXT 13       /* r[dst] = sum_{i<b} 2^i next_values[a+i] */
#define NLX_AIR_EMIT_BOOL 14       /* constraint(x * (x - 1)) for x = local_values[a .. a + max(b, 1)), in column order */
#define NLX_AIR_LOADV 15           /* scheduling hint: the next `dst` (<= 8) words are independent LOCAL / NEXT / PUBLIC /
                                      PERIODIC loads with distinct destinations; the kernel issues them together */
/* three-operand forms for bit-valued columns (bitwise hash AIRs); the third register index is in bits 56..61 */
#define NLX_AIR_XOR3 16            /* r[dst] = a ^ b ^ c as a polynomial: s = a + b - 2ab, s + c - 2sc */
#define NLX_AIR_CH 17              /* r[dst] = c + a (b - c) */
#define NLX_AIR_MAJ 18             /* r[dst] = ab + c (a + b - 2ab) */
/* A segment boundary: no register value is carried across this word (the builder rejects a read of a register not
 * written since the last boundary).  A sequential interpreter may ignore it; the GPU evaluates the segments of a
 * long program as independent work items - (quotient points) x (segments) waves instead of (quotient points) -
 * and adds the segments' partial sums with the alpha powers their position in the program implies, so a wide AIR
 * on a short trace still fills the chip.  At most NLX_AIR_MAX_SEGMENTS - 1 boundaries per program. */
#define NLX_AIR_SEGMENT 19
/* The two base-field constraints of one LogUp helper (near-light-client_amd/logup.py) as one instruction:
 *   h (alpha + v1)(alpha + v2) = (alpha + v1) + (alpha + v2)   in F_p[X]/(X^2 - 7),
 * v1 = local[a], v2 = local[dst] (dst = 0xFFFF: a single lookup, h (alpha + v1) = 1), h = local[b] + local[b+1] X,
 * alpha = challenge k + challenge k+1 X with k in word bits 56..61.  Emits the X^0 then the X^1 coefficient. */
#define NLX_AIR_EMIT_LOGUP 20
#define NLX_AIR_MAC 21             /* r[dst] = r[c] + r[a] * r[b], c in word bits 56..61: the inner step of every limb convolution */
#define NLX_AIR_MAX_SEGMENTS 256
#define NLX_AIR_NUM_REGS 64
#define NLX_AIR_MAX_PERIODIC 128

typedef struct {
    uint32_t degree_bits;
    uint32_t n_cols;                  /* Stark::COLUMNS */
    uint32_t num_challenges;          /* StarkConfig::standard_fast_config: 2 */
    uint32_t rate_bits;               /* 1 */
    uint32_t cap_height;              /* 4 */
    uint32_t quotient_degree_factor;  /* Stark::quotient_degree_factor() rounded up to a power of two, <= 2^rate_bits */
    uint32_t fri_pow_bits;            /* 16 */
    uint32_t fri_num_queries;         /* 84 */
    uint32_t fri_arity_bits;          /* 4 */
    uint32_t fri_final_poly_bits;     /* 5 */
    uint32_t num_public_inputs;       /* Stark::PUBLIC_INPUTS */
    uint32_t n_words;
    const uint64_t* program;          /* host */
    /* Periodic columns (round constants, round selectors): known to the verifier, not committed.  Column a
     * has the value periodic[a * period + (row mod period)], period = 2^period_bits <= n; as a polynomial it
     * is P_a(x^(n/period)) with P_a the interpolation over the period-th roots of unity (degree < n, counts
     * as degree 1 in the constraint degree). */
    uint32_t n_periodic;              /* <= NLX_AIR_MAX_PERIODIC */
    uint32_t period_bits;
    const uint64_t* periodic;         /* host, n_periodic x period */
    /* Rounds of commitment (starkyx's TraceWriter rounds: lookup / bus accumulators are functions of challenges
     * drawn after the main trace is committed).  0 = classic single-round starky.  Round r commits round_cols[r]
     * columns (sum = n_cols; program column indices run through the rounds in order); once its Merkle cap is in the
     * transcript the verifier draws round_challenges[r] base-field challenges, which the program reads as
     * NLX_AIR_PUBLIC indices num_public_inputs + k in the order drawn.  The alphas follow the last round. */
    uint32_t n_rounds;                /* 0..3 */
    uint32_t round_cols[3];
    uint32_t round_challenges[3];
    /* Grouped Merkle leaves.  0 = every leaf is plonky2's hash_or_noop of the whole LDE row (starky's MerkleTree).  G > 0:
     * a row of more than G columns is hashed as hash_no_pad(hash_no_pad(cols [0, G)) || hash_no_pad(cols [G, 2G)) || ...) -
     * the tree's bottom level has arity ceil(n_cols / G) over column runs.  The proof's layout does not change (opened rows
     * and sibling paths), the verifier spends ceil(K / 2) more permutations per opened row; for the prover the K runs of a
     * leaf are independent work, which a trace of thousands of columns on a few thousand rows needs to fill the GPU
     * (host rule: stark.py StarkConfig.leaf_group_cols).  Applies to every commitment of the proof
     * (narrower ones are unaffected) and is part of the statement digest when non-zero.  8 <= G <= 4096. */
    uint32_t leaf_group_cols;
    /* Round values: round_values[r] (<= 64) field elements the prover sends with round r - totals of bus / accumulator
     * columns that depend on earlier challenges.  They enter the transcript after the round's cap and before its
     * challenges are drawn, travel after the public inputs at the end of the proof, and the program reads them as
     * NLX_AIR_PUBLIC: the values array is  public inputs | values of round 0 | challenges of round 0 | values of round 1 |
     * challenges of round 1 | ...  The proof only shows that the constraints hold for the values it carries; whoever
     * relies on the proof compares them with what they should be (e.g. the fingerprint of the claimed data). */
    uint32_t round_values[3];
    /* Openings digest.  0 = the transcript observes every opened value (starky's observe_openings: local ++ quotient at zeta,
     * then the next values).  G > 0: it observes FOUR elements instead - that vector, zero-padded to a multiple of G, hashed
     * in runs of G (hash_no_pad each) and the run digests hashed once more.  The binding is the same; the sequential absorption
     * of 19 000 values on one host thread (2 400 permutations: 3 of the 8 ms of the Sync step's SHA-512 proof) becomes one
     * small device launch and 150 host permutations.  Part of the statement digest when non-zero.
     * 8 <= G <= 4096; a patch that must stay compatible with an unpatched starky verifier passes 0. */
    uint32_t openings_group;
    /* Batches.  0 = a round's columns are ONE PolynomialBatch (one Merkle tree, one cap).  B > 0: a round of more than B columns
     * is committed as ceil(cols / B) PolynomialBatches of B columns (the last one what is left), in column order - each exactly
     * plonky2's PolynomialBatch::from_values: leaf = hash_or_noop(that batch's row), its own 2^cap_height-entry cap, its own FRI
     * oracle.  Nothing new for a verifier: the transcript observes the caps in order, the proof carries them in order, every
     * query opens each batch's row with its own Merkle path, the openings and their order do not change.  Why: a leaf of a
     * 4 745-column row is 594 permutations in SEQUENCE (a sponge), and a trace of 2^10 LDE rows has 1 024 of them - the GPU
     * idles while every lane walks its chain; ten batches are ten independent sponges per row.  The cost is on the verifier's
     * side: ceil(cols / B) - 1 more Merkle paths per query and round.  Part of the statement digest when non-zero.
     * 8 <= B <= 65535; at most NLX_STARK_MAX_ORACLES batches + 1 (the quotient) in all. */
    uint32_t batch_cols;
} nlx_stark_desc;
#define NLX_STARK_MAX_ORACLES 31
typedef struct nlx_stark nlx_stark;

/* Validates the program and keeps it and the coset tables resident on the device. */
int32_t nlx_stark_build(nlx_ctx* ctx, const nlx_stark_desc* desc, nlx_stark** out);
void nlx_stark_destroy(nlx_stark* s);
size_t nlx_stark_proof_max_bytes(const nlx_stark* s);
/* Which kernel evaluates this STARK's constraints on the quotient coset (starky::prover::compute_quotient_polys ->
 * Stark::eval_packed_generic; for the reference's circuits the curta AIRs behind /root/reference/nearx/src/builder.rs:152,220,316):
 * 1 = a straight-line kernel generated at library build time from exactly this program (near-light-client_amd/airgen.py: the
 * fixed AIRs of a Sync step and of the Verify job's map STARKs), 0 = the register-program interpreter (any program).  Same
 * results either way; the environment variable NLX_AIR_VM=1, read when the STARK is built, keeps the interpreter. */
int32_t nlx_stark_quotient_kernel(const nlx_stark* s);
/* starky::prover::prove + StarkProofWithPublicInputs serialisation (wire format in DESIGN.md):
 * trace: n_cols x n column-major (host or device), every value canonical. */
int32_t nlx_stark_prove(nlx_stark* s, const uint64_t* trace, const uint64_t* public_inputs, uint8_t* proof_out,
                        size_t proof_cap, size_t* proof_len);
/* Multi-round proving: round_fn(user, r, known, n_known, values_out) returns round r's columns (round_cols[r] x n,
 * column-major, host or device pointer, valid until the next callback or the end of the call) given `known` - the
 * round values and challenges of the earlier rounds, in values-array order - and writes the round's round_values[r]
 * values to values_out (NULL when the round sends none).  Proof bytes: one cap per round, the quotient cap, local / next values of every column in round
 * order, quotient values, FriProof (one oracle per round + the quotient oracle), public inputs, round values. */
typedef const uint64_t* (*nlx_round_fn)(void* user, uint32_t round, const uint64_t* known, uint32_t n_known, uint64_t* values_out);
int32_t nlx_stark_prove_rounds(nlx_stark* s, nlx_round_fn round_fn, void* user, const uint64_t* public_inputs,
                               uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
int32_t nlx_stark_stage_times(const nlx_stark* s, uint32_t* n_stages, const char** names_out, float* ms_out);
/* As nlx_batch_prove, for STARK jobs: workers = provers built from the SAME description on DISTINCT contexts;
 * a job's `wires` field is its trace (n_cols x n, host or device). */
int32_t nlx_stark_batch_prove(nlx_stark* const* workers, uint32_t n_workers, nlx_prove_job* jobs, size_t n_jobs);

/* ---- trace checker: which row and which constraint a trace breaks ----
 * nlx_stark_prove and nlx_stark_prove_rounds never ask whether the trace satisfies the AIR: a wrong trace becomes proof bytes
 * that a verifier rejects.  The checker runs the STARK's register program on the n TRACE ROWS (local = row i, next = row
 * (i + 1) mod n, NLX_AIR_PERIODIC = periodic[a * period + (i mod period)]; no LDE, no hashing, no random combination) with the
 * quotient's filters as row predicates: EMIT_FIRST counts on row 0 only, EMIT_LAST on row n - 1 only, EMIT_TRANSITION on rows
 * 0 .. n - 2, EMIT / EMIT_BOOL / EMIT_LOGUP on every row, the wrap at n - 1 included; a constraint outside its rows counts as
 * zero.  That is the condition under which a verifier accepts an honest proof: the filtered constraints vanish on H.
 * A constraint's index is its position in emission order over the whole program (segment boundaries do not count; EMIT_BOOL
 * counts one per column, EMIT_LOGUP two: X^0, then X^1); nlx_stark_num_constraints is how many there are. */
typedef struct {
    uint32_t satisfied;        /* 1: every constraint is zero on every row it applies to */
    uint32_t n_constraints;    /* what the program emits */
    uint64_t rows_bad;         /* rows with at least one non-zero constraint */
    uint64_t pairs_bad;        /* non-zero (row, constraint) pairs */
    /* first = lowest row, then lowest constraint index */
    uint32_t row, constraint, kind /* NLX_AIR_EMIT* opcode */, word /* index of the emitting program word */;
    uint32_t sub;              /* EMIT_BOOL: column offset; EMIT_LOGUP: 0 / 1; else 0 */
    uint32_t pad_;
    uint64_t value;            /* canonical */
} nlx_trace_report;

uint32_t nlx_stark_num_constraints(const nlx_stark* s);
/* trace and public_inputs as nlx_stark_prove takes them (n_cols x n column-major, host or device, canonical words); the trace is
 * never written.  per_constraint: NULL, or a host array of n_constraints words that receives, per constraint, the number of
 * rows on which it is not zero.
 * Both entries return NLX_OK whenever the check ran - the verdict is in *report, which is zero-filled before anything else
 * happens; when report->satisfied == 0, nlx_last_error holds one line naming the row, the constraint index, its kind, the word
 * index and the value.  NLX_E_INVAL: a NULL s, trace, round_fn or report; public_inputs NULL while the STARK has public inputs;
 * nlx_stark_check_trace on a STARK with more than one round or with round challenges; a round callback that returns NULL (the
 * message of nlx_stark_prove_rounds).  NLX_E_RANGE: a public input, or a caller's challenge, that is not canonical.  The checker
 * always runs the register program, whichever kernel nlx_stark_quotient_kernel names.  The first check of a STARK uploads the periodic table as it stands and each segment's first constraint index; the
 * STARK keeps both until nlx_stark_destroy, and one that is never checked pays nothing for them at nlx_stark_build. */
int32_t nlx_stark_check_trace(nlx_stark* s, const uint64_t* trace, const uint64_t* public_inputs,
                              nlx_trace_report* report, uint64_t* per_constraint /* host, n_constraints words, or NULL */);
/* The multi-round form.  round_fn is called exactly as nlx_stark_prove_rounds calls it - the same `known` array, the round's
 * values taken from values_out - but nothing is committed.  challenges == NULL: each round's challenges are drawn from a host
 * transcript that has observed the AIR digest, the public inputs and every earlier round's values (deterministic; there is no
 * cap to observe, so they are NOT the challenges of the proof).  Otherwise the caller's values are used, in the order a prover
 * would draw them (NLX_E_RANGE if one is not canonical).  A correct trace writer satisfies the constraints for any challenges,
 * with one proviso: a LogUp helper h = 1 / (alpha + v) has no value where alpha + v = 0 in the quadratic extension, which for a
 * challenge drawn from a transcript happens with probability about n_lookups / 2^128 - negligible, but a caller who passes
 * challenges of their own choosing can make it happen. */
int32_t nlx_stark_check_rounds(nlx_stark* s, nlx_round_fn round_fn, void* user, const uint64_t* public_inputs,
                               const uint64_t* challenges /* NULL, or sum(round_challenges) canonical values */,
                               nlx_trace_report* report, uint64_t* per_constraint);

/* ---- STARK verifier: does a proof verify, and if not, which check breaks ----
 * starky::verifier::verify_stark_proof for the proofs nlx_stark_prove / nlx_stark_prove_rounds write (wire format: DESIGN.md
 * section 8), one proof or a batch of proofs of the same STARK.  The host parses the proof against the layout the descriptor
 * implies, replays the transcript, checks the proof of work and draws the query indices; the device hashes every Merkle path
 * (one quad of lanes per proof x query x tree), does the FRI arithmetic (one wave per proof x query) and evaluates the register
 * program at zeta over the quadratic extension (one lane per proof, one block per program segment).
 * The verdict names the FIRST failing check in this order: malformed structure; the caller's public inputs; the constraints
 * at zeta; the proof of work; then the lowest failing query and within it the trace paths in tree order (trace batches, then
 * the quotient), per FRI layer the fold before the path, and the final polynomial.  Fields that do not apply are 0. */
#define NLX_VERIFY_ACCEPT        0
#define NLX_VERIFY_MALFORMED     1  /* length, public-input count, a path-length byte, trailing bytes, a field word >= p */
#define NLX_VERIFY_PUBLIC_INPUTS 2  /* the caller's expected public inputs differ from the proof's */
#define NLX_VERIFY_CONSTRAINTS   3  /* sum alpha^i c_i(zeta) != Z_H(zeta) * sum zeta^(n k) q_k(zeta) for `challenge` */
#define NLX_VERIFY_POW           4
#define NLX_VERIFY_TRACE_PATH    5  /* an opened row of commitment `tree` does not hash up to its cap, query `query` */
#define NLX_VERIFY_FRI_FOLD      6  /* layer `layer`: evals[x mod arity] != the value folded so far */
#define NLX_VERIFY_FRI_PATH      7  /* layer `layer`'s coset does not hash up to that layer's cap */
#define NLX_VERIFY_FINAL_POLY    8
typedef struct {
    uint32_t accepted;   /* 1: the proof verifies */
    uint32_t reason;     /* NLX_VERIFY_* */
    uint32_t challenge;  /* CONSTRAINTS: which alpha's identity fails */
    uint32_t query;      /* from TRACE_PATH on (and a MALFORMED path-length byte): the query */
    uint32_t tree;       /* TRACE_PATH (and a MALFORMED path-length byte of a commitment): the commitment, in proof order */
    uint32_t layer;      /* FRI_FOLD, FRI_PATH (and a MALFORMED path-length byte of a FRI layer): the layer */
    uint64_t x_index;    /* from TRACE_PATH on: the query's index into the LDE, as drawn from the transcript */
} nlx_stark_verdict;
/* Both entries return NLX_OK whenever the check ran - the verdict is in *verdict (verdicts[i] for proof i), zero-filled before
 * anything else happens; on a rejection (of the first rejected proof of a batch) nlx_last_error holds one line naming reason,
 * query, tree and layer.  public_inputs: NULL - the statement is the one the proof carries - or num_public_inputs canonical
 * words (per proof, back to back, for a batch) that the proof's must equal.  NLX_E_INVAL: a NULL s, proof, lens or verdict;
 * NLX_E_RANGE: a caller's public input that is not canonical.  No device address and no loop bound depends on a byte of the
 * proof.  The first verify of a STARK uploads the periodic columns' interpolation coefficients, which the STARK keeps until
 * nlx_stark_destroy (each segment's constraint count and the table of the proof's trees travel with every launch); a STARK that
 * is never verified pays nothing for them at nlx_stark_build.  The register program always runs on the interpreter. */
int32_t nlx_stark_verify(nlx_stark* s, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                         nlx_stark_verdict* verdict);
int32_t nlx_stark_verify_batch(nlx_stark* s, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                               const uint64_t* public_inputs, nlx_stark_verdict* verdicts);
/* the exact length of a proof of this STARK (0 for NULL) */
size_t nlx_stark_proof_bytes(const nlx_stark* s);

/* ---- plonky2 verifier: does a ProofWithPublicInputs verify, and if not, which check breaks ----
 * plonky2::plonk::verifier::verify for the proofs nlx_prove / nlx_batch_prove write, over the whole gate set the prover supports
 * (the gate kinds 1 .. 18 and the lookup argument), one proof or a batch of proofs of the same circuit.  An nlx_verifier is
 * plonky2's VerifierCircuitData: the common data (a copy of the descriptor with its gates, k_is and lookup tables) and the
 * verifier-only data (constants_sigmas_cap, circuit_digest) - it needs none of the prover's resident tables.
 * The host parses the proof against the layout the descriptor implies, hashes the public inputs, replays the transcript, checks
 * the proof of work, draws the query indices and reduces the openings; the device hashes every Merkle path (one quad of lanes
 * per proof x query x tree), does the FRI arithmetic (one wave per proof x query) and evaluates every gate's constraints, the
 * permutation argument and the lookup argument at zeta over the quadratic extension (one lane per proof, one block row per gate).
 * The verdict has nlx_stark_verdict's fields and the NLX_VERIFY_* reasons, and names the FIRST failing check in a sequential
 * verifier's order: malformed structure; the caller's public inputs; the vanishing identity (lowest failing challenge); the
 * proof of work; then the lowest failing query and within it the four initial paths in tree order (`tree` 0 .. 3:
 * constants_sigmas, wires, zs_partial, quotient), per FRI layer the fold before the path, and the final polynomial.
 * One deliberate difference from the test oracle's verifier (oracle/plonk.c), which does not look at it: a field word of the
 * proof that is not below p is NLX_VERIFY_MALFORMED here, as for STARK proofs.
 * nlx_verifier_from_circuit and nlx_verifier_create are the Goldilocks Poseidon config's: a NLX_HASHER_POSEIDON_BN128 circuit
 * gives NLX_E_UNSUPPORTED there.  The *_hasher entries below take either config. */
typedef nlx_stark_verdict nlx_proof_verdict;
typedef struct nlx_verifier nlx_verifier;
/* the cap and the digest of a built circuit; the verifier lives on the circuit's context and does not need the circuit later */
int32_t nlx_verifier_from_circuit(const nlx_circuit* c, nlx_verifier** out);
/* for a party that holds only the verifying key: the descriptor (checked as nlx_circuit_build checks it; its arrays are
 * copied), the cap (4 << cap_height words) and the digest.  A non-zero desc->circuit_digest must equal `digest`
 * (NLX_E_INVAL otherwise). */
int32_t nlx_verifier_create(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap,
                            const uint64_t digest[4], nlx_verifier** out);
/* The same with the config's Hasher named (NLX_HASHER_*).  NLX_HASHER_POSEIDON_GOLDILOCKS is exactly the
 * two entries above.  NLX_HASHER_POSEIDON_BN128 verifies the proofs of a nlx_circuit_build_hasher circuit under plonky2x's
 * PoseidonBN128GoldilocksConfig (rules recalled, not pinned against plonky2x's own verifier): every Merkle path over BN254 Fr, the
 * circuit digest and the caps entering the transcript as five limbs a digest, everything else as above.  A digest of the proof -
 * the caps, the FRI caps, every sibling - is four little-endian words of ONE integer that must be below r (its words need not be
 * below p); a digest that is not is NLX_VERIFY_MALFORMED, as a field word that is not below p.
 * create_hasher: the descriptor is checked as nlx_circuit_build_hasher checks it (NLX_E_UNSUPPORTED under BN128 for lookup tables
 * and for an oracle of <= 4 columns), cap and digest as digests of that hasher (NLX_E_RANGE).
 * from_circuit_hasher: the config the caller expects; NLX_E_INVAL when the circuit was built under the other one, NLX_E_RANGE
 * for an unknown hasher. */
int32_t nlx_verifier_create_hasher(nlx_ctx* ctx, const nlx_circuit_desc* desc, const uint64_t* constants_sigmas_cap,
                                   const uint64_t digest[4], uint32_t hasher, nlx_verifier** out);
int32_t nlx_verifier_from_circuit_hasher(const nlx_circuit* c, uint32_t hasher, nlx_verifier** out);
/* the verifier's NLX_HASHER_* (NLX_E_INVAL for NULL) */
int32_t nlx_verifier_hasher(const nlx_verifier* v);
void nlx_verifier_destroy(nlx_verifier* v);
/* the exact length of a proof of this circuit (0 for NULL) */
size_t nlx_verifier_proof_bytes(const nlx_verifier* v);
/* The conventions of nlx_stark_verify: NLX_OK whenever the check ran - the verdict is in *verdict (verdicts[i] for proof i),
 * zero-filled before anything else happens; on a rejection (of the first rejected proof of a batch) nlx_last_error holds one
 * line naming reason, query, tree and layer.  public_inputs: NULL, or num_public_inputs canonical words (per proof, back to
 * back, for a batch) that the proof's must equal (NLX_VERIFY_PUBLIC_INPUTS); NLX_E_RANGE if one is not canonical.
 * NLX_E_INVAL: a NULL v, proof, lens or verdict.  No device address and no loop bound depends on a byte of the proof. */
int32_t nlx_verify(nlx_verifier* v, const uint8_t* proof, size_t len, const uint64_t* public_inputs, nlx_proof_verdict* verdict);
int32_t nlx_verify_batch(nlx_verifier* v, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                         const uint64_t* public_inputs, nlx_proof_verdict* verdicts);
/* a12: range-check lookups for multi-round AIRs - the log-derivative argument with the challenge in the quadratic
 * extension (starkyx's lookup / bus accumulators are the reason it commits in rounds; its own constraints are not in
 * the reference tree, Cargo.lock:6515).  Constraint side: near-light-client_amd/logup.py.  Witness side, on the device:
 *   nlx_logup_multiplicities: trace is the round-0 buffer (n_cols x 2^log_n, column-major, host or device); the cells of
 *     the n_lookups columns `cols` must lie in [0, 2^table_bits) (else NLX_E_RANGE: the witness is wrong); column
 *     mult_col is overwritten with the multiplicities (the count of value v in row v).
 *   nlx_logup_round: for alpha = alpha[0] + alpha[1] X writes the nlx_logup_round_cols(n_lookups) round-1 columns into
 *     out: helpers h_j = 1/(alpha+v_2j) + 1/(alpha+v_2j+1) (two base columns each), g = m/(alpha+t) with t(i) = i mod
 *     2^table_bits, and the running sum phi(0) = 0, phi(i+1) = phi(i) + sum_j h_j(i) - g(i).
 * table_cols (a power of two, normally 1): the table may be spread over that many periodic columns of period
 * P = 2^table_bits / table_cols, column c holding c P + (i mod P), so that a trace shorter than the table can carry it;
 * mult_col is then the first of table_cols consecutive multiplicity columns (value v counts in column v / P, row v mod P)
 * and the round has one g per table column: helpers | g_0 .. g_(table_cols-1) | phi.
 * Both may be called from inside an nlx_round_fn callback on the same context. */
int32_t nlx_logup_multiplicities(nlx_ctx* ctx, uint64_t* trace, uint32_t n_cols, uint32_t log_n, const uint32_t* cols,
                                 uint32_t n_lookups, uint32_t table_bits, uint32_t table_cols, uint32_t mult_col);
uint32_t nlx_logup_round_cols(uint32_t n_lookups, uint32_t table_cols);
int32_t nlx_logup_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t n_cols, uint32_t log_n, const uint32_t* cols,
                        uint32_t n_lookups, uint32_t table_bits, uint32_t table_cols, uint32_t mult_col, const uint64_t alpha[2],
                        uint64_t* out);
/* a12: the multiplication unit mod 2^255 - 19 (the field under the Ed25519 verifications of
 * curta_eddsa_verify_sigs_conditional, nearx/src/builder.rs:152) as a stand-alone chip: one a * b = c (mod p) per row.
 * Constraints: near-light-client_amd/fp25519.py::FpMulChip.  a, b: 2^log_rows operands of four little-endian 64-bit
 * words each (any value < 2^256).  Writes the NLX_FP25519_CHIP_COLS x 2^log_rows round-0 trace (16-bit limbs of a, b,
 * the canonical c, the quotient, the carries' low and high parts; the two multiplicity columns - of the 2^16 table and of
 * the 2^9 table of the carries' high parts - zeroed: fill them with nlx_logup_multiplicities). */
#define NLX_FP25519_CHIP_COLS 97
int32_t nlx_fp25519_chip_trace(nlx_ctx* ctx, const uint64_t* a, const uint64_t* b, uint32_t log_rows, uint64_t* trace_out);
/* a12 / f.1: trace generation on the GPU for the Ed25519 verification AIR (constraints and column layout:
 * near-light-client_amd/ed25519_air.py; caller in the reference: curta_eddsa_verify_sigs_conditional,
 * nearx/src/builder.rs:152).  slots: 2^log_slots signatures of NLX_ED25519_SLOT_WORDS = 32 little-endian 64-bit words
 * each: five 256-bit numbers A.x, A.y, R.x, R.y (affine, reduced), S; the 512-bit D = SHA-512(R || A || M) read as a
 * little-endian integer (8 words; the AIR reduces it mod L itself); word 28 = the slot's `active` flag (0: a validator
 * that did not sign - the rows are generated with the three checks off); three spare words.  Writes the NLX_ED25519_COLS0 x
 * (256 << log_slots) round-0 trace (host or device), the two multiplicity columns (2^9 table of the carries' high parts,
 * then the 2^16 table - last, so that a proof of fewer than 2^8 slots can append the further multiplicity columns of a
 * table spread over several columns) zeroed (nlx_logup_multiplicities fills them).  Returns NLX_E_INVAL naming the first
 * slot whose statement is false (an active slot whose signature does not verify or whose A / R is off the curve; any slot
 * with S >= L or a coordinate >= p): no trace satisfies the AIR for it. */
#define NLX_ED25519_SLOT_WORDS 32
#define NLX_ED25519_COLS0 1488
int32_t nlx_ed25519_trace(nlx_ctx* ctx, const uint64_t* slots, uint32_t log_slots, uint64_t* trace_out);
/* The AIR's binding accumulator (round 1, two base columns = one column over F_p^2) for the challenge gamma = gamma[0] +
 * gamma[1] X: the running Horner fingerprint of every slot's 96 limbs (limb 15 first; the 32-byte encodings of A and R - y with the
 * parity of x in bit 255 -, S, D mod 2^256, D div 2^256, active), each row
 * holding what was absorbed before it.  trace: the round-0 trace (host or device); acc_out: 2 x (256 << log_slots);
 * total_out: the fingerprint of all slots - the round value the proof sends, which the relying party recomputes from
 * the tuples it believes were verified (near-light-client_amd/ed25519_air.py::fingerprint). */
int32_t nlx_ed25519_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_slots, const uint64_t gamma[2],
                               uint64_t* acc_out, uint64_t total_out[2]);
/* Self-test entry for the arithmetic mod 2^255 - 19 of the trace generator's scan (csrc/fe25519_fast.hpp and the four-lane
 * moves of k_ed_scan4), one lane per element.  a, b: n x 10 signed limbs of 26 bits (value = sum l_i 2^(26 i)), |l_i| < 2^28, NOT
 * reduced first.  out: n x NLX_FE25519_OPS_WORDS u32 (host or device), per element: words 0-15 the canonical value of a as
 * 16-bit limbs; 16-31 the canonical product a b; 32-41 the product's ten carried limbs as the device holds them (two's
 * complement); 42-57 the canonical product of the NEXT lane of the element's quad (element 4 (i / 4) + (i + 1) % 4), fetched
 * through the quad broadcasts and the lane select of the scan; lanes past n compute element n - 1. */
#define NLX_FE25519_OPS_WORDS 58
int32_t nlx_fe25519_ops(nlx_ctx* ctx, const int32_t* a, const int32_t* b, size_t n, uint32_t* out);
/* f.1: trace generation on the GPU for the SHA-256 compression AIR (column layout and constraints:
 * near-light-client_amd/sha256_air.py; callers in the reference: curta_sha256 at nearx/src/merkle.rs:49,
 * nearx/src/variables.rs:71-72).  blocks: 2^log_blocks padded 512-bit blocks as 16 big-endian-decoded words
 * each; is_first[b] != 0 where block b starts a new message (block 0 always does).  Writes the
 * NLX_SHA256_COLS x (4 << log_blocks) column-major trace (host or device buffer) and, if digest_out is
 * not NULL, the eight words of the last block's output chaining value (the AIR's public inputs). */
#define NLX_SHA256_COLS 1953
int32_t nlx_sha256_trace(nlx_ctx* ctx, const uint32_t* blocks, const uint8_t* is_first, uint32_t log_blocks,
                         uint64_t* trace_out, uint64_t digest_out[8]);
/* The SHA-256 AIR's binding accumulator (round 1, one column over F_p^2 = two base columns) for the challenge gamma:
 * the running Horner fingerprint of every block's (message-start flag, 16 message words) - absorbed on the block's first
 * row - and 8 output chaining words - on its last row -, each row holding what was absorbed before it.  trace: the
 * round-0 trace; acc_out: 2 x (4 << log_blocks); total_out: the round value the proof sends
 * (near-light-client_amd/sha256_air.py::fingerprint is the relying party's side). */
int32_t nlx_sha256_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_blocks, const uint64_t gamma[2],
                              uint64_t* acc_out, uint64_t total_out[2]);
/* The SHA-512 sibling (column layout and constraints: near-light-client_amd/sha512_air.py; caller in the reference:
 * the SHA-512 of R || A || M inside curta_eddsa_verify_sigs_conditional, nearx/src/builder.rs:152).  blocks:
 * 2^log_blocks padded 1024-bit blocks as 16 big-endian-decoded 64-bit words each.  Writes the NLX_SHA512_COLS x
 * (4 << log_blocks) column-major trace and, if digest_out is not NULL, the eight 64-bit words of the last block's
 * output chaining value (the AIR's sixteen public inputs are their (low, high) 32-bit halves, in that order). */
#define NLX_SHA512_COLS 4745
int32_t nlx_sha512_trace(nlx_ctx* ctx, const uint64_t* blocks, const uint8_t* is_first, uint32_t log_blocks,
                         uint64_t* trace_out, uint64_t digest_out[8]);
/* Round 1 of the SHA-512 AIR: the binding accumulator for gamma (as nlx_sha256_bind_round; 64-bit words are absorbed as
 * (low, high) halves: 33 elements on a block's first row, 16 on its last). */
int32_t nlx_sha512_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_blocks, const uint64_t gamma[2],
                              uint64_t* acc_out, uint64_t total_out[2]);
#ifdef __cplusplus
}
#endif
#endif /* NLX_H */
