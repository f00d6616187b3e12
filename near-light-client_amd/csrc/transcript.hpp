// Host-side Fiat-Shamir transcript, proof byte writer and the pinned device->host fetch shared by the
// plonky2 prover (prover.hip), the generic FRI prover (fri.hip) and the STARK prover (stark.hip).
#pragma once
#include <cstring>
#include <stdint.h>
#include <stddef.h>
#include "ctx.hpp"
#include "gl.hpp"
#include "poseidon.hpp"
#include "poseidon_bn128.hpp"

namespace nlx {

// plonky2::iop::challenger::Challenger (host)
struct Challenger {
    uint64_t state[12] = {0};
    uint64_t in_buf[8];
    unsigned n_in = 0;
    uint64_t out_buf[8];
    unsigned n_out = 0;
    void duplex() {
        for (unsigned i = 0; i < n_in; i++) state[i] = in_buf[i];
        n_in = 0;
        poseidon::permute(state);
        for (int i = 0; i < 8; i++) out_buf[i] = state[i];
        n_out = 8;
    }
    void observe(uint64_t e) {
        n_out = 0;
        in_buf[n_in++] = e;
        if (n_in == 8) duplex();
    }
    void observe(const uint64_t* e, size_t n) {
        for (size_t i = 0; i < n; i++) observe(e[i]);
    }
    uint64_t challenge() {
        if (n_in != 0 || n_out == 0) duplex();
        return out_buf[--n_out];
    }
    void ext_challenge(uint64_t out[2]) {
        out[0] = challenge();
        out[1] = challenge();
    }
};

// GenericHashOut::to_vec of a PoseidonBN128 digest (plonky2x plonky2_config.rs, recalled - tools/bn128_config_model.py rule 2):
// the 32 little-endian bytes of the canonical value cut into chunks of 7, 7, 7, 7 and 4 bytes, each a Goldilocks element
// (limbs 0..3 < 2^56, limb 4 < 2^32)
constexpr int BN128_DIGEST_LIMBS = 5;
inline void bn128_digest_limbs(const uint64_t w[4], uint64_t out[BN128_DIGEST_LIMBS]) {
    constexpr uint64_t M56 = ((uint64_t)1 << 56) - 1;
    out[0] = w[0] & M56;
    out[1] = ((w[0] >> 56) | (w[1] << 8)) & M56;
    out[2] = ((w[1] >> 48) | (w[2] << 16)) & M56;
    out[3] = ((w[2] >> 40) | (w[3] << 24)) & M56;
    out[4] = w[3] >> 32;
}

// Challenger::observe_hash / observe_cap for the config's Hasher: `n` digests of four little-endian words.  Goldilocks digests
// are their own four elements; a BN128 digest enters as its five limbs and must be canonical (NLX_E_RANGE otherwise, nothing
// observed).  The sponge itself stays the Goldilocks permutation under both configs.
inline int32_t observe_hash(uint32_t hasher, Challenger& ch, const uint64_t* digests, size_t n) {
    if (hasher == NLX_HASHER_POSEIDON_GOLDILOCKS) {
        ch.observe(digests, 4 * n);
        return NLX_OK;
    }
    for (size_t i = 0; i < n; i++)
        if (!pbn::lt_r(digests[4 * i], digests[4 * i + 1], digests[4 * i + 2], digests[4 * i + 3])) return NLX_E_RANGE;
    for (size_t i = 0; i < n; i++) {
        uint64_t l[BN128_DIGEST_LIMBS];
        bn128_digest_limbs(digests + 4 * i, l);
        ch.observe(l, BN128_DIGEST_LIMBS);
    }
    return NLX_OK;
}

// PoseidonBN128Hash::hash_no_pad on the host (the circuit digest under the BN128 config: a dozen permutations, once per circuit):
// the absorption of poseidon_bn128.hip's pbn_absorb, canonical elements in, the canonical digest out as four words
inline void bn128_hash_no_pad_host(const uint64_t* in, size_t len, uint64_t out[4]) {
    pbn::Fe s[pbn::T];
    for (int i = 0; i < pbn::T; i++) s[i] = f29::zero();
    for (size_t off = 0; off < len; off += pbn::CHUNK) {
        uint64_t e[pbn::CHUNK] = {0};
        const size_t k = len - off < (size_t)pbn::CHUNK ? len - off : (size_t)pbn::CHUNK;
        for (size_t j = 0; j < k; j++) e[j] = in[off + j];
        for (size_t g = 0; 3 * g < k; g++) s[g + 1] = pbn::from_gl3(e[3 * g], e[3 * g + 1], e[3 * g + 2]);
        pbn::permute(s);
    }
    pbn::to_words(s[0], out);
}

inline void hash_no_pad_host(const uint64_t* in, size_t len, uint64_t out[4]) {
    uint64_t st[12] = {0};
    for (size_t off = 0; off < len; off += 8) {
        size_t k = len - off < 8 ? len - off : 8;
        for (size_t j = 0; j < k; j++) st[j] = in[off + j];
        poseidon::permute(st);
    }
    memcpy(out, st, 32);
}

// plonky2::util::serialization::Buffer (write side), little-endian
struct Writer {
    uint8_t* p;
    size_t len = 0, cap;
    bool overflow = false;
    void bytes(const void* src, size_t n) {
        if (len + n > cap) { overflow = true; return; }
        memcpy(p + len, src, n);
        len += n;
    }
    void u64s(const uint64_t* v, size_t n) { bytes(v, n * 8); }
    void u8(uint8_t v) { bytes(&v, 1); }
    void usize(uint64_t v) { bytes(&v, 8); }  // Write::write_usize: 8 little-endian bytes
};

// plonky2::fri::reduction_strategies::FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits)
inline uint32_t fri_num_rounds(uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t arity_bits,
                               uint32_t final_poly_bits) {
    uint32_t r = 0;
    while (degree_bits > final_poly_bits && degree_bits + rate_bits >= cap_height + arity_bits) {
        if (degree_bits < arity_bits) break;
        degree_bits -= arity_bits;
        r++;
    }
    return r;
}

inline int32_t ensure_pinned(nlx_ctx* ctx, size_t bytes) {
    if (ctx->pinned_bytes >= bytes) return NLX_OK;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    hipError_t e = hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipHostMalloc");
    ctx->pinned_bytes = bytes;
    return NLX_OK;
}

// device -> host through the pinned staging buffer, synchronous.  `last`: this read ends the call that owns that Scratch -
// its synchronise is last->drain(), so the Scratch's destructor has nothing left to wait for.
inline int32_t fetch(nlx_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, Scratch* last = nullptr) {
    int32_t rc = ensure_pinned(ctx, bytes < (1u << 20) ? (1u << 20) : bytes);
    if (rc) return rc;
    NLX_HIP(ctx, hipMemcpyAsync(ctx->pinned, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    const hipError_t e = last ? last->drain() : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipStreamSynchronize(ctx->stream)");
    memcpy(host_dst, ctx->pinned, bytes);
    return NLX_OK;
}

}  // namespace nlx
