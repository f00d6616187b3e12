// The PLONK verifier over BN254 on the device: gnark v0.9 plonk.Verify on the bytes
// of Proof.WriteTo, with kzg.BatchVerifyMultiPoints' two openings folded into one check of two pairs.  Parity with gnark's own
// Verify is UNPINNED like the rest of f.4: the specification is tools/gnark_bsb22_model.py, the model with real pairings
// tools/gnark_plonk_verify_model.py.
//
// Host, per proof (bn254_plonk_verify_host.hpp): decoding, transcript, scalars, the algebraic relation, gamma' and lambda.
// Device, the same four launches for one proof as for a batch (kernel-timing names "bn254_plonk_verify_lincomb_a", "_lincomb_b",
// "bn254_pairing_miller", "bn254_pairing_final_exp"):
//   combination A  k_bn254_g1_lincomb, two segments a proof: the folded H digest and the linearised digest -> back to the host,
//                  whose _batch_gamma hashes their marshalled bytes
//   combination B  two segments a proof, written where the Miller kernel reads its G1 points: the left point as one combination
//                  over the proof's points, the key's points and G, and -(H_b + lambda H_z)
//   k_bn254_miller over two pairs a proof against [1]_2 and [tau]_2; k_bn254_final_exp with one lane a proof, compared with 1
// A proof rejected on the host has no terms: its pairs stay at infinity and its result word is not read.
#include <cstring>
#include <vector>
#include "bn254_g1_lincomb.hpp"
#include "bn254_pairing_launch.hpp"
#include "bn254_plonk_verify_host.hpp"
#include "ctx.hpp"
#include "transcript.hpp"
#include "../../include/nlx.h"

using namespace nlx;

static_assert(pvh::MAX_COMMIT == NLX_BN254_PLONK_MAX_COMMIT, "the host half's commitment bound");
static_assert(pvh::REASON_MALFORMED == NLX_BN254_VERIFY_MALFORMED && pvh::REASON_PAIRING == NLX_BN254_VERIFY_PAIRING &&
              pvh::REASON_ALGEBRAIC == NLX_BN254_VERIFY_ALGEBRAIC, "the host half's reasons");

struct nlx_bn254_plonk_vk {
    nlx_ctx* ctx = nullptr;
    pvh::Key key;
    uint64_t g2[16], g2_tau[16];
    uint64_t* d_points = nullptr;   // (9 + k) x 8 words: the commitments, then G
    std::vector<void*> blocks;
};

namespace {

using pvh::Fr;

void vk_free(nlx_bn254_plonk_vk* vk) {
    if (!vk) return;
    if (vk->ctx) {
        (void)hipStreamSynchronize(vk->ctx->stream);
        for (void* p : vk->blocks) vk->ctx->release(p);
    }
    delete vk;
}

int32_t vk_build(nlx_ctx* ctx, const nlx_bn254_plonk_vk_desc* d, nlx_bn254_plonk_vk* vk) {
    const uint32_t k = d->n_commit;
    if (d->log_n < 3 || d->log_n > 26) return ctx->fail(NLX_E_RANGE, "log_n = %u: 3 .. 26", d->log_n);
    if (k > NLX_BN254_PLONK_MAX_COMMIT) return ctx->fail(NLX_E_RANGE, "%u commitments: at most %u", k, NLX_BN254_PLONK_MAX_COMMIT);
    if (!d->k1 || !d->k2 || !d->commitments || !d->g1 || !d->g2 || !d->g2_tau || (k && !d->commit_rows)) return ctx->fail(NLX_E_INVAL, "NULL argument");
    const uint64_t n = (uint64_t)1 << d->log_n;
    if (d->n_public > n) return ctx->fail(NLX_E_RANGE, "%u public inputs on %llu rows", d->n_public, (unsigned long long)n);
    if (!bnf::below_mod<bnf::RP>(d->k1) || !bnf::below_mod<bnf::RP>(d->k2)) return ctx->fail(NLX_E_RANGE, "k1 / k2 is not below r");
    for (uint32_t j = 0; j < k; j++)
        if (d->commit_rows[j] >= n) return ctx->fail(NLX_E_RANGE, "commitment %u: row %u is not below n", j, d->commit_rows[j]);
    pvh::Key& key = vk->key;
    key.log_n = d->log_n, key.n_public = d->n_public, key.k = k;
    key.k1 = bnf::load_words<bnf::RP>(d->k1), key.k2 = bnf::load_words<bnf::RP>(d->k2);
    memcpy(key.points, d->commitments, (size_t)(8 + k) * 64);
    memcpy(key.points + 8 * key.key_g(), d->g1, 64);
    for (uint32_t j = 0; j < k; j++) key.commit_rows[j] = d->commit_rows[j];
    memcpy(vk->g2, d->g2, 128);
    memcpy(vk->g2_tau, d->g2_tau, 128);
    // every point through the device's checks, as nlx_bn254_groth16_vk_create does
    const size_t n1 = 9 + k;
    uint64_t g2[32];
    memcpy(g2, d->g2, 128);
    memcpy(g2 + 16, d->g2_tau, 128);
    Scratch scratch(ctx);
    uint64_t* d_g2 = scratch.alloc_as<uint64_t>(sizeof g2);
    vk->d_points = (uint64_t*)ctx->alloc(n1 * 64);
    if (vk->d_points) vk->blocks.push_back(vk->d_points);
    if (!d_g2 || !vk->d_points) return scratch.finish(ctx->fail(NLX_E_NOMEM, "verifying key: device memory"));
    auto body = [&]() -> int32_t {
        NLX_HIP(ctx, hipMemcpyAsync(vk->d_points, key.points, n1 * 64, hipMemcpyHostToDevice, ctx->stream));
        NLX_HIP(ctx, hipMemcpyAsync(d_g2, g2, sizeof g2, hipMemcpyHostToDevice, ctx->stream));
        NLX_RC(pairing::check_points(ctx, scratch, vk->d_points, nullptr, n1, "verifying key G1 point (s1 s2 s3 ql qr qm qo qk, the qcp, then g1)"));
        return pairing::check_points(ctx, scratch, nullptr, d_g2, 2, "verifying key G2 point (g2, g2_tau)");
    };
    return scratch.finish(body());
}

const char* reason_text(uint32_t r) {
    return r == NLX_BN254_VERIFY_MALFORMED ? "malformed" : r == NLX_BN254_VERIFY_ALGEBRAIC ? "the algebraic relation fails"
         : r == NLX_BN254_VERIFY_PAIRING ? "the pairing equation fails" : "accepted";
}

// one combination of the batch: the proofs' two segments each -> the flat arrays the kernel reads
struct Flat {
    std::vector<uint32_t> src, first;
    std::vector<uint64_t> scalars;
    void begin() { first.assign(1, 0); }
    void segment(const std::vector<pvh::Term>* terms, uint32_t proof_base) {
        for (size_t t = 0; terms && t < terms->size(); t++) {
            const pvh::Term& x = (*terms)[t];
            src.push_back(x.src < pvh::SRC_PROOF ? x.src : proof_base + (x.src - pvh::SRC_PROOF));
            uint64_t w[4];
            bnf::store_words(x.scalar, w);
            scalars.insert(scalars.end(), w, w + 4);
        }
        first.push_back((uint32_t)src.size());
    }
};

int32_t verify_body(const nlx_bn254_plonk_vk* vk, Scratch& scratch, const uint8_t* const* proofs, const size_t* lens, size_t n,
                    const uint64_t* public_inputs, nlx_bn254_verdict* verdicts) {
    nlx_ctx* ctx = vk->ctx;
    const pvh::Key& key = vk->key;
    const uint32_t np = key.n_public, kp = 9 + key.k, pp = key.proof_points();
    std::vector<Fr> publics(n * (size_t)np);
    for (size_t i = 0; i < publics.size(); i++) {
        if (!bnf::below_mod<bnf::RP>(public_inputs + 4 * i)) return ctx->fail(NLX_E_RANGE, "proof %zu, public input %zu is not below r", i / np, i % np);
        publics[i] = bnf::load_words<bnf::RP>(public_inputs + 4 * i);
    }
    std::vector<pvh::Proof> dec(n);
    // the points of every combination: the key's, then the proofs' back to back (a rejected proof's stay zero and are not named)
    std::vector<uint64_t> points((size_t)n * pp * 8, 0);
    for (size_t i = 0; i < n; i++) {
        pvh::decode(key, proofs[i], lens[i], dec[i]);
        if (!dec[i].rejected()) pvh::relation(key, publics.data() + i * np, dec[i]);
        if (!dec[i].rejected()) memcpy(&points[i * pp * 8], dec[i].points, (size_t)pp * 64);
    }
    const size_t n_seg = 2 * n, max_terms = n * (size_t)(20 + 2 * key.k);
    if (n_seg > pairing::MAX_PAIRS) return ctx->fail(NLX_E_RANGE, "at most 2^19 proofs per call");
    uint64_t* d_points = scratch.alloc_as<uint64_t>(((size_t)kp + n * pp) * 64);
    uint64_t* d_scalars = scratch.alloc_as<uint64_t>((max_terms + 1) * 32);
    uint32_t* d_words = scratch.alloc_as<uint32_t>((max_terms + 2 * (n_seg + 1)) * 4);   // src | first | the Miller offsets
    uint64_t* d_a = scratch.alloc_as<uint64_t>(n_seg * 64);
    uint64_t* d_g1 = scratch.alloc_as<uint64_t>(n_seg * 64);
    uint64_t* d_g2 = scratch.alloc_as<uint64_t>(n_seg * 128);
    uint32_t* d_result = scratch.alloc_as<uint32_t>(n * 4);
    if (!d_points || !d_scalars || !d_words || !d_a || !d_g1 || !d_g2 || !d_result) return ctx->fail(NLX_E_NOMEM, "plonk verify: device memory");
    hipStream_t st = ctx->stream;
    NLX_HIP(ctx, hipMemcpyAsync(d_points, vk->d_points, (size_t)kp * 64, hipMemcpyDeviceToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_points + (size_t)kp * 8, points.data(), points.size() * 8, hipMemcpyHostToDevice, st));
    Flat flat;
    auto run = [&](bool second, uint64_t* d_out) -> int32_t {
        flat.src.clear();
        flat.scalars.clear();
        flat.begin();
        for (size_t i = 0; i < n; i++) {
            const bool live = !dec[i].rejected();
            flat.segment(live ? (second ? &dec[i].b0 : &dec[i].a0) : nullptr, (uint32_t)(kp + i * pp));
            flat.segment(live ? (second ? &dec[i].b1 : &dec[i].a1) : nullptr, (uint32_t)(kp + i * pp));
        }
        const size_t n_terms = flat.src.size();
        if (n_terms > max_terms) return ctx->fail(NLX_E_INVAL, "plonk verify: %zu terms, room for %zu", n_terms, max_terms);
        if (n_terms) {
            NLX_HIP(ctx, hipMemcpyAsync(d_scalars, flat.scalars.data(), n_terms * 32, hipMemcpyHostToDevice, st));
            NLX_HIP(ctx, hipMemcpyAsync(d_words, flat.src.data(), n_terms * 4, hipMemcpyHostToDevice, st));
        }
        NLX_HIP(ctx, hipMemcpyAsync(d_words + max_terms, flat.first.data(), (n_seg + 1) * 4, hipMemcpyHostToDevice, st));
        return lincomb::enqueue(ctx, d_points, d_words, d_scalars, d_words + max_terms, n_seg, n_terms, d_out,
                                second ? "bn254_plonk_verify_lincomb_b" : "bn254_plonk_verify_lincomb_a");
    };
    // combination A and its points back: the host hashes their bytes
    NLX_RC(run(false, d_a));
    std::vector<uint64_t> a(n_seg * 8);
    NLX_RC(fetch(ctx, a.data(), d_a, a.size() * 8));   // synchronises: `flat` is free again
    for (size_t i = 0; i < n; i++)
        if (!dec[i].rejected()) pvh::fold(key, &a[16 * i], &a[16 * i + 8], dec[i]);
    // combination B writes the Miller kernel's G1 side: pair 2 i = (left, [1]_2), pair 2 i + 1 = (-(H_b + lambda H_z), [tau]_2)
    NLX_RC(run(true, d_g1));
    std::vector<uint64_t> g2(n_seg * 16, 0);
    std::vector<uint32_t> first(n + 1);
    for (size_t i = 0; i <= n; i++) first[i] = (uint32_t)(2 * i);
    for (size_t i = 0; i < n; i++) {
        if (dec[i].rejected()) continue;
        memcpy(&g2[32 * i], vk->g2, 128);
        memcpy(&g2[32 * i + 16], vk->g2_tau, 128);
    }
    uint32_t* d_first = d_words + max_terms + n_seg + 1;
    NLX_HIP(ctx, hipMemcpyAsync(d_g2, g2.data(), g2.size() * 8, hipMemcpyHostToDevice, st));
    NLX_HIP(ctx, hipMemcpyAsync(d_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, st));
    NLX_RC(pairing::enqueue_checks(ctx, scratch, d_g1, d_g2, n_seg, d_first, n, 0, nullptr, 0, nullptr, d_result));
    std::vector<uint32_t> res(n);
    NLX_RC(fetch(ctx, res.data(), d_result, n * 4));
    bool named = false;
    for (size_t i = 0; i < n; i++) {
        nlx_bn254_verdict& v = verdicts[i];
        if (dec[i].rejected()) {
            v.reason = dec[i].reason;
            v.index = dec[i].index;
        } else {
            if (res[i] > 1) return ctx->fail(NLX_E_HIP, "plonk verify: the final exponentiation wrote no result for proof %zu", i);
            if (res[i]) v.accepted = 1;
            else v.reason = NLX_BN254_VERIFY_PAIRING;
        }
        if (!v.accepted && !named) {
            named = true;
            ctx->fail(NLX_OK, "proof %zu rejected: %s (index %u)", i, reason_text(v.reason), v.index);
        }
    }
    return NLX_OK;
}

}  // namespace

extern "C" int32_t nlx_bn254_plonk_vk_create(nlx_ctx* ctx, const nlx_bn254_plonk_vk_desc* desc, nlx_bn254_plonk_vk** out) NLX_TRY {
    if (!ctx) return NLX_E_INVAL;
    if (!desc || !out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    nlx_bn254_plonk_vk* vk = new nlx_bn254_plonk_vk();
    vk->ctx = ctx;
    const int32_t rc = vk_build(ctx, desc, vk);
    if (rc) {
        vk_free(vk);
        return rc;
    }
    *out = vk;
    return NLX_OK;
} NLX_CATCH(ctx)

extern "C" void nlx_bn254_plonk_vk_destroy(nlx_bn254_plonk_vk* vk) NLX_TRY {
    vk_free(vk);
} NLX_CATCH_VOID(nullptr)

extern "C" int32_t nlx_bn254_plonk_verify_batch(const nlx_bn254_plonk_vk* vk, const uint8_t* const* proofs, const size_t* lens, size_t n_proofs,
                                                const uint64_t* public_inputs, nlx_bn254_verdict* verdicts) NLX_TRY {
    if (!vk) return NLX_E_INVAL;
    nlx_ctx* ctx = vk->ctx;
    for (size_t i = 0; verdicts && i < n_proofs; i++) verdicts[i] = nlx_bn254_verdict{0, 0, 0};
    if (n_proofs && (!proofs || !lens || !verdicts || (vk->key.n_public && !public_inputs))) return ctx->fail(NLX_E_INVAL, "NULL argument");
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (n_proofs > ((size_t)1 << 17)) return ctx->fail(NLX_E_RANGE, "at most 2^17 proofs per call");
    if (!n_proofs) return NLX_OK;
    (void)hipSetDevice(ctx->device);
    if (vk->key.n_public && is_device_ptr(public_inputs)) return ctx->fail(NLX_E_INVAL, "public_inputs is a host array");
    Scratch scratch(ctx);
    return scratch.finish(verify_body(vk, scratch, proofs, lens, n_proofs, public_inputs, verdicts));
} NLX_CATCH(vk ? vk->ctx : nullptr)

extern "C" int32_t nlx_bn254_plonk_verify(const nlx_bn254_plonk_vk* vk, const uint8_t* proof, size_t len, const uint64_t* public_inputs,
                                          nlx_bn254_verdict* verdict) NLX_TRY {
    if (!vk) return NLX_E_INVAL;
    if (verdict) *verdict = nlx_bn254_verdict{0, 0, 0};
    if (!proof || !verdict) return vk->ctx->fail(NLX_E_INVAL, "NULL argument");
    return nlx_bn254_plonk_verify_batch(vk, &proof, &len, 1, public_inputs, verdict);
} NLX_CATCH(vk ? vk->ctx : nullptr)
