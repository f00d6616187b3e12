// The host half of the PLONK verifier (bn254_plonk_verify.hip): gnark v0.9 plonk.Verify on the bytes of
// Proof.WriteTo as tools/gnark_bsb22_model.py states it (rules 5, 7, 8, 9, 10, _lin_scalars, _batch_gamma, proof_from_bytes) -
// decoding and square roots, the SHA-256 transcript, the Bsb22 hashes, every scalar in Fr, the algebraic relation, and the
// scalars of the two device combinations.  Plain C++ over bn254_gnark_bytes.hpp: builds with g++
// (tests/native/bn254_plonk_verify_host_check.cpp compares it with vectors the model writes).
//
// The three steps of one proof:
//   decode()     bytes -> points and values; MALFORMED names the first offending field
//   relation()   gamma beta alpha zeta, the Lagrange values (ONE inversion, a batch inversion of the denominators; an inverse
//                of 0 is 0), PI(zeta) with the Bsb22 terms, the algebraic relation; the terms of combination A:
//                segment 0 = H1 + zeta^(n+2) H2 + zeta^(2n+4) H3, segment 1 = the linearised digest
//   fold()       with A's two points: gamma' (_batch_gamma hashes their marshalled bytes), lambda, the terms of combination B:
//                segment 0 = D_f + lambda Z - (v_f + lambda z_w) G + zeta H_b + lambda zeta w H_z with D_f spelled out over
//                the proof's and the key's points, segment 1 = -(H_b + lambda H_z)
// The lambda rule (stated once more in include/nlx.h): lambda = fr.Hash(zeta || gamma' || Z.Marshal() || H_b.Marshal() ||
// H_z.Marshal() || v_f || z_w, dst "nlx-plonk-kzg-fold"), 1 in place of 0.  gamma' stands for the folded digest D_f: it is a hash
// over zeta, every digest D_i and every claimed value, so it binds D_f = sum gamma'^i D_i, which is never computed on its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "bn254_gnark_bytes.hpp"

namespace nlx {
namespace pvh {

using namespace bnf;
using ppr::Fr;

constexpr uint32_t MAX_COMMIT = 4;   // NLX_BN254_PLONK_MAX_COMMIT
constexpr uint32_t REASON_ACCEPT = 0, REASON_MALFORMED = 1, REASON_PAIRING = 3, REASON_ALGEBRAIC = 4;   // NLX_BN254_VERIFY_*
// where a term's point lies: below SRC_PROOF a point of the key (KEY_*), from SRC_PROOF up a point of the proof (PROOF_*)
constexpr uint32_t SRC_PROOF = 16;
enum { KEY_S1 = 0, KEY_S2, KEY_S3, KEY_QL, KEY_QR, KEY_QM, KEY_QO, KEY_QK, KEY_QCP0 };   // nlx_bn254_plonk_key_commitments' order; G follows the last qcp
enum { PROOF_L = 0, PROOF_R, PROOF_O, PROOF_Z, PROOF_H1, PROOF_H2, PROOF_H3, PROOF_PI2_0 };   // byte order; H_b and H_z follow the last PI2

struct Key {
    uint32_t log_n = 0, n_public = 0, k = 0;
    Fr k1, k2;                                        // Montgomery
    uint64_t points[(9 + MAX_COMMIT) * 8] = {};       // the 8 + k commitments, then G
    uint32_t commit_rows[MAX_COMMIT] = {};
    uint32_t key_g() const { return 8 + k; }
    uint32_t proof_hb() const { return 7 + k; }
    uint32_t proof_hz() const { return 8 + k; }
    uint32_t proof_points() const { return 9 + k; }
    size_t proof_length() const { return 7 * 32 + 4 + 32 * (size_t)k + 32 + 4 + 32 * (size_t)(7 + k) + 64; }
};

struct Term {
    uint32_t src;
    Fr scalar;   // the canonical integer, as the kernel reads it
};

struct Proof {
    uint32_t reason = REASON_ACCEPT, index = 0;       // set by the step that rejects; nothing after it runs
    uint64_t points[(9 + MAX_COMMIT) * 8];            // PROOF_* order
    Fr vals[7 + MAX_COMMIT], zw;                      // folded_h lin l r o s1 s2 qcp_j at zeta, z at zeta w; Montgomery
    Fr gamma, beta, alpha, zeta, gp, lambda, vf;      // Montgomery
    std::vector<Term> a0, a1, b0, b1;                 // the segments of the two combinations
    bool rejected() const { return reason != REASON_ACCEPT; }
};

inline void push(std::vector<Term>& seg, uint32_t src, const Fr& mont) { seg.push_back(Term{src, from_mont(mont)}); }

// 32 big-endian bytes -> the element (Montgomery); false if the integer is not below r
inline bool fr_from_be_below(const uint8_t* b, Fr& out) {
    Fr a;
    for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)b[31 - 4 * i] | (uint32_t)b[30 - 4 * i] << 8 | (uint32_t)b[29 - 4 * i] << 16 | (uint32_t)b[28 - 4 * i] << 24;
    if (geq_mod(a)) return false;
    out = to_mont(a);
    return true;
}
inline uint32_t be_u32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// rule 10.  index: 0 the length or a count; points 0 L, 1 R, 2 O, 3 Z, 4 .. 6 H1 .. H3, 7 + j PI2_j, 7 + k H_b, 8 + k H_z; values
// 9 + k + i claimed value i, 16 + 2 k the shifted value.  After the length, the fields are judged in byte order.
inline void decode(const Key& key, const uint8_t* p, size_t len, Proof& o) {
    const uint32_t k = key.k;
    auto bad = [&](uint32_t index) {
        o.reason = REASON_MALFORMED;
        o.index = index;
    };
    o.reason = REASON_ACCEPT;
    o.index = 0;
    if (len != key.proof_length()) return bad(0);
    size_t off = 0;
    for (uint32_t i = 0; i < 7; i++, off += 32)
        if (!ppr::g1_decode(p + off, o.points + 8 * i)) return bad(i);
    if (be_u32(p + off) != k) return bad(0);
    off += 4;
    for (uint32_t j = 0; j < k; j++, off += 32)
        if (!ppr::g1_decode(p + off, o.points + 8 * (PROOF_PI2_0 + j))) return bad(7 + j);
    if (!ppr::g1_decode(p + off, o.points + 8 * key.proof_hb())) return bad(7 + k);
    off += 32;
    if (be_u32(p + off) != 7 + k) return bad(0);
    off += 4;
    for (uint32_t i = 0; i < 7 + k; i++, off += 32)
        if (!fr_from_be_below(p + off, o.vals[i])) return bad(9 + k + i);
    if (!ppr::g1_decode(p + off, o.points + 8 * key.proof_hz())) return bad(8 + k);
    off += 32;
    if (!fr_from_be_below(p + off, o.zw)) return bad(16 + 2 * k);
}

// every x_i -> 1 / x_i with one inversion; the inverse of 0 is 0 (the model's pow(0, r - 2, r))
inline void batch_inverse(std::vector<Fr>& x) {
    std::vector<Fr> prefix(x.size());
    Fr acc = one<RP>();
    for (size_t i = 0; i < x.size(); i++) {
        prefix[i] = acc;
        if (!is_zero(x[i])) acc = mul(acc, x[i]);
    }
    Fr inv = inv_host(acc);
    for (size_t i = x.size(); i-- > 0;) {
        if (is_zero(x[i])) continue;
        const Fr xi = x[i];
        x[i] = mul(inv, prefix[i]);
        inv = mul(inv, xi);
    }
}

inline Fr root_of_unity(uint32_t log_n) {
    Fr w = root28();
    for (uint32_t i = log_n; i < 28; i++) w = sqr(w);
    return w;
}

const uint8_t BSB22_DST[] = "BSB22-Plonk", FOLD_DST[] = "nlx-plonk-kzg-fold";

// rules 5, 7, 9 and the relation.  publics: n_public elements, Montgomery, below r.
inline void relation(const Key& key, const Fr* publics, Proof& o) {
    const uint32_t k = key.k;
    const uint64_t n = (uint64_t)1 << key.log_n;
    const Fr one_m = one<RP>();
    auto pt = [&](uint32_t i) { return o.points + 8 * i; };
    ppr::Challenge gamma_c("gamma", nullptr);
    for (uint32_t i = 0; i < 8 + k; i++) gamma_c.bind_point(key.points + 8 * i);
    for (uint32_t i = 0; i < key.n_public; i++) gamma_c.bind_fr(publics[i]);
    for (uint32_t i = PROOF_L; i <= PROOF_O; i++) gamma_c.bind_point(pt(i));
    const Fr gamma = o.gamma = gamma_c.value();
    ppr::Challenge beta_c("beta", &gamma_c);
    const Fr beta = o.beta = beta_c.value();
    ppr::Challenge alpha_c("alpha", &beta_c);
    for (uint32_t j = 0; j < k; j++) alpha_c.bind_point(pt(PROOF_PI2_0 + j));
    alpha_c.bind_point(pt(PROOF_Z));
    const Fr alpha = o.alpha = alpha_c.value();
    ppr::Challenge zeta_c("zeta", &alpha_c);
    for (uint32_t i = PROOF_H1; i <= PROOF_H3; i++) zeta_c.bind_point(pt(i));
    const Fr zeta = o.zeta = zeta_c.value();

    const Fr folded_h_zeta = o.vals[0], lin_zeta = o.vals[1], l = o.vals[2], r = o.vals[3], oz = o.vals[4], s1 = o.vals[5], s2 = o.vals[6], zw = o.zw;
    Fr zeta_n = zeta;
    for (uint32_t i = 0; i < key.log_n; i++) zeta_n = sqr(zeta_n);
    const Fr zh = sub(zeta_n, one_m), n_m = ppr::fr_small(n), w = root_of_unity(key.log_n);
    // the Lagrange denominators n (zeta - w^i): row 0 (L_1 of the relation; also public input 0), the public rows, the commitment rows
    std::vector<Fr> wpow(1 + (size_t)key.n_public + k), den(wpow.size());
    Fr wi = one_m;
    for (uint32_t i = 0; i < key.n_public; i++) {
        wpow[1 + i] = wi;
        wi = mul(wi, w);
    }
    wpow[0] = one_m;
    for (uint32_t j = 0; j < k; j++) wpow[1 + key.n_public + j] = pow_host(w, key.commit_rows[j]);
    for (size_t i = 0; i < den.size(); i++) den[i] = mul(n_m, sub(zeta, wpow[i]));
    batch_inverse(den);
    auto lagrange = [&](size_t i) { return mul(mul(wpow[i], zh), den[i]); };
    const Fr l1 = lagrange(0);
    Fr pi = zero<RP>();
    for (uint32_t i = 0; i < key.n_public; i++) pi = add(pi, mul(publics[i], lagrange(1 + i)));
    for (uint32_t j = 0; j < k; j++) {
        uint8_t m[64];
        ppr::g1_marshal(pt(PROOF_PI2_0 + j), m);
        pi = add(pi, mul(ppr::hash_to_field(m, 64, BSB22_DST, sizeof BSB22_DST - 1), lagrange(1 + key.n_public + j)));
    }
    // _lin_scalars
    const Fr bz = mul(beta, zeta);
    const Fr a_ = mul(mul(add(add(l, bz), gamma), add(add(r, mul(bz, key.k1)), gamma)), add(add(oz, mul(bz, key.k2)), gamma));
    const Fr b_ = mul(add(add(l, mul(beta, s1)), gamma), add(add(r, mul(beta, s2)), gamma));
    const Fr alpha2 = sqr(alpha), ab = mul(alpha, b_);
    const Fr sc_z = add(mul(alpha, a_), mul(alpha2, l1)), sc_s3 = neg(mul(mul(ab, beta), zw));
    // lin(zeta) + PI(zeta) - alpha b (o + gamma) z_w - alpha^2 L_1(zeta) = folded_h(zeta) (zeta^n - 1)
    const Fr lhs = sub(sub(add(lin_zeta, pi), mul(mul(ab, add(oz, gamma)), zw)), mul(alpha2, l1));
    if (!equal(lhs, mul(folded_h_zeta, zh))) {
        o.reason = REASON_ALGEBRAIC;
        o.index = 0;
        return;
    }
    const Fr zn2 = mul(zeta_n, sqr(zeta));
    o.a0.clear();
    o.a1.clear();
    push(o.a0, SRC_PROOF + PROOF_H1, one_m);
    push(o.a0, SRC_PROOF + PROOF_H2, zn2);
    push(o.a0, SRC_PROOF + PROOF_H3, sqr(zn2));
    push(o.a1, KEY_QM, mul(l, r));
    push(o.a1, KEY_QL, l);
    push(o.a1, KEY_QR, r);
    push(o.a1, KEY_QO, oz);
    push(o.a1, KEY_QK, one_m);
    push(o.a1, SRC_PROOF + PROOF_Z, sc_z);
    push(o.a1, KEY_S3, sc_s3);
    for (uint32_t j = 0; j < k; j++) push(o.a1, SRC_PROOF + PROOF_PI2_0 + j, o.vals[7 + j]);
}

// rule 8 and the fold of the two openings.  folded_h, lin: combination A's two points (G1Affine words).
inline void fold(const Key& key, const uint64_t folded_h[8], const uint64_t lin[8], Proof& o) {
    const uint32_t k = key.k;
    auto pt = [&](uint32_t i) { return o.points + 8 * i; };
    ppr::Challenge gp_c("gamma", nullptr);
    gp_c.bind_fr(o.zeta);
    gp_c.bind_point(folded_h);
    gp_c.bind_point(lin);
    for (uint32_t i = PROOF_L; i <= PROOF_O; i++) gp_c.bind_point(pt(i));
    gp_c.bind_point(key.points + 8 * KEY_S1);
    gp_c.bind_point(key.points + 8 * KEY_S2);
    for (uint32_t j = 0; j < k; j++) gp_c.bind_point(key.points + 8 * (KEY_QCP0 + j));
    for (uint32_t i = 0; i < 7 + k; i++) gp_c.bind_fr(o.vals[i]);
    const Fr gp = o.gp = gp_c.value();
    Fr g[7 + MAX_COMMIT], vf = zero<RP>();
    g[0] = one<RP>();
    for (uint32_t i = 1; i < 7 + k; i++) g[i] = mul(g[i - 1], gp);
    for (uint32_t i = 0; i < 7 + k; i++) vf = add(vf, mul(g[i], o.vals[i]));
    o.vf = vf;
    uint8_t msg[32 * 4 + 64 * 3];
    ppr::be32(o.zeta, msg);
    ppr::be32(gp, msg + 32);
    ppr::g1_marshal(pt(PROOF_Z), msg + 64);
    ppr::g1_marshal(pt(key.proof_hb()), msg + 128);
    ppr::g1_marshal(pt(key.proof_hz()), msg + 192);
    ppr::be32(vf, msg + 256);
    ppr::be32(o.zw, msg + 288);
    Fr lambda = ppr::hash_to_field(msg, sizeof msg, FOLD_DST, sizeof FOLD_DST - 1);
    if (is_zero(lambda)) lambda = one<RP>();
    o.lambda = lambda;
    // D_f = g0 (H1 + zn2 H2 + zn2^2 H3) + g1 lin + g2 L + g3 R + g4 O + g5 S1 + g6 S2 + g_(7+j) Qcp_j, lin spelled out (a1's terms)
    o.b0.clear();
    o.b1.clear();
    for (const Term& t : o.a0) o.b0.push_back(t);
    for (const Term& t : o.a1) {
        Fr s = mul(to_mont(t.scalar), gp);
        if (t.src == SRC_PROOF + PROOF_Z) s = add(s, lambda);   // + lambda Z
        push(o.b0, t.src, s);
    }
    push(o.b0, SRC_PROOF + PROOF_L, g[2]);
    push(o.b0, SRC_PROOF + PROOF_R, g[3]);
    push(o.b0, SRC_PROOF + PROOF_O, g[4]);
    push(o.b0, KEY_S1, g[5]);
    push(o.b0, KEY_S2, g[6]);
    for (uint32_t j = 0; j < k; j++) push(o.b0, KEY_QCP0 + j, g[7 + j]);
    push(o.b0, key.key_g(), neg(add(vf, mul(lambda, o.zw))));
    push(o.b0, SRC_PROOF + key.proof_hb(), o.zeta);
    push(o.b0, SRC_PROOF + key.proof_hz(), mul(mul(lambda, o.zeta), root_of_unity(key.log_n)));
    push(o.b1, SRC_PROOF + key.proof_hb(), neg(one<RP>()));
    push(o.b1, SRC_PROOF + key.proof_hz(), neg(lambda));
}

}  // namespace pvh
}  // namespace nlx
