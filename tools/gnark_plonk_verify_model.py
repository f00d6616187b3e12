#!/usr/bin/env python3
"""gnark v0.9 plonk.Verify over BN254 on big integers WITH the pairings: what the device verifier (csrc/bn254_plonk_verify.hip,
DESIGN.md section 32) is compared with.  Test infrastructure.  The parsing and every scalar rule are tools/gnark_bsb22_model.py's
(proof_from_bytes, _bind_key, _lin_scalars, _batch_gamma, hash_to_field: rules 5, 7, 8, 9, 10), the pairings
tools/bn254_pairing_model.py's.  The two KZG openings are checked SEPARATELY, each as

    e(C - v G + z H, [1]_2) e(-H, [tau]_2) = 1

(the batch at zeta with the folded digest and value, Z at zeta w), so there is no lambda here and no folding shared with the
device, which checks the two at once.  Status: RECALLED, UNPINNED like gnark_bsb22_model itself.

verify() -> (accepted, reason, index): reason MALFORMED / ALGEBRAIC / PAIRING in that order, index naming a malformed proof's
first offending field: 0 the length or a count that does not fit; points 0 L, 1 R, 2 O, 3 Z, 4 .. 6 H1 .. H3, 7 + j PI2_j, 7 + k the
batched opening's H, 8 + k the shifted opening's H (a bad flag byte, a coordinate >= q, an x with no y; the compressed point at
infinity is valid); values not below r: 9 + k + i claimed value i, 16 + 2 k the shifted value.  After the length the fields are
judged in byte order."""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import bn254_py as bn  # noqa: E402
import bn254_pairing_model as pm  # noqa: E402
import gnark_bsb22_model as gm  # noqa: E402

R, Q = bn.R, bn.Q
ACCEPT, MALFORMED, PAIRING, ALGEBRAIC = 0, 1, 3, 4


def point_fault(b):
    """is this 32-byte string NOT what G1Affine.SetBytes takes?  (gnark_bsb22_model's parser is laxer: it reads the flag 0b00 as
    0b10, ignores the rest of an infinity string and reduces x mod q)"""
    flag = b[0] >> 6
    if flag == 1:
        return b != bytes([0x40]) + bytes(31)
    if flag == 0:
        return True
    x = int.from_bytes(bytes([b[0] & 0x3F]) + b[1:], "big")
    if x >= Q:
        return True
    rhs = (x * x * x + 3) % Q
    return pow(rhs, (Q - 1) // 2, Q) != 1 and rhs != 0


def malformed_index(data, k):
    """None, or the index of the first offending field"""
    data = bytes(data)
    if len(data) != gm.proof_length(k):
        return 0
    reg = gm.proof_regions(k)
    part = lambda name: data[reg[name][0]:reg[name][0] + reg[name][1]]
    for i, name in enumerate(("l", "r", "o", "z", "h1", "h2", "h3")):
        if point_fault(part(name)):
            return i
    if int.from_bytes(part("bsb22_count"), "big") != k:
        return 0
    for j in range(k):
        if point_fault(part("bsb22_%d" % j)):
            return 7 + j
    if point_fault(part("batched_h")):
        return 7 + k
    if int.from_bytes(part("claimed_count"), "big") != 7 + k:
        return 0
    names = ["folded_h", "lin", "l_zeta", "r_zeta", "o_zeta", "s1_zeta", "s2_zeta"] + ["qcp%d_zeta" % j for j in range(k)]
    for i, name in enumerate(names):
        if int.from_bytes(part(name), "big") >= R:
            return 9 + k + i
    if point_fault(part("z_shifted_h")):
        return 8 + k
    if int.from_bytes(part("z_shifted_value"), "big") >= R:
        return 16 + 2 * k
    return None


def opening_holds(c, v, z, h, g2, g2_tau):
    """e(C - v G + z H, [1]_2) e(-H, [tau]_2) = 1"""
    left = bn.g1_add(bn.g1_add(c, bn.g1_neg(bn.g1_mul(v % R, bn.G1))), bn.g1_mul(z % R, h))
    return pm.pairing_product([(left, g2), (bn.g1_neg(h), g2_tau)]) == pm.F12_ONE


def derive(proof, vk, n, k1, k2, public=()):
    """every value the verifier derives from a parsed proof, by name: the challenges, the scalars of the linearised digest, whether
    the algebraic relation holds and - if it does - the two digests, gamma' and the folded digest and value"""
    k = len(vk["qcp"])
    w = bn.root_of_unity(n.bit_length() - 1)
    fs = bn.GnarkTranscript("gamma", "beta", "alpha", "zeta")
    gm._bind_key(fs, vk, public)
    for c in proof["lro"]:
        fs.bind("gamma", bn.g1_marshal(c))
    gamma, beta = fs.challenge("gamma"), fs.challenge("beta")
    for c in proof["bsb22"]:
        fs.bind("alpha", bn.g1_marshal(c))
    fs.bind("alpha", bn.g1_marshal(proof["z"]))
    alpha = fs.challenge("alpha")
    for c in proof["h"]:
        fs.bind("zeta", bn.g1_marshal(c))
    zeta = fs.challenge("zeta")
    vals = proof["batched"]["values"]
    folded_h_zeta, lin_zeta, l, r, o, s1, s2 = vals[:7]
    qcp_z = vals[7:]
    zw = proof["z_shifted"]["value"]
    sc, l1, b_ = gm._lin_scalars(l, r, o, s1, s2, zw, n, zeta, alpha, beta, gamma, k1, k2)
    zh = (pow(zeta, n, R) - 1) % R
    lagrange = lambda i: pow(w, i, R) * zh % R * pow(n * (zeta - pow(w, i, R)) % R, R - 2, R) % R
    pi = 0
    for i, x in enumerate(public):
        pi = (pi + int(x) * lagrange(i)) % R
    for j in range(k):
        pi = (pi + gm.hash_to_field(bn.g1_marshal(proof["bsb22"][j])) * lagrange(vk["commit_rows"][j])) % R
    t = {"gamma": gamma, "beta": beta, "alpha": alpha, "zeta": zeta, "sc": sc, "pi": pi, "zn2": pow(zeta, n + 2, R), "relation": True}
    if (lin_zeta + pi - alpha * b_ % R * (o + gamma) % R * zw - alpha * alpha % R * l1) % R != folded_h_zeta * zh % R:
        return dict(t, relation=False)
    pts = {"qm": vk["qm"], "ql": vk["ql"], "qr": vk["qr"], "qo": vk["qo"], "qk": vk["qk"], "z": proof["z"], "s3": vk["s3"]}
    names = list(sc)
    lin_digest = bn.msm_g1([sc[x] for x in names] + qcp_z, [pts[x] for x in names] + proof["bsb22"])
    zn2 = pow(zeta, n + 2, R)
    folded_h_digest = bn.g1_add(bn.g1_add(proof["h"][0], bn.g1_mul(zn2, proof["h"][1])), bn.g1_mul(zn2 * zn2 % R, proof["h"][2]))
    digests = [folded_h_digest, lin_digest] + proof["lro"] + [vk["s1"], vk["s2"]] + vk["qcp"]
    gp = gm._batch_gamma(zeta, digests, vals)
    d_f, v_f, g = None, 0, 1
    for d, v in zip(digests, vals):
        d_f, v_f = bn.g1_add(d_f, bn.g1_mul(g, d)), (v_f + g * v) % R
        g = g * gp % R
    return dict(t, folded_h_digest=folded_h_digest, lin_digest=lin_digest, gp=gp, d_f=d_f, v_f=v_f)


def verify(data, vk, n, k1, k2, public=(), g2=None, g2_tau=None):
    """vk: the eight commitments by name, "qcp": the list of [Qcp_j], "commit_rows": the rows i_j (gnark_bsb22_model.verifying_key);
    g2, g2_tau: [1]_2 and [tau]_2 as bn254_py G2 points"""
    k = len(vk["qcp"])
    bad = malformed_index(data, k)
    if bad is not None:
        return False, MALFORMED, bad
    proof = gm.proof_from_bytes(data)   # raises on what the walk above let through: there is nothing of that kind
    t = derive(proof, vk, n, k1, k2, public)
    if not t["relation"]:
        return False, ALGEBRAIC, 0
    zeta, zw, w = t["zeta"], proof["z_shifted"]["value"], bn.root_of_unity(n.bit_length() - 1)
    d_f, v_f = t["d_f"], t["v_f"]
    if not opening_holds(d_f, v_f, zeta, proof["batched"]["h"], g2, g2_tau):
        return False, PAIRING, 0
    if not opening_holds(proof["z"], zw, zeta * w % R, proof["z_shifted"]["h"], g2, g2_tau):
        return False, PAIRING, 0
    return True, ACCEPT, 0


def g2_pair(tau):
    """([1]_2, [tau]_2) of a test SRS"""
    return bn.G2, bn.g2_mul(tau % R, bn.G2)


if __name__ == "__main__":
    import random
    import time
    rng = random.Random(1)
    for k in (0, 1, 2):
        inst = gm.Instance(4, k, rng, n_pi=2)
        tau = rng.randrange(1, R)
        srs = bn.kzg_srs(tau, inst.n + 3)
        _, data = gm.prove(inst, srs, [rng.randrange(R) for _ in range(9)], [rng.randrange(R) for _ in range(2 * k)], tau=tau)
        t0 = time.time()
        print("k = %d: %d bytes, verifier %s (%.1f s)" % (k, len(data), verify(data, gm.verifying_key(inst, srs, tau), inst.n, inst.k1, inst.k2,
                                                                            inst.public_inputs, *g2_pair(tau)), time.time() - t0))
