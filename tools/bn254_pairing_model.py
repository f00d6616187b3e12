#!/usr/bin/env python3
"""The optimal ate pairing on BN254 the slow textbook way, on big integers: what the device's pairing
(csrc/bn254_pairing.hpp) is compared with.  Test infrastructure, in the manner of tools/groth16_model.py; Fq, Fq2 and the two
groups come from the frozen oracle/bn254_py.py.  It shares no formula with the device code:

  Fq12     ONE polynomial ring Fq[w] / (w^12 - 18 w^6 + 82) (w^6 = 9 + u and u^2 = -1), twelve coefficients, schoolbook
           product, inverse by the extended Euclidean algorithm on polynomials - no tower, no Karatsuba, no Frobenius constants
  Q        untwisted into E(Fq12): (x', y') -> (x' w^2, y' w^3), from y^2 = x^3 + 3 / (9 + u) onto y^2 = x^3 + 3
  Miller   f_(6x+2, Q)(P) by affine chord-and-tangent lines in E(Fq12), then the two lines through pi(Q) and -pi^2(Q), pi the
           q-power map computed as a pow
  final    ONE pow by HARD_MULTIPLE (q^12 - 1) / r

HARD_MULTIPLE: the device's hard part is the addition chain of Scott, Benger, Charlemagne, Dominguez Perez and Kachisa ("On the
final exponentiation for calculating pairings on ordinary elliptic curves", the chain with y0 .. y6), which for this curve
raises to exactly (q^4 - q^2 + 1) / r: the multiple is 1.  hard_chain_multiple() recomputes it from the chain written as
integers mod q^4 - q^2 + 1 (Frobenius = times q, conjugate = times -1, the x-power = times x), and the CPU test holds the
two together.
"""
import os
import sys
from math import gcd

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
sys.path.insert(0, _HERE)
import bn254_py as bn  # noqa: E402

Q, R = bn.Q, bn.R
X = 4965661367192848881
ATE_LOOP = 6 * X + 2
assert Q == 36 * X**4 + 36 * X**3 + 24 * X**2 + 6 * X + 1 and R == 36 * X**4 + 36 * X**3 + 18 * X**2 + 6 * X + 1
HARD_MULTIPLE = 1
assert gcd(HARD_MULTIPLE, R) == 1
FINAL_EXPONENT = HARD_MULTIPLE * ((Q**12 - 1) // R)

# ---- Fq12 = Fq[w] / (w^12 - 18 w^6 + 82): a tuple of twelve integers, the coefficient of w^i at i ----
F12_ONE = (1,) + (0,) * 11
F12_ZERO = (0,) * 12


def f12_add(a, b):
    return tuple((x + y) % Q for x, y in zip(a, b))


def f12_sub(a, b):
    return tuple((x - y) % Q for x, y in zip(a, b))


def f12_neg(a):
    return tuple(-x % Q for x in a)


def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):        # w^k = 18 w^(k-6) - 82 w^(k-12)
        c = t[k]
        t[k - 6] += 18 * c
        t[k - 12] -= 82 * c
    return tuple(x % Q for x in t[:12])


def f12_pow(a, e):
    assert e >= 0
    out = F12_ONE
    for bit in bin(e)[2:]:
        out = f12_mul(out, out)
        if bit == "1":
            out = f12_mul(out, a)
    return out


def _poly_trim(p):
    while p and p[-1] == 0:
        p.pop()
    return p


def _poly_divmod(a, b):
    a, out = list(a), [0] * max(1, len(a) - len(b) + 1)
    binv = pow(b[-1], Q - 2, Q)
    while len(a) >= len(b):
        c, s = a[-1] * binv % Q, len(a) - len(b)
        out[s] = c
        for i, y in enumerate(b):
            a[s + i] = (a[s + i] - c * y) % Q
        a.pop()
        _poly_trim(a)
    return _poly_trim(out), a


def f12_inv(a):
    """extended Euclid on (the modulus, a): s a = gcd (a constant)"""
    r0, r1 = [82, 0, 0, 0, 0, 0, Q - 18, 0, 0, 0, 0, 0, 1], _poly_trim(list(a))
    assert r1, "0 has no inverse"
    s0, s1 = [], [1]
    while len(r1) > 1:
        qt, rem = _poly_divmod(r0, r1)
        prod = [0] * (len(qt) + len(s1))
        for i, x in enumerate(qt):
            for j, y in enumerate(s1):
                prod[i + j] = (prod[i + j] + x * y) % Q
        s2 = [(x - y) % Q for x, y in zip(s0 + [0] * (len(prod) - len(s0)), prod + [0] * (len(s0) - len(prod)))]
        r0, r1, s0, s1 = r1, rem, s1, _poly_trim(s2)
        assert r1, "not invertible"
    c = pow(r1[0], Q - 2, Q)
    out = [x * c % Q for x in s1]
    return tuple(out + [0] * (12 - len(out)))


def f12_from_fq(x):
    return (x % Q,) + (0,) * 11


def f12_from_f2(a, shift=0):
    """(a0 + a1 u) w^shift with u = w^6 - 9, shift < 6"""
    out = [0] * 12
    out[shift] = (a[0] - 9 * a[1]) % Q
    out[shift + 6] = a[1] % Q
    return tuple(out)


# ---- E(Fq12): y^2 = x^3 + 3, affine, None = the point at infinity ----
def untwist(q2):
    return None if q2 is None else (f12_from_f2(q2[0], 2), f12_from_f2(q2[1], 3))


def _line_and_sum(t, s, p):
    """the line through t and s (the tangent where t = s) at p = (xP, yP) in Fq, and t + s"""
    xp, yp = f12_from_fq(p[0]), f12_from_fq(p[1])
    if t[0] == s[0] and t[1] != s[1]:
        return f12_sub(xp, t[0]), None                  # the vertical line
    if t == s:
        lam = f12_mul(f12_mul(f12_from_fq(3), f12_mul(t[0], t[0])), f12_inv(f12_add(t[1], t[1])))
    else:
        lam = f12_mul(f12_sub(s[1], t[1]), f12_inv(f12_sub(s[0], t[0])))
    line = f12_sub(f12_sub(yp, t[1]), f12_mul(lam, f12_sub(xp, t[0])))
    x3 = f12_sub(f12_sub(f12_mul(lam, lam), t[0]), s[0])
    return line, (x3, f12_sub(f12_mul(lam, f12_sub(t[0], x3)), t[1]))


def _frobenius_point(t):
    return f12_pow(t[0], Q), f12_pow(t[1], Q)


def miller_loop(p, q2):
    """f_(6x+2, Q)(P) l_(T, pi Q)(P) l_(T + pi Q, -pi^2 Q)(P); 1 if either point is the point at infinity"""
    if p is None or q2 is None:
        return F12_ONE
    qq = untwist(q2)
    f, t = F12_ONE, qq
    for bit in bin(ATE_LOOP)[3:]:
        line, t = _line_and_sum(t, t, p)
        f = f12_mul(f12_mul(f, f), line)
        if bit == "1":
            line, t = _line_and_sum(t, qq, p)
            f = f12_mul(f, line)
    q1 = _frobenius_point(qq)
    q2m = _frobenius_point(q1)
    q2m = (q2m[0], f12_neg(q2m[1]))
    line, t = _line_and_sum(t, q1, p)
    f = f12_mul(f, line)
    line, t = _line_and_sum(t, q2m, p)
    return f12_mul(f, line)


def final_exponentiation(f):
    return f12_pow(f, FINAL_EXPONENT)


def pairing(p, q2):
    return final_exponentiation(miller_loop(p, q2))


def pairing_product(pairs):
    f = F12_ONE
    for p, q2 in pairs:
        f = f12_mul(f, miller_loop(p, q2))
    return final_exponentiation(f)


def hard_chain_multiple():
    """The exponent the device's hard-part chain raises to, as a multiple of (q^4 - q^2 + 1) / r, mod r."""
    phi = Q**4 - Q**2 + 1
    f = 1
    fp, fp2 = f * Q, f * Q**2
    fp3 = fp2 * Q
    fu = f * X
    fu2 = fu * X
    fu3 = fu2 * X
    y3 = -(fu * Q)
    fu2p, fu3p = fu2 * Q, fu3 * Q
    y2 = fu2 * Q**2
    y0 = fp + fp2 + fp3
    y1 = -f
    y5 = -fu2
    y4 = -(fu + fu2p)
    y6 = -(fu3 + fu3p)
    t0 = 2 * y6 + y4 + y5
    t1 = y3 + y5 + t0
    t0 = t0 + y2
    t1 = 2 * (2 * t1 + t0)
    t0 = t1 + y1
    t1 = t1 + y0
    e = (2 * t0 + t1) % phi
    assert e % (phi // R) == 0
    return e // (phi // R) % R


# ---- the order in which the device writes an element: gnark-crypto's E12 (C0.B0.A0, C0.B0.A1, C0.B1.A0, ... C1.B2.A1), with
# C_c.B_b = the Fq2 coefficient of w^(2 b + c) ----
def f12_to_gnark(a):
    """twelve integers in E12 order"""
    out = []
    for c in range(2):
        for b in range(3):
            k = 2 * b + c
            a1 = a[k + 6]
            out += [(a[k] + 9 * a1) % Q, a1]
    return out


def f12_from_gnark(v):
    out = [0] * 12
    i = 0
    for c in range(2):
        for b in range(3):
            k = 2 * b + c
            a0, a1 = v[i], v[i + 1]
            i += 2
            out[k] = (a0 - 9 * a1) % Q
            out[k + 6] = a1 % Q
    return tuple(out)


# ---- the G2 subgroup test, the plain one ----
def g2_on_curve(q2):
    if q2 is None:
        return True
    x, y = q2
    return bn.f2_mul(y, y) == bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.B2)


def _g2_mul_any(k, p):
    """k p for a twist point of ANY order (bn.g2_mul reduces k mod r)"""
    acc = None
    for bit in bin(k)[2:]:
        acc = bn.g2_add(acc, acc)
        if bit == "1":
            acc = bn.g2_add(acc, p)
    return acc


def g2_in_subgroup(q2):
    return q2 is None or _g2_mul_any(R, q2) is None


def twist_point_outside_subgroup(rng):
    """a point of the twist that is not in the r-torsion subgroup (the twist's order is r (2 q - r))"""
    import groth16_model as gm
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = gm.f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.B2))
        if y is not None and not g2_in_subgroup((x, y)):
            return x, y


_E_ALPHA_BETA = {}


def _pairing_equation(pk, vk, ar, bs, krs, ksum):
    """e(Ar, Bs) = e(alpha, beta) e(kSum, gamma) e(Krs, delta); e(alpha, beta) is computed once per key (gnark's Precompute)"""
    key = (pk["g1_alpha"], pk["g2_beta"])
    if key not in _E_ALPHA_BETA:
        _E_ALPHA_BETA[key] = pairing(*key)
    rhs = f12_mul(_E_ALPHA_BETA[key], pairing_product([(ksum, vk["g2_gamma"]), (krs, pk["g2_delta"])]))
    return pairing(ar, bs) == rhs


# ---- Groth16's verifier with real pairings (gnark's Verify; rule 8 of tools/groth16_model.py without the trapdoor) ----
def groth16_verify(vk, pk, proof_bytes, public):
    """vk, pk: groth16_model.setup's dictionaries (alpha, beta, delta lie in pk); public: wires 1 .. n_public - 1"""
    import groth16_commit_model as cm
    try:
        ar, bs, krs, cs, _ = cm.proof_from_bytes(proof_bytes)     # the strict decoder: flag bytes, x < q, the exact length
    except (AssertionError, ValueError):
        return False
    if cs:
        return False
    if not g2_in_subgroup(bs) or len(public) != len(vk["ic"]) - 1:
        return False
    ksum = vk["ic"][0]
    for w, pt in zip(public, vk["ic"][1:]):
        ksum = bn.g1_add(ksum, bn.g1_mul(int(w) % R, pt))
    return _pairing_equation(pk, vk, ar, bs, krs, ksum)


def pedersen_vk(td):
    """The Pedersen verifying key (G, GRootSigmaNeg) of a committed setup: the pair with e(C, GRootSigmaNeg) e(Pok, G) = 1 for
    Pok = sum_i w_i BasisExpSigma_i.  tools/groth16_commit_model.py takes BasisExpSigma = sigma Basis, so the pair is
    ([1]_2, [-sigma]_2) for ITS sigma (a setup that takes BasisExpSigma = (1 / sigma') Basis gets [-1 / sigma']_2: the same key)."""
    import groth16_model as gm
    return bn.G2, gm.g2_gen_mul(-td.sigma % R)


def groth16_verify_committed(vk, pk, inst, pedersen, proof_bytes, public):
    """The same for a key with Bsb22 / Pedersen commitments (tools/groth16_commit_model.py): the commitment wires' values are
    recomputed from the bytes' C_j, the Pedersen check e(sum_j rho^j C_j, GRootSigmaNeg) e(Pok, G) = 1 comes first, then the
    pairing equation with the commitment wires and the C_j in the public sum.  inst: only its commitments' hashed wire ids."""
    import groth16_commit_model as cm
    try:
        ar, bs, krs, cs, pok = cm.proof_from_bytes(proof_bytes)
    except (AssertionError, ValueError):
        return False
    if len(cs) != inst.k or len(public) != inst.n_public - 1 or not g2_in_subgroup(bs):
        return False
    v = {0: 1}
    v.update({i + 1: int(x) % R for i, x in enumerate(public)})
    for j, c_ in enumerate(inst.commitments):
        v[c_["wire"]] = cm.commitment_challenge(cs[j], [v[i] for i in c_["public"]])
    if inst.k:
        rho = cm.fold_challenge([v[c_["wire"]] for c_ in inst.commitments])
        folded, power = None, 1
        for c_point in cs:
            folded = bn.g1_add(folded, bn.g1_mul(power, c_point))
            power = power * rho % R
        if pairing_product([(folded, pedersen[1]), (pok, pedersen[0])]) != F12_ONE:
            return False
    ksum = None
    wires = list(range(inst.n_public)) + [c_["wire"] for c_ in inst.commitments]
    for i, pt in zip(wires, vk["ic"]):
        ksum = bn.g1_add(ksum, bn.g1_mul(v[i], pt))
    for c_point in cs:
        ksum = bn.g1_add(ksum, c_point)
    return _pairing_equation(pk, vk, ar, bs, krs, ksum)


if __name__ == "__main__":
    import time
    t0 = time.time()
    e = pairing(bn.G1, bn.G2)
    print("e(G1, G2) in %.2f s; != 1: %s; ^r = 1: %s; chain multiple %d" % (time.time() - t0, e != F12_ONE, f12_pow(e, R) == F12_ONE,
                                                                              hard_chain_multiple()))
