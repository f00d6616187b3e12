#!/usr/bin/env python3
"""Groth16 over BN254 in gnark's shape, on big integers: an R1CS instance generator, setup from a trapdoor in gnark's
ProvingKey layout, a model prover that returns the proof's three points and its Proof.WriteTo bytes, a parser and a trapdoor
verifier (the pairing equation checked in the exponent).  Test infrastructure, in the manner of tools/gnark_bsb22_model.py;
field, G1, G2, NTT and the quotient h come from the frozen oracle/bn254_py.py.

Status of every rule: RECALLED from gnark v0.9 backend/groth16/bn254 (setup.go, prove.go, marshal.go) and gnark-crypto
(ecc/bn254 marshal.go), UNPINNED - there is no Go source and no gnark-produced vector to compare with.
Each rule is written once, here.

  rule 1  wires      ONE (wire 0, value 1), public, secret, internal; n_public counts the constant wire      (Instance)
  rule 2  domain     the next power of two >= n_constraints; a = A w, b = B w, c = C w zero-padded to it     (Instance.abc)
  rule 3  key        A_i(tau), B_i(tau), C_i(tau) = sum_rows M[row][i] L_row(tau); G1.A / G1.B / G2.B = [A_i] [B_i]_1 [B_i]_2
                     FILTERED of the points at infinity, InfinityA / InfinityB = the masks over the wires; G1.K over the private
                     wires only = [(beta A_i + alpha B_i + C_i) / delta]; G1.Z[i] = [tau^i Z_H(tau) / delta], i < n - 1; the
                     single points [alpha]_1 [beta]_1 [delta]_1 [beta]_2 [delta]_2; the verifying key's [gamma]_2 and
                     IC_i = [(beta A_i + alpha B_i + C_i) / gamma] over the public wires                       (setup)
  rule 4  quotient   h = (a b - c) / Z_H on the coset 5 H of the SAME size (bn254_py.groth16_quotient)         (prove)
  rule 5  proof      Ar = sum w_i A_i + alpha + r delta; Bs1 = sum w_i B_i + beta + s delta in G1, Bs the same in G2;
                     Krs = sum_private w_i K_i + sum_(i < n-1) h_i Z_i + s Ar + r Bs1 - r s delta                (prove)
  rule 6  bytes      Proof.WriteTo without commitments: Ar compressed (32), Bs compressed (64), Krs compressed (32), uint32 0
                     big-endian (the empty Commitments slice), a compressed point at infinity (CommitmentPok): 164 bytes
                                                                                                             (proof_bytes)
  rule 7  G2 bytes   X.A1 || X.A0 big-endian, the flag in the top two bits of the first byte as for G1 (0b10 smallest Y, 0b11
                     largest Y, 0b01 infinity); "largest" is decided on Y.A1, on Y.A0 when Y.A1 is zero          (g2_compress)
  rule 8  verifier   e(Ar, Bs) = e(alpha, beta) e(sum_public w_i IC_i, gamma) e(Krs, delta), here in the exponent with the
                     setup's trapdoor                                                                          (verify_trapdoor)
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import bn254_py as bn  # noqa: E402

R, Q = bn.R, bn.Q
COSET_SHIFT = 5


def inv(x):
    return pow(x % R, R - 2, R)


# ---- group arithmetic beyond the oracle's: fixed-base multiples of the generators (a setup is thousands of them) and a
# Jacobian G2 sum; both are checked against bn.g1_mul / bn.g2_mul in tests/test_groth16_model_cpu.py ----
def _f2_sqr(a):
    return bn.f2_mul(a, a)


def _g2_jac_dbl(p):
    x, y, z = p
    if z == (0, 0):
        return p
    a, b = _f2_sqr(x), _f2_sqr(y)
    c = _f2_sqr(b)
    t = bn.f2_sub(bn.f2_sub(_f2_sqr(bn.f2_add(x, b)), a), c)
    d = bn.f2_add(t, t)
    e = bn.f2_add(bn.f2_add(a, a), a)
    x3 = bn.f2_sub(_f2_sqr(e), bn.f2_add(d, d))
    c8 = bn.f2_mul((8, 0), c)
    yz = bn.f2_mul(y, z)
    return x3, bn.f2_sub(bn.f2_mul(e, bn.f2_sub(d, x3)), c8), bn.f2_add(yz, yz)


def _g2_jac_add_affine(p, q):
    x1, y1, z1 = p
    if z1 == (0, 0):
        return q[0], q[1], (1, 0)
    z1z1 = _f2_sqr(z1)
    u2, s2 = bn.f2_mul(q[0], z1z1), bn.f2_mul(bn.f2_mul(q[1], z1), z1z1)
    h, r = bn.f2_sub(u2, x1), bn.f2_sub(s2, y1)
    if h == (0, 0):
        return _g2_jac_dbl((q[0], q[1], (1, 0))) if r == (0, 0) else ((1, 0), (1, 0), (0, 0))
    hh = _f2_sqr(h)
    hhh, v = bn.f2_mul(h, hh), bn.f2_mul(x1, hh)
    x3 = bn.f2_sub(bn.f2_sub(_f2_sqr(r), hhh), bn.f2_add(v, v))
    return x3, bn.f2_sub(bn.f2_mul(r, bn.f2_sub(v, x3)), bn.f2_mul(y1, hhh)), bn.f2_mul(z1, h)


def _g2_jac_to_affine(p):
    if p[2] == (0, 0):
        return None
    zi = bn.f2_inv(p[2])
    zi2 = _f2_sqr(zi)
    return bn.f2_mul(p[0], zi2), bn.f2_mul(p[1], bn.f2_mul(zi2, zi))


def g2_mul(k, p):
    """k * p over G2 in Jacobian coordinates (one inversion)"""
    k %= R
    if p is None or k == 0:
        return None
    acc = ((1, 0), (1, 0), (0, 0))
    for bit in range(k.bit_length() - 1, -1, -1):
        acc = _g2_jac_dbl(acc)
        if (k >> bit) & 1:
            acc = _g2_jac_add_affine(acc, p)
    return _g2_jac_to_affine(acc)


class FixedBase:
    """k -> k * base through a table of d * 16^j * base (d < 16, j < 64): 64 mixed additions per multiple"""

    def __init__(self, base, g2=False):
        self.g2 = g2
        add = bn.g2_add if g2 else bn.g1_add
        self.table, p = [], base
        for _ in range(64):
            row, acc = [None], None
            for _ in range(15):
                acc = add(acc, p)
                row.append(acc)
            self.table.append(row)
            p = add(acc, p)

    def mul(self, k):
        k %= R
        if self.g2:
            acc = ((1, 0), (1, 0), (0, 0))
            for j in range(64):
                d = (k >> (4 * j)) & 15
                if d:
                    acc = _g2_jac_add_affine(acc, self.table[j][d])
            return _g2_jac_to_affine(acc)
        acc = (1, 1, 0)
        for j in range(64):
            d = (k >> (4 * j)) & 15
            if d:
                acc = bn._jac_add_affine(acc, self.table[j][d])
        if acc[2] == 0:
            return None
        zi = pow(acc[2], Q - 2, Q)
        return acc[0] * zi * zi % Q, acc[1] * zi * zi * zi % Q


_BASES = {}


def g1_gen_mul(k):
    if "g1" not in _BASES:
        _BASES["g1"] = FixedBase(bn.G1)
    return _BASES["g1"].mul(k)


def g2_gen_mul(k):
    if "g2" not in _BASES:
        _BASES["g2"] = FixedBase(bn.G2, g2=True)
    return _BASES["g2"].mul(k)


def msm_g2(scalars, points):
    acc = None
    for k, p in zip(scalars, points):
        acc = bn.g2_add(acc, g2_mul(int(k), p))
    return acc


# ---- rules 1 and 2: an instance ----
class Instance:
    """A random satisfiable R1CS over Fr.  Matrices A, B, C in CSR: row_ptr, wire, coeff_id into ONE coefficient table.

    A constraint is one of
      defining  A and B are combinations of wires that exist already, C = (a combination of such wires) + k * (a NEW internal
                wire), whose value is solved for: (a b - the combination) / k
      idle      one of A, B is empty (its value is 0) and so is C: the other side may hold anything - an EMPTY row on one side,
                and the place for a row that touches EVERY wire.
    shape options (all default off / small):
      long_rows     that many defining constraints carry a row of `long_len` terms (several hundred), cycling through A, B, C
      all_wires     "a" / "b": the last constraint's A (or B) row touches every wire (the other two rows are empty)
      empty_rows    that many idle constraints with all three rows empty are spread among the others
      absent_a / absent_b   fractions of the free wires that are kept out of every row of A / of B (all_wires overrides it for
                            its one row: use one or the other)
      coeffs        "mixed": the table holds 1, -1 and random values; "unit": only 1 and -1; "general": neither 1 nor -1
    n_wires is a result: n_public + n_secret + the number of defining constraints."""

    def __init__(self, n_constraints, rng, n_public=1, n_secret=3, long_rows=0, long_len=300, all_wires=None, empty_rows=0,
                 absent_a=0.0, absent_b=0.0, coeffs="mixed", max_terms=3):
        assert n_public >= 1 and n_constraints >= 1
        self.n_constraints, self.n_public = n_constraints, n_public
        self.log_n = max(1, (n_constraints - 1).bit_length())
        self.n = 1 << self.log_n
        if coeffs == "unit":
            self.coeffs = [1, R - 1]
        elif coeffs == "general":
            self.coeffs = [rng.randrange(2, R - 1) for _ in range(12)]
        else:
            self.coeffs = [1, R - 1] + [rng.randrange(2, R - 1) for _ in range(10)] + [2, 0]
        nonzero = [i for i, v in enumerate(self.coeffs) if v]
        cinv = [inv(v) if v else 0 for v in self.coeffs]
        w = [1] + [rng.randrange(R) for _ in range(n_public - 1 + n_secret)]
        n_free = len(w)
        out_a = set(i for i in range(1, n_free) if rng.random() < absent_a)
        out_b = set(i for i in range(1, n_free) if rng.random() < absent_b)
        rows = {"A": [], "B": [], "C": []}
        n_idle = empty_rows + (1 if all_wires else 0)
        n_def = n_constraints - n_idle
        assert n_def >= 0 and long_rows <= n_def
        kinds = ["def"] * n_def + ["empty"] * empty_rows
        rng.shuffle(kinds)
        if all_wires:
            kinds.append("all")
        long_at = set(rng.sample([i for i, k in enumerate(kinds) if k == "def"], long_rows)) if long_rows else set()
        long_side = 0

        pools = {"a": [i for i in range(n_free) if i not in out_a], "b": [i for i in range(n_free) if i not in out_b],
                 "c": list(range(n_free))}            # the wires a row of A / B / C may pick from; internal wires join all three

        def combo(count, side):
            pool = pools[side]
            return [(pool[rng.randrange(len(pool))], nonzero[rng.randrange(len(nonzero))]) for _ in range(count)]

        def value(terms):
            return sum(self.coeffs[c] * w[i] for i, c in terms) % R

        for j, kind in enumerate(kinds):
            if kind == "empty":
                ra, rb, rc = [], [], []
            elif kind == "all":
                full = [(i, nonzero[rng.randrange(len(nonzero))]) for i in range(len(w))]
                ra, rb, rc = (full, [], []) if all_wires == "a" else ([], full, [])
            else:
                na, nb, ncc = (1 + rng.randrange(max_terms) for _ in range(3))
                if j in long_at:
                    if long_side % 3 == 0:
                        na = long_len
                    elif long_side % 3 == 1:
                        nb = long_len
                    else:
                        ncc = long_len
                    long_side += 1
                ra, rb, rc = combo(na, "a"), combo(nb, "b"), combo(ncc - 1, "c")
                k = nonzero[rng.randrange(len(nonzero))]
                new = (value(ra) * value(rb) - value(rc)) * cinv[k] % R
                rc.insert(rng.randrange(len(rc) + 1), (len(w), k))
                for pool in pools.values():
                    pool.append(len(w))
                w.append(new)
            rows["A"].append(ra)
            rows["B"].append(rb)
            rows["C"].append(rc)
        self.witness, self.n_wires = w, len(w)
        self.csr = {}
        for name in "ABC":
            row_ptr, wire, cid = [0], [], []
            for r_ in rows[name]:
                wire += [i for i, _ in r_]
                cid += [c for _, c in r_]
                row_ptr.append(len(wire))
            self.csr[name] = (row_ptr, wire, cid)
        self.rows = rows

    def matvec(self, name, witness=None):
        """M w, zero-padded to the domain (rule 2)"""
        w = self.witness if witness is None else witness
        out = [sum(self.coeffs[c] * w[i] for i, c in r_) % R for r_ in self.rows[name]]
        return out + [0] * (self.n - len(out))

    def abc(self, witness=None):
        return self.matvec("A", witness), self.matvec("B", witness), self.matvec("C", witness)

    def satisfied(self, witness=None):
        a, b, c = self.abc(witness)
        return all(x * y % R == z for x, y, z in zip(a, b, c))

    def unsatisfied_witness(self):
        """one entry changed: the last internal wire, which a C row carries with a non-zero coefficient"""
        w = list(self.witness)
        assert self.n_wires > self.n_public
        w[-1] = (w[-1] + 1) % R
        return w

    def occurs(self, name):
        seen = [False] * self.n_wires
        for i in self.csr[name][1]:
            seen[i] = True
        return seen


# ---- rule 3: setup ----
def lagrange_at(log_n, tau):
    """L_j(tau) for j < n over H = <w_n>: w^j Z_H(tau) / (n (tau - w^j))"""
    n = 1 << log_n
    w = bn.root_of_unity(log_n)
    zh = (pow(tau, n, R) - 1) % R
    out, x = [], 1
    for _ in range(n):
        out.append(x * zh % R * inv(n * (tau - x)) % R)
        x = x * w % R
    return out


class Trapdoor:
    def __init__(self, tau, alpha, beta, gamma, delta):
        self.tau, self.alpha, self.beta, self.gamma, self.delta = (int(v) % R for v in (tau, alpha, beta, gamma, delta))

    @classmethod
    def random(cls, rng):
        return cls(*(rng.randrange(2, R) for _ in range(5)))


def wire_polys_at(inst, tau):
    """(A_i(tau), B_i(tau), C_i(tau)) for every wire"""
    lag = lagrange_at(inst.log_n, tau)
    out = {}
    for name in "ABC":
        v = [0] * inst.n_wires
        for row, terms in enumerate(inst.rows[name]):
            for i, c in terms:
                v[i] = (v[i] + inst.coeffs[c] * lag[row]) % R
        out[name] = v
    return out["A"], out["B"], out["C"]


def setup(inst, td):
    """gnark's ProvingKey (dict "pk") and what the verifier needs of the VerifyingKey (dict "vk"), as points"""
    n = inst.n
    at, bt, ct = wire_polys_at(inst, td.tau)
    zh = (pow(td.tau, n, R) - 1) % R
    dinv, ginv = inv(td.delta), inv(td.gamma)
    k_all = [(td.beta * at[i] + td.alpha * bt[i] + ct[i]) % R for i in range(inst.n_wires)]
    a_pts = [g1_gen_mul(x) for x in at]
    b_pts = [g1_gen_mul(x) for x in bt]
    b2_pts = [g2_gen_mul(x) for x in bt]
    pk = {
        "log_n": inst.log_n, "n_wires": inst.n_wires, "n_public": inst.n_public, "n_constraints": inst.n_constraints,
        "infinity_a": [p is None for p in a_pts], "infinity_b": [p is None for p in b_pts],
        "g1_a": [p for p in a_pts if p is not None], "g1_b": [p for p in b_pts if p is not None],
        "g2_b": [p for p in b2_pts if p is not None],
        "g1_k": [g1_gen_mul(k_all[i] * dinv) for i in range(inst.n_public, inst.n_wires)],
        "g1_z": [g1_gen_mul(pow(td.tau, i, R) * zh % R * dinv) for i in range(n - 1)],
        "g1_alpha": g1_gen_mul(td.alpha), "g1_beta": g1_gen_mul(td.beta), "g1_delta": g1_gen_mul(td.delta),
        "g2_beta": g2_gen_mul(td.beta), "g2_delta": g2_gen_mul(td.delta),
    }
    vk = {"g2_gamma": g2_gen_mul(td.gamma), "ic": [g1_gen_mul(k_all[i] * ginv) for i in range(inst.n_public)]}
    return pk, vk


# ---- rules 4 and 5: the prover ----
def prove(inst, pk, witness, r, s, h=None):
    """(Ar, Bs, Krs) as affine points from the key's POINTS (an honest prover's sums).  h: override the quotient (tests)."""
    assert witness[0] == 1 and len(witness) == inst.n_wires
    a, b, c = inst.abc(witness)
    if h is None:
        h = bn.groth16_quotient(a, b, c, COSET_SHIFT)
    wa = [witness[i] for i in range(inst.n_wires) if not pk["infinity_a"][i]]
    wb = [witness[i] for i in range(inst.n_wires) if not pk["infinity_b"][i]]
    ar = bn.g1_add(bn.g1_add(bn.msm_g1(wa, pk["g1_a"]), pk["g1_alpha"]), bn.g1_mul(r, pk["g1_delta"]))
    bs1 = bn.g1_add(bn.g1_add(bn.msm_g1(wb, pk["g1_b"]), pk["g1_beta"]), bn.g1_mul(s, pk["g1_delta"]))
    bs = bn.g2_add(bn.g2_add(msm_g2(wb, pk["g2_b"]), pk["g2_beta"]), g2_mul(s, pk["g2_delta"]))
    krs = bn.g1_add(bn.msm_g1(witness[inst.n_public:], pk["g1_k"]), bn.msm_g1(h[:inst.n - 1], pk["g1_z"]))
    krs = bn.g1_add(krs, bn.g1_mul(s, ar))
    krs = bn.g1_add(krs, bn.g1_mul(r, bs1))
    krs = bn.g1_add(krs, bn.g1_neg(bn.g1_mul(r * s % R, pk["g1_delta"])))
    return ar, bs, krs


def proof_logs(inst, td, witness, r, s, h=None):
    """the discrete logs (a, b, c) of an honest proof's Ar, Bs, Krs - what the points must be multiples of the generators by.
    With the true quotient sum_(i < n-1) h_i tau^i Z_H(tau) = A(tau) B(tau) - C(tau) (h's top coefficient is zero)."""
    at, bt, ct = wire_polys_at(inst, td.tau)
    A = sum(w * x for w, x in zip(witness, at)) % R
    B = sum(w * x for w, x in zip(witness, bt)) % R
    C = sum(w * x for w, x in zip(witness, ct)) % R
    a = (A + td.alpha + r * td.delta) % R
    b = (B + td.beta + s * td.delta) % R
    if h is None:
        hz = (A * B - C) % R
    else:
        hz = bn.eval_poly(h[:inst.n - 1], td.tau) * (pow(td.tau, inst.n, R) - 1) % R
    priv = sum(witness[i] * (td.beta * at[i] + td.alpha * bt[i] + ct[i]) for i in range(inst.n_public, inst.n_wires)) % R
    c = ((priv + hz) * inv(td.delta) + s * a + r * b - r * s % R * td.delta) % R
    return a, b, c


def prove_by_logs(inst, td, witness, r, s):
    """the same three points as prove(), from the trapdoor: three fixed-base multiples (what makes 2^10 constraints cheap)"""
    a, b, c = proof_logs(inst, td, witness, r, s)
    return g1_gen_mul(a), g2_gen_mul(b), g1_gen_mul(c)


# ---- rules 6 and 7: bytes ----
def _lex_largest_fq(y):
    return int(y) > (Q - 1) // 2


def g2_y_is_largest(y):
    return _lex_largest_fq(y[0]) if y[1] == 0 else _lex_largest_fq(y[1])


def g2_compress(p):
    """G2Affine.Bytes(): 64 bytes"""
    if p is None:
        return bytes([0x40]) + bytes(63)
    b = bytearray(int(p[0][1]).to_bytes(32, "big") + int(p[0][0]).to_bytes(32, "big"))
    b[0] |= 0xC0 if g2_y_is_largest(p[1]) else 0x80
    return bytes(b)


def fq_sqrt(a):
    a %= Q
    y = pow(a, (Q + 1) // 4, Q)          # q = 3 mod 4
    return y if y * y % Q == a else None


def f2_sqrt(a):
    """a square root in Fq2 = Fq[u] / (u^2 + 1), or None (the complex method: norm, then two square roots in Fq)"""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        y = fq_sqrt(a0)
        if y is not None:
            return (y, 0)
        y = fq_sqrt(-a0)                  # -1 is not a square: exactly one of a0, -a0 is
        return (0, y)
    s = fq_sqrt(a0 * a0 + a1 * a1)
    if s is None:
        return None
    half = pow(2, Q - 2, Q)
    x0 = fq_sqrt((a0 + s) * half)
    if x0 is None:
        x0 = fq_sqrt((a0 - s) * half)
    if x0 is None or x0 == 0:
        return None
    y = (x0, a1 * pow(2 * x0, Q - 2, Q) % Q)
    return y if bn.f2_mul(y, y) == (a0, a1) else None


def g2_decompress(data):
    assert len(data) == 64
    flag = data[0] >> 6
    if flag == 1:
        assert not any(data[1:]) and data[0] == 0x40
        return None
    assert flag in (2, 3), "not a compressed point"
    x = (int.from_bytes(data[32:], "big"), int.from_bytes(bytes([data[0] & 0x3F]) + data[1:32], "big"))
    assert x[0] < Q and x[1] < Q
    y = f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.B2))
    assert y is not None, "not on the curve"
    if g2_y_is_largest(y) != (flag == 3):
        y = ((-y[0]) % Q, (-y[1]) % Q)
    return x, y


PROOF_BYTES = 164


def proof_bytes(ar, bs, krs):
    """Proof.WriteTo with no commitments"""
    return bn.g1_compress(ar) + g2_compress(bs) + bn.g1_compress(krs) + (0).to_bytes(4, "big") + bn.g1_compress(None)


def proof_from_bytes(data):
    assert len(data) == PROOF_BYTES
    assert int.from_bytes(data[128:132], "big") == 0, "commitments are not supported"
    assert bn.g1_decompress(data[132:164]) is None and not any(data[133:164])
    return bn.g1_decompress(data[0:32]), g2_decompress(data[32:96]), bn.g1_decompress(data[96:128])


# ---- rule 8: the verifier, in the exponent ----
def verify_trapdoor(data, inst, td, witness, r, s, public=None):
    """The verifier's check on the proof BYTES with the setup's trapdoor in place of the pairing.  The test recovers the witness
    and r, s (a verifier proper knows neither: they only serve to find the points' discrete logs); `public`: the public inputs
    the verifier holds (wires 1 .. n_public - 1), by default the witness's own."""
    try:
        ar, bs, krs = proof_from_bytes(data)
    except (AssertionError, ValueError):
        return False
    w = list(witness)
    if public is not None:
        assert len(public) == inst.n_public - 1
        w[1:inst.n_public] = [int(x) % R for x in public]
    a, b, c = proof_logs(inst, td, w, r, s)
    if ar != g1_gen_mul(a) or bs != g2_gen_mul(b) or krs != g1_gen_mul(c):
        return False
    at, bt, ct = wire_polys_at(inst, td.tau)
    ic = sum(w[i] * (td.beta * at[i] + td.alpha * bt[i] + ct[i]) % R * inv(td.gamma) for i in range(inst.n_public)) % R
    return a * b % R == (td.alpha * td.beta + ic * td.gamma + c * td.delta) % R


# ---- shapes the tests walk through ----
SHAPES = {
    "common": {},
    "public3": {"n_public": 3},
    "long": {"long_rows": 3, "long_len": 300},
    "all_a": {"all_wires": "a"},
    "all_b": {"all_wires": "b", "n_public": 3},
    "empty": {"empty_rows": 2},
    "absent": {"absent_a": 0.5, "absent_b": 0.5, "n_secret": 8},
    "unit": {"coeffs": "unit"},
    "general": {"coeffs": "general"},
}


if __name__ == "__main__":
    import random
    rng = random.Random(16)
    for name, kw in SHAPES.items():
        inst = Instance(11 if name != "long" else 13, rng, **kw)
        td = Trapdoor.random(rng)
        pk, vk = setup(inst, td)
        r, s = rng.randrange(R), rng.randrange(R)
        pts = prove(inst, pk, inst.witness, r, s)
        assert pts == prove_by_logs(inst, td, inst.witness, r, s)
        data = proof_bytes(*pts)
        assert verify_trapdoor(data, inst, td, inst.witness, r, s)
        print("%-8s %d constraints, %d wires: %d-byte proof verifies" % (name, inst.n_constraints, inst.n_wires, len(data)))
