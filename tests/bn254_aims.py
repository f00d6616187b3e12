"""Aimed inputs for the BN254 scalar-field chain (csrc/bn254_plonk.hip, csrc/bn254.hip) and for the nine-limb field it computes
on (csrc/bn254_f29.hpp): memory words at the edges of the limbs, operands at the edges of the stated bounds, grand-product rows
whose numerator or denominator vanishes, and quotient inputs whose values at chosen points of the 4n coset are chosen.

The quotient is evaluated on shift * <w_4n>, position i = 4 k + c holding the point shift * w_4n^(4 k + c) = (shift w_4n^c) w_n^k
(class c, index k).  A polynomial of degree below n is fixed by its n values on one class, so those can be chosen: on_class()
returns the values on H of that polynomial, and the prover then reads exactly the chosen values at positions 4 k + c.  z(w x) of
position 4 k + c is position 4 (k + 1) + c, wrapping at k = n - 1.

Elements rest in memory as fr.Element words (Montgomery, 2^256): the limbs see the WORD, so an aim is stated as a word and the
field value the models compute with is from_montgomery(word).

A plain module (not a conftest): the CPU tests check the construction, the GPU tests use it.  The reference is always Python
integers (oracle/bn254_py.py and the functions below)."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_py as bn  # noqa: E402
import gnark_bsb22_model as gm  # noqa: E402

R, Q = bn.R, bn.Q
RP = 1 << 261                      # the Montgomery radix of the nine-limb form

# named 256-bit memory words below r
WORD_AIMS = [("0", 0), ("1", 1), ("r-1", R - 1), ("r-2", R - 2), ("2^253-1: every low limb all ones", (1 << 253) - 1),
             ("2^232: top limb only", 1 << 232), ("2^29-1", (1 << 29) - 1), ("2^29", 1 << 29), ("2^256 mod r", (1 << 256) % R),
             ("(r-1)/2", (R - 1) // 2)]
assert all(0 <= w < R for _, w in WORD_AIMS)
AIM_VALUES = [bn.from_montgomery(w) for _, w in WORD_AIMS]      # the field values whose words are WORD_AIMS
V_RM1 = bn.from_montgomery(R - 1)                               # the value whose word is r - 1


def aim_value(i):
    return AIM_VALUES[i % len(AIM_VALUES)]


# ---- packing without a Python loop per word ----------------------------------------------------------------------------------
def pack(ints):
    """integers below 2^256 -> (n, 4) uint64 little-endian words"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), dtype=np.uint64).reshape(-1, 4).copy()


def unpack(words):
    b = np.ascontiguousarray(words, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def pack_mont(values):
    return pack([v * bn.MONT_R % R for v in values])


_MONT_INV = pow(bn.MONT_R, R - 2, R)


def unpack_mont(words):
    return [x * _MONT_INV % R for x in unpack(words)]


# ---- bn254_f29.hpp: operands for the host check (tests/native/bn254_f29_check.cpp) and the device check (nlx_bn254_f29_ops) ----
def f29_cases(rng):
    """(modulus name, op, a, b): random operands and the extremes of the ranges the header allows, for both moduli; x32 (the
    prover's way back to memory form after a product of two data values) for r"""
    cases = []
    for name, q in (("q", Q), ("r", R)):
        tight = lambda: rng.randrange(1 << 255)                              # noqa: E731
        mul_in = lambda: rng.choice([rng.randrange(int(2 ** 257.5)), int(2 ** 257.5) - 1, 0, 1, q, q - 1, 2 * q])   # noqa: E731,B023
        for _ in range(200):
            cases.append((name, "mul", mul_in(), mul_in()))
            cases.append((name, "add", rng.randrange(1 << 257), rng.randrange(1 << 257)))
            cases.append((name, "sub4", rng.randrange(1 << 257), rng.choice([tight(), (1 << 255) - 1, 0])))
            cases.append((name, "sub8", rng.randrange(1 << 257), rng.choice([rng.randrange(3 << 255), (3 << 255) - 1, 0])))
            cases.append((name, "tighten", rng.choice([rng.randrange(1 << 258), (1 << 258) - 1, 0, q, 21 * q, q - 1, 7 * q + 5]), 0))
            cases.append((name, "canonical", rng.choice([rng.randrange(1 << 258), (1 << 258) - 1, 0, q, 21 * q, q - 1, 7 * q + 5, 2 * q - 1]), 0))
            cases.append((name, "iszero", rng.choice([rng.randrange(1 << 258), 0, q, 5 * q, 21 * q, q + 1, 13 * q - 1]), 0))
            cases.append((name, "frommont", rng.choice([rng.randrange(q), 0, q - 1, (1 << 256) % q]), 0))
            cases.append((name, "words", rng.choice([rng.randrange(1 << 256), (1 << 256) - 1, 0]), 0))
            cases.append((name, "tocanon", rng.choice([tight(), 0, q, 2 * q, RP % q]), 0))
    # the kernels hand x32 products (< 2^255) and memory words (< 2^256); its own bound is tighten's 2^258, and only above 2^256
    # does its first tighten matter
    for a in [0, R - 1, R, 11 * R // 10] + [rng.randrange(1 << 255) for _ in range(60)] + \
            [(1 << 256) - 1, (1 << 258) - 1] + [rng.randrange(1 << 256, 1 << 258) for _ in range(30)]:
        cases.append(("r", "x32", a, 0))
    return cases


def f29_check(case, got, normalised):
    """what both checks assert of one case's result: its value and bound as Python integers, and that limbs 0 .. 7 are below 2^29"""
    name, op, a, b = case
    q = Q if name == "q" else R
    assert normalised == 1, (op, a, b)
    if op == "mul":
        assert got % q == a * b * pow(RP, -1, q) % q and got < (1 << 254) + q, (op, hex(a), hex(b))
    elif op == "add":
        assert got == a + b
    elif op == "sub4":
        assert got == a + 4 * q - b
    elif op == "sub8":
        assert got == a + 8 * q - b
    elif op == "tighten":
        assert got % q == a % q and got < 1.1 * q
    elif op == "canonical":
        assert got == a % q
    elif op == "iszero":
        assert got == (1 if a % q == 0 else 0)
    elif op == "frommont":
        assert got % q == a * 32 % q and got < (1 << 255)            # x 2^256 -> x 2^261
    elif op == "words":
        assert got == a
    elif op == "tocanon":
        assert got == a * pow(RP, -1, q) % q
    elif op == "x32":
        assert got % q == 32 * a % q and got < 1.1 * q, (op, hex(a))
    else:
        raise AssertionError("unknown op %s" % op)


def to_limbs(x):
    """an integer below 2^261 + ... as nine 29-bit limbs, limb 8 taking what is left"""
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


def from_limbs(limbs):
    """(value, limbs 0 .. 7 are below 2^29)"""
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs)), int(all(int(v) < (1 << 29) for v in limbs[:8]))


# ---- the grand product ------------------------------------------------------------------------------------------------------------
def gp_factors(p, i, x, beta, gamma, k1, k2):
    """(numerator, denominator) of row i, x = w^i"""
    num = (p["l"][i] + beta * x + gamma) * (p["r"][i] + beta * k1 * x + gamma) * (p["o"][i] + beta * k2 * x + gamma) % R
    den = (p["l"][i] + beta * p["s1"][i] + gamma) * (p["r"][i] + beta * p["s2"][i] + gamma) * (p["o"][i] + beta * p["s3"][i] + gamma) % R
    return num, den


def grand_product_model(p, beta, gamma, k1, k2):
    """the row formula z_0 = 1, z_{i+1} = z_i num_i / den_i with 1 / 0 := 0 (gnark's BatchInvert; pow(0, r - 2, r) = 0) ->
    (z, closes): closes = the product returns to 1 after the last row"""
    n = len(p["l"])
    w = bn.root_of_unity(n.bit_length() - 1)
    z, acc, x = [], 1, 1
    for i in range(n):
        z.append(acc)
        num, den = gp_factors(p, i, x, beta, gamma, k1, k2)
        acc = acc * num % R * (pow(den, -1, R) if den else 0) % R
        x = x * w % R
    return z, acc == 1


def gp_zero_cases(p, beta, gamma, k1, k2):
    """(name, witness, rows whose denominator is 0, rows whose numerator is 0) from a satisfying witness p of n >= 128 rows: one
    wire of each named row replaced so that a factor vanishes (a wire the permutation moves, so that the other side's factor
    does not vanish with it; for "both", a second wire for the numerator).  `base` is the first row of a run of 64 that is not the first
    run (and, from 2^13 rows on, lies in the second block of 64 runs)"""
    n = len(p["l"])
    w = bn.root_of_unity(n.bit_length() - 1)
    base = n // 2 + (320 if n >= 8192 else 0)
    assert base % 64 == 0 and 64 <= base and base + 64 <= n

    cols = (("l", "s1", 1), ("r", "s2", k1), ("o", "s3", k2))

    def moved(i):
        """the wires of row i that the permutation does not leave in place: there a zero denominator factor is no zero numerator factor"""
        x = pow(w, i, R)
        return [c for c in cols if p[c[1]][i] != c[2] * x % R]

    def with_rows(den_rows=(), num_rows=(), both_rows=()):
        q = dict(p, l=list(p["l"]), r=list(p["r"]), o=list(p["o"]))
        for i in list(den_rows) + list(both_rows):
            wire, sigma, _ = moved(i)[0]
            q[wire][i] = -(beta * p[sigma][i] + gamma) % R
        for i in list(num_rows) + list(both_rows):         # both: another wire than the denominator's
            wire, _, k = moved(i)[0] if i in num_rows else [c for c in cols if c != moved(i)[0]][0]
            q[wire][i] = -(beta * k * pow(w, i, R) + gamma) % R
        return q, sorted(set(den_rows) | set(both_rows)), sorted(set(num_rows) | set(both_rows))
    named = [("first row of a run", dict(den_rows=[base])), ("a middle row of a run", dict(den_rows=[base + 6])),
             ("last row of a run", dict(den_rows=[base + 63])), ("row 0", dict(den_rows=[0])),
             ("row n - 1: the ratio that goes to `last`", dict(den_rows=[n - 1])),
             ("two zeros in one run", dict(den_rows=[base + 3, base + 40])),
             ("zeros in two runs", dict(den_rows=[base - 64 + 10, base + 20])),
             ("a zero numerator", dict(num_rows=[base + 5])),
             ("numerator and denominator both vanish", dict(both_rows=[base + 9]))]
    return [(name,) + with_rows(**kw) for name, kw in named]


# ---- the quotient at aimed points --------------------------------------------------------------------------------------------------
def on_class(values, c, log_n, shift):
    """values[k] chosen at the points shift * w_4n^(4 k + c), k < n -> the values on H of the polynomial of degree < n that takes
    them: with g = shift w_4n^c the points are g w_n^k, so the coefficients are FFTInverse(values)_j / g^j"""
    n = 1 << log_n
    assert len(values) == n
    g = shift * pow(bn.root_of_unity(log_n + 2), c, R) % R
    ginv = pow(g, R - 2, R)
    co, s = [], 1
    for v in bn.ntt(values, inverse=True):
        co.append(v * s % R)
        s = s * ginv % R
    return bn.ntt(co)


def class_point(c, k, log_n, shift):
    return shift * pow(bn.root_of_unity(log_n + 2), 4 * k + c, R) % R


FIXED = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")
THIRTEEN = FIXED + ("l", "r", "o", "z", "pi")
GATE_TERMS = ("ql", "qr", "qm", "qo", "qk", "l", "r", "o", "pi", "qcp0", "pi20")
QUOTIENT_AIMS = ("all zero", "all words r-1", "l = -(beta x + gamma)", "l = -(beta s1 + gamma)", "f = h", "z = 1", "z = 0",
                 "f = h at k = n - 1: z(w x) wraps", "gate terms all r-1")


def quotient_aim(aim, names, c, log_n, shift, k1, k2, beta, gamma):
    """{name: the n chosen values on class c} and the aimed index k0: every position holds WORD_AIMS in rotation (polynomial j at
    index k: word (j + k) mod 10), but index k0 (and for f = h its successor in z), which holds the aim"""
    n = 1 << log_n
    assert aim in QUOTIENT_AIMS
    k0 = n - 1 if "wraps" in aim else (n // 2 + c) % (n - 1)
    rows = {name: [aim_value(j + k) for k in range(n)] for j, name in enumerate(names)}
    x = class_point(c, k0, log_n, shift)
    if aim == "all zero":
        for name in names:
            rows[name][k0] = 0
    elif aim == "all words r-1":
        for name in names:
            rows[name][k0] = V_RM1
    elif aim == "l = -(beta x + gamma)":
        rows["l"][k0] = -(beta * x + gamma) % R
    elif aim == "l = -(beta s1 + gamma)":
        rows["l"][k0] = -(beta * rows["s1"][k0] + gamma) % R
    elif aim.startswith("f = h"):
        rows["s1"][k0], rows["s2"][k0], rows["s3"][k0] = x, k1 * x % R, k2 * x % R
        rows["z"][(k0 + 1) % n] = rows["z"][k0]
    elif aim == "z = 1":
        rows["z"][k0] = 1
    elif aim == "z = 0":
        rows["z"][k0] = 0
    elif aim == "gate terms all r-1":
        for name in names:
            if name in GATE_TERMS:
                rows[name][k0] = V_RM1
    return rows, k0


def quotient_inputs(aim, variant, c, log_n, shift, k1, k2, beta, gamma):
    """the polynomials of one aimed quotient call as values on H, by name (variant: "plain", "pi", "blinded", "commit": the last
    one carries pi, qcp0 and pi20) -> (on_h, rows, k0)"""
    names = list(THIRTEEN[:12])
    if variant in ("pi", "commit"):
        names.append("pi")
    if variant == "commit":
        names += ["qcp0", "pi20"]
    rows, k0 = quotient_aim(aim, names, c, log_n, shift, k1, k2, beta, gamma)
    return {name: on_class(v, c, log_n, shift) for name, v in rows.items()}, rows, k0


def quotient_model(on_h, variant, n, shift, k1, k2, alpha, beta, gamma, blinding=None):
    """the model function the existing test of each variant compares with -> (coefficients the call returns, high_chunk_is_zero)"""
    if variant in ("plain", "pi"):
        want = bn.plonk_quotient(on_h, shift, k1, k2, alpha, beta, gamma)
        return want[:3 * n], not any(want[3 * n:])
    co = {name: bn.ntt(v, inverse=True) for name, v in on_h.items()}
    if variant == "blinded":
        b = blinding
        co.update(l=bn.blind_coeffs(co["l"], n, b[0:2]), r=bn.blind_coeffs(co["r"], n, b[2:4]), o=bn.blind_coeffs(co["o"], n, b[4:6]),
                  z=bn.blind_coeffs(co["z"], n, b[6:9]))
        want = bn.gnark_quotient(co, n, shift, k1, k2, alpha, beta, gamma)
        return want, not any(want[3 * n + 6:])
    want = gm.quotient(co, n, shift, k1, k2, alpha, beta, gamma, 1)
    return want[:3 * n], not any(want[3 * n:])


def coset_is_defined(log_n, shift):
    """Z_H and x - 1 are non-zero at every point of the 4n coset: what the quotient's model divides by"""
    n = 1 << log_n
    x, w4 = shift % R, bn.root_of_unity(log_n + 2)
    for _ in range(4 * n):
        if (pow(x, n, R) - 1) % R == 0 or (x - 1) % R == 0:
            return False
        x = x * w4 % R
    return True
