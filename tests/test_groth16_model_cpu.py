"""CPU: the big-integer model of Groth16 proofs in gnark's shape (tools/groth16_model.py) - instances of every generator shape
are proved from the key's points, the trapdoor verifier accepts the bytes and rejects the three tamperings, the bytes are 164
long and round-trip through the parser, G2 compression round-trips on both signs of Y and with Y.A1 = 0.  Needs no GPU and no
library."""
import os
import random
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_model as gm  # noqa: E402

bn = gm.bn
R, Q = gm.R, gm.Q

# (shape, n_constraints): 2^2 .. 2^6 constraints, powers of two and not; `long` needs room for its three long rows
CASES = [("common", 4), ("common", 7), ("public3", 8), ("public3", 13), ("empty", 16), ("absent", 24), ("all_a", 32), ("all_b", 21),
         ("unit", 11), ("general", 12), ("long", 37), ("common", 64)]


def _instance(shape, n_constraints, seed):
    rng = random.Random(seed)
    kw = dict(gm.SHAPES[shape])
    if shape == "long":
        kw["long_len"] = 70          # past the device's lane / wave threshold, and cheap for the model's point sums
    inst = gm.Instance(n_constraints, rng, **kw)
    td = gm.Trapdoor.random(rng)
    return inst, td, rng


def test_fixed_base_and_jacobian_g2_agree_with_the_frozen_model():
    rng = random.Random(1)
    for k in (0, 1, 2, 15, 16, R - 1, rng.randrange(R), rng.randrange(R)):
        assert gm.g1_gen_mul(k) == bn.g1_mul(k, bn.G1), k
        assert gm.g2_gen_mul(k) == bn.g2_mul(k, bn.G2), k
    p = bn.g2_mul(rng.randrange(R), bn.G2)
    for k in (0, 1, 3, rng.randrange(R)):
        assert gm.g2_mul(k, p) == bn.g2_mul(k, p)


@pytest.mark.parametrize("shape,n_constraints", CASES)
def test_model_proof_verifies_and_tampering_is_rejected(shape, n_constraints):
    inst, td, rng = _instance(shape, n_constraints, 100 + n_constraints)
    assert inst.satisfied()
    assert inst.n == 1 << inst.log_n and inst.n >= n_constraints and (inst.n // 2 < n_constraints or inst.n == 2)
    assert inst.witness[0] == 1 and inst.n_public == gm.SHAPES[shape].get("n_public", 1)
    a, b, c = inst.abc()
    assert len(a) == inst.n and not any(a[n_constraints:] + b[n_constraints:] + c[n_constraints:])
    pk, vk = gm.setup(inst, td)
    # gnark's layout: filtered queries and their masks, K over the private wires, n - 1 powers in Z
    occ_a, occ_b = inst.occurs("A"), inst.occurs("B")
    assert all(pk["infinity_a"][i] for i in range(inst.n_wires) if not occ_a[i])
    assert all(pk["infinity_b"][i] for i in range(inst.n_wires) if not occ_b[i])
    assert len(pk["g1_a"]) == pk["infinity_a"].count(False) and len(pk["g1_b"]) == len(pk["g2_b"]) == pk["infinity_b"].count(False)
    assert len(pk["g1_k"]) == inst.n_wires - inst.n_public and len(pk["g1_z"]) == inst.n - 1 and len(vk["ic"]) == inst.n_public
    if shape == "absent":
        assert any(pk["infinity_a"]) and any(pk["infinity_b"])
    if shape in ("all_a", "all_b"):
        assert len(inst.rows["A" if shape == "all_a" else "B"][-1]) == inst.n_wires
    if shape == "empty":
        assert sum(1 for j in range(n_constraints) if not inst.rows["A"][j] and not inst.rows["B"][j] and not inst.rows["C"][j]) >= 2
    r, s = rng.randrange(R), rng.randrange(R)
    pts = gm.prove(inst, pk, inst.witness, r, s)
    assert pts == gm.prove_by_logs(inst, td, inst.witness, r, s)
    data = gm.proof_bytes(*pts)
    assert len(data) == gm.PROOF_BYTES == 164 and gm.proof_from_bytes(data) == pts
    assert gm.verify_trapdoor(data, inst, td, inst.witness, r, s)
    # 1. Krs from a wrong h
    h = bn.groth16_quotient(a, b, c, gm.COSET_SHIFT)
    assert h[-1] == 0
    bad_h = list(h)
    bad_h[0] = (bad_h[0] + 1) % R
    bad = gm.proof_bytes(*gm.prove(inst, pk, inst.witness, r, s, h=bad_h))
    assert bad != data and not gm.verify_trapdoor(bad, inst, td, inst.witness, r, s)
    # 2. one byte changed (in each of the three points and in the tail)
    for at in (5, 40, 100, 130, 140):
        flipped = bytearray(data)
        flipped[at] ^= 1
        assert not gm.verify_trapdoor(bytes(flipped), inst, td, inst.witness, r, s), at
    # 3. a public input changed (an instance without public inputs has only the constant wire to offer)
    if inst.n_public > 1:
        public = list(inst.witness[1:inst.n_public])
        public[0] = (public[0] + 1) % R
        assert not gm.verify_trapdoor(data, inst, td, inst.witness, r, s, public=public)
    # an unsatisfied witness is visible in a b - c on H (what the device checks before it commits)
    w_bad = inst.unsatisfied_witness()
    assert not inst.satisfied(w_bad) and sum(x != y for x, y in zip(w_bad, inst.witness)) == 1


@pytest.mark.parametrize("r,s", [(0, 0), (R - 1, R - 1), (0, R - 1)])
def test_extreme_blinding_scalars(r, s):
    inst, td, _ = _instance("public3", 6, 7)
    pk, _ = gm.setup(inst, td)
    pts = gm.prove(inst, pk, inst.witness, r, s)
    assert pts == gm.prove_by_logs(inst, td, inst.witness, r, s)
    assert gm.verify_trapdoor(gm.proof_bytes(*pts), inst, td, inst.witness, r, s)
    assert not gm.verify_trapdoor(gm.proof_bytes(*pts), inst, td, inst.witness, (r + 1) % R, s)


def _f2_pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = bn.f2_mul(out, a)
        a = bn.f2_mul(a, a)
        e >>= 1
    return out


def _f2_cube_root(c):
    """a cube root of c in Fq2, or None.  q^2 - 1 = 9 m with 3 not dividing m: c^k for 3 k = 1 mod m is a root up to a cube root of
    unity, which a ninth root of unity repairs."""
    m = (Q * Q - 1) // 9
    assert m % 3 and (Q * Q - 1) % 9 == 0
    if _f2_pow(c, 3 * m) != (1, 0):
        return None
    x = _f2_pow(c, pow(3, -1, m))
    z = 2
    while True:
        eta = _f2_pow((z, 1), m)
        if _f2_pow(eta, 3) != (1, 0):
            break
        z += 1
    for _ in range(9):
        if bn.f2_mul(bn.f2_mul(x, x), x) == c:
            return x
        x = bn.f2_mul(x, eta)
    return None


def test_g2_compression_round_trips():
    rng = random.Random(22)
    seen = set()
    while len(seen) < 2:                                  # both signs of Y
        p = bn.g2_mul(rng.randrange(1, R), bn.G2)
        for pt in (p, bn.g2_neg(p)):
            data = gm.g2_compress(pt)
            assert len(data) == 64 and data[0] >> 6 == (3 if gm.g2_y_is_largest(pt[1]) else 2)
            assert gm.g2_decompress(data) == pt
            seen.add(data[0] >> 6)
        assert gm.g2_compress(p)[0] >> 6 != gm.g2_compress(bn.g2_neg(p))[0] >> 6
    assert gm.g2_decompress(gm.g2_compress(None)) is None and gm.g2_compress(None) == bytes([0x40]) + bytes(63)
    # X.A1 comes first
    p = bn.g2_mul(5, bn.G2)
    data = gm.g2_compress(p)
    assert int.from_bytes(data[32:], "big") == p[0][0] and int.from_bytes(bytes([data[0] & 0x3F]) + data[1:32], "big") == p[0][1]
    # Y.A1 = 0: a point of the twist y^2 = x^3 + b' with a real y (compression is defined on the curve, not only on the subgroup):
    # y = (y0, 0), x a cube root of y0^2 - b'; the sign is then decided on Y.A0
    y0, found = 1, 0
    while found < 2:
        y0 += 1
        x = _f2_cube_root(bn.f2_sub((y0 * y0 % Q, 0), bn.B2))
        if x is None:
            continue
        for y in ((y0, 0), (Q - y0, 0)):
            pt = (x, y)
            data = gm.g2_compress(pt)
            assert data[0] >> 6 == (3 if y[0] > (Q - 1) // 2 else 2)
            assert gm.g2_decompress(data) == pt
        found += 1
