"""CPU tests of the big-integer pairing model (tools/bn254_pairing_model.py): the pairing's defining properties, its Groth16
verifiers against the trapdoor verifiers of tools/groth16_model.py and tools/groth16_commit_model.py, the exponent of the
device's hard-part chain, and the generated constants file against a fresh run of its generator."""
import os
import random
import sys

import pytest

from conftest import ROOT
from groth16_verify_cases import case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_pairing_model as pm  # noqa: E402
import gen_bn254_pairing  # noqa: E402

bn, R, Q = pm.bn, pm.R, pm.Q


@pytest.fixture(scope="module")
def e11():
    return pm.pairing(bn.G1, bn.G2)


def test_pairing_is_not_degenerate_and_has_order_r(e11):
    assert e11 != pm.F12_ONE
    assert pm.f12_pow(e11, R) == pm.F12_ONE


def test_bilinear(e11):
    rng = random.Random(12)
    for a, b in [(rng.randrange(1, R), rng.randrange(1, R)), (1, R - 1), (R - 1, 1), (R - 1, R - 1), (1, 1)]:
        assert pm.pairing(bn.g1_mul(a, bn.G1), bn.g2_mul(b, bn.G2)) == pm.f12_pow(e11, a * b % R), (a, b)


def test_inverse_pair_and_infinity(e11):
    p, q2 = bn.g1_mul(77, bn.G1), bn.g2_mul(1234567, bn.G2)
    assert pm.pairing_product([(p, q2), (bn.g1_neg(p), q2)]) == pm.F12_ONE
    assert pm.f12_mul(pm.pairing(p, q2), pm.pairing(bn.g1_neg(p), q2)) == pm.F12_ONE
    assert pm.pairing(None, q2) == pm.F12_ONE and pm.pairing(p, None) == pm.F12_ONE and pm.miller_loop(None, None) == pm.F12_ONE


def test_tower_order_round_trip_and_inverse():
    rng = random.Random(3)
    a = tuple(rng.randrange(Q) for _ in range(12))
    assert pm.f12_from_gnark(pm.f12_to_gnark(a)) == a
    assert pm.f12_mul(a, pm.f12_inv(a)) == pm.F12_ONE
    u = pm.f12_from_gnark([0, 1] + [0] * 10)                  # u, with u^2 = -1 and (9 + u) = w^6
    assert pm.f12_mul(u, u) == pm.f12_from_fq(Q - 1)
    w = (0, 1) + (0,) * 10
    assert pm.f12_pow(w, 6) == pm.f12_from_gnark([9, 1] + [0] * 10)


def test_hard_part_chain_raises_to_the_stated_multiple():
    assert pm.hard_chain_multiple() == pm.HARD_MULTIPLE
    assert pm.FINAL_EXPONENT == pm.HARD_MULTIPLE * ((Q**12 - 1) // R)


def test_subgroup_test():
    rng = random.Random(5)
    assert pm.g2_in_subgroup(bn.G2) and pm.g2_in_subgroup(bn.g2_mul(rng.randrange(R), bn.G2)) and pm.g2_in_subgroup(None)
    outside = pm.twist_point_outside_subgroup(rng)
    assert pm.g2_on_curve(outside) and not pm.g2_in_subgroup(outside)


def test_generated_constants_are_fresh():
    with open(gen_bn254_pairing.OUT) as f:
        assert f.read() == gen_bn254_pairing.render()


# the nine keys of the issue: every shape x k accepts, and every named tamper is judged as the trapdoor verifier judges it
@pytest.mark.parametrize("shape", ["common", "public3", "all_b"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_model_verifier_accepts_honest_proofs(shape, k):
    c = case(shape, 8, k)
    assert c.trapdoor_accepts(c.proof) and c.model_accepts(c.proof)


@pytest.mark.parametrize("shape", ["common", "public3", "all_b"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_model_verifier_agrees_with_the_trapdoor_on_tampers(shape, k):
    c = case(shape, 8, k)
    tampers = c.tampers()
    labels = [t[0] for t in tampers]
    want = ["Ar replaced", "Krs replaced", "Bs replaced", "Bs outside the subgroup", "Krs: x with no y", "Bs: X.A1 = q", "Pok: x = q",
            "one byte short", "one byte long", "commitment count off by one"] + (["Pok replaced", "C_0 replaced"] if k else [])
    # "common" has the constant wire alone: there is no public input to change, and the test says so rather than skip it unseen
    assert ("public input changed" in labels) == (c.inst.n_public > 1) and c.inst.n_public == (1 if shape == "common" else 3)
    assert sorted(labels) == sorted(want + (["public input changed"] if c.inst.n_public > 1 else []))
    for label, data, public, reason, _ in tampers:
        assert not c.trapdoor_accepts(data, public), label
        assert not c.model_accepts(data, public), label
