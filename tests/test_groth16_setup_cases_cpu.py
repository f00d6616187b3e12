"""CPU: the yardstick of the Groth16 setup tests (tests/groth16_setup_cases.py) holds before the device leans on it: on every
aimed instance the model's setup gives a key under which the model's honest proof passes the model's trapdoor verifier; the
hand-made instances have the property they were made for; and `setup_logs` - the discrete logs the large device cases are checked
against - equals the model's points array by array."""
import random

import pytest

import groth16_setup_cases as gc

gm, cm, bn, R = gc.gm, gc.cm, gc.bn, gc.R


@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_model_setup_prove_verify(name):
    inst, td = gc.case(name)
    assert inst.satisfied()
    pk, vk = gm.setup(inst, td)
    assert len(pk["g1_a"]) == pk["infinity_a"].count(False) and len(pk["g1_b"]) == len(pk["g2_b"]) == pk["infinity_b"].count(False)
    assert len(pk["g1_k"]) == inst.n_wires - inst.n_public and len(pk["g1_z"]) == inst.n - 1 and len(vk["ic"]) == inst.n_public
    rng = random.Random(name)
    r, s = rng.randrange(R), rng.randrange(R)
    data = gm.proof_bytes(*gm.prove(inst, pk, inst.witness, r, s))
    assert gm.verify_trapdoor(data, inst, td, inst.witness, r, s)
    other = gm.Trapdoor(td.tau, td.alpha, td.beta, td.gamma, (td.delta + 1) % R)
    assert not gm.verify_trapdoor(data, inst, other, inst.witness, r, s)          # the verifier does look at the key


@pytest.mark.parametrize("name", gc.COMMITTED_NAMES)
def test_committed_model_setup_prove_verify(name):
    inst, td = gc.case(name)
    pk, vk = cm.setup(inst, td)
    assert len(vk["ic"]) == inst.n_public + inst.k
    assert len(pk["g1_k"]) == inst.n_wires - inst.n_public - inst.n_committed - inst.k
    w = cm.solve(inst, pk)
    assert inst.satisfied(w)
    rng = random.Random(name)
    r, s = rng.randrange(R), rng.randrange(R)
    data = cm.proof_bytes(*cm.prove(inst, pk, w, r, s))
    assert cm.verify_trapdoor(data, inst, td, w, r, s)


def test_cancelling_wire_occurs_and_is_masked():
    inst, td = gc.case("cancel")
    assert inst.occurs("A")[1] and inst.rows["A"][0].count((1, 1)) == 1 and inst.rows["A"][0].count((1, 2)) == 1
    assert (inst.coeffs[1] + inst.coeffs[2]) % R == 0 and inst.coeffs[1] != 0
    pk, _ = gm.setup(inst, td)
    assert pk["infinity_a"][1] and not pk["infinity_b"][1]
    assert gm.wire_polys_at(inst, td.tau)[0][1] == 0


def test_one_sits_in_every_row_of_a():
    inst, td = gc.case("one_every-12")
    assert all(any(i == 0 for i, _ in row) for row in inst.rows["A"]) and inst.n_constraints == 12
    assert inst.csr["A"][1].count(0) == 12
    big = gc.one_every_instance(100, random.Random(5), n_public=3)
    assert big.csr["A"][1].count(0) == 100 and big.n_public == 3 and big.satisfied()


def _points(logs, g2=False):
    mul = gm.g2_gen_mul if g2 else gm.g1_gen_mul
    return [mul(x) for x in logs] if isinstance(logs, list) else mul(logs)


@pytest.mark.parametrize("name", ["public3-13", "cancel", "absent-50"])
def test_logs_equal_model(name):
    inst, td = gc.case(name)
    pk, vk = gm.setup(inst, td)
    lpk, lvk = gc.setup_logs(inst, td)
    assert lpk["infinity_a"] == pk["infinity_a"] and lpk["infinity_b"] == pk["infinity_b"]
    for key in ("g1_a", "g1_b", "g1_k", "g1_z", "g1_alpha", "g1_beta", "g1_delta"):
        assert _points(lpk[key]) == pk[key], key
    for key in ("g2_b", "g2_beta", "g2_delta"):
        assert _points(lpk[key], g2=True) == pk[key], key
    assert _points(lvk["ic"]) == vk["ic"] and _points(lvk["g2_gamma"], g2=True) == vk["g2_gamma"]
    assert _points(lvk["g1_alpha"]) == pk["g1_alpha"] and _points(lvk["g2_beta"], g2=True) == pk["g2_beta"]
    assert True in pk["infinity_a"] or name == "public3-13"            # the masked cases do mask something


def test_logs_equal_committed_model():
    name = gc.COMMITTED_NAMES[2]
    inst, td = gc.case(name)
    pk, vk = cm.setup(inst, td)
    lpk, lvk = gc.setup_logs(inst, td)
    assert _points(lpk["g1_k"]) == pk["g1_k"] and _points(lvk["ic"]) == vk["ic"]
    for got, want in zip(lpk["commitments"], pk["commitments"]):
        assert _points(got["basis"]) == want["basis"] and _points(got["basis_exp_sigma"]) == want["basis_exp_sigma"]
    assert lvk["pedersen_g"] == 1 and (lvk["pedersen_g_root_sigma_neg"] + td.sigma) % R == 0
    import bn254_pairing_model as pm
    assert pm.pedersen_vk(td) == (gm.g2_gen_mul(lvk["pedersen_g"]), gm.g2_gen_mul(lvk["pedersen_g_root_sigma_neg"]))
