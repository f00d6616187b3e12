"""CPU: the big-integer model of Groth16 with Bsb22 / Pedersen commitments (tools/groth16_commit_model.py) agrees with itself -
the honest prover over the key's points equals the prover from discrete logs, the bytes are 164 + 32 k long and parse back, the
verifier in the exponent accepts them and rejects every kind of damage - and with no commitment it is groth16_model."""
import os
import random
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_commit_model as cm  # noqa: E402
import groth16_model as gm  # noqa: E402

bn, R = gm.bn, gm.R


def _proof(n_constraints, counts, shape, seed, **kw):
    rng = random.Random(seed)
    inst = cm.CommittedInstance(n_constraints, rng, counts, **dict(gm.SHAPES[shape], **kw))
    td = cm.Trapdoor.random(rng)
    pk, vk = cm.setup(inst, td)
    w = cm.solve(inst, pk)
    return inst, td, pk, vk, w, rng.randrange(R), rng.randrange(R)


@pytest.fixture(scope="module")
def three():
    """one proof with three commitments that every rejection test damages (computed once, never changed)"""
    inst, td, pk, vk, w, r, s = _proof(16, [3, 2, 2], "public3", 77, hashed_public=3)
    return inst, td, pk, w, r, s, cm.proof_bytes(*cm.prove_by_logs(inst, td, w, r, s))


@pytest.mark.parametrize("n_constraints,counts,shape", [(8, [2], "common"), (16, [3, 1], "public3"), (32, [2, 0, 3], "empty"),
                                                        (64, [5, 4], "absent"), (13, [1, 1, 1], "unit"), (40, [6], "all_b")])
def test_points_prover_equals_logs_prover_and_verifies(n_constraints, counts, shape):
    inst, td, pk, vk, w, r, s = _proof(n_constraints, counts, shape, 100 + n_constraints)
    k = len(counts)
    assert inst.satisfied(w) and w == cm.solve(inst, td=td)                       # the hint from points = the hint from logs
    assert len(pk["g1_k"]) == inst.n_wires - inst.n_public - sum(counts) - k and len(vk["ic"]) == inst.n_public + k
    sets = [set(c["private"]) for c in inst.commitments]
    assert all(c["private"] == sorted(c["private"]) for c in inst.commitments) and sum(map(len, sets)) == len(set().union(*sets))
    for j, c in enumerate(inst.commitments):
        assert all(e["wire"] in c["public"] for e in inst.commitments[:j])        # earlier commitment wires are hashed
        if j and counts[j]:                                                       # a committed wire depends on challenge j - 1
            before = inst.solve(lambda i, w_: w[inst.commitments[i]["wire"]] + (i == j - 1), upto=j)
            assert any(before[i] != w[i] for i in c["private"])
        if not counts[j]:
            assert cm.commit(pk, j, w) is None
    pts = cm.prove(inst, pk, w, r, s)
    assert pts == cm.prove_by_logs(inst, td, w, r, s)
    data = cm.proof_bytes(*pts)
    assert len(data) == 164 + 32 * k
    assert cm.proof_from_bytes(data) == pts
    assert cm.verify_trapdoor(data, inst, td, w, r, s)


def test_no_commitment_is_groth16_model():
    rng = random.Random(5)
    inst = cm.CommittedInstance(12, rng, [], n_public=2)
    plain = gm.Instance(12, random.Random(5), n_public=2)
    assert inst.csr == plain.csr
    td = cm.Trapdoor.random(rng)
    pk, _ = cm.setup(inst, td)
    w = cm.solve(inst, pk)
    assert w == plain.witness
    r, s = rng.randrange(R), rng.randrange(R)
    ar, bs, krs, cs, pok = cm.prove(inst, pk, w, r, s)
    assert (ar, bs, krs) == gm.prove(plain, gm.setup(plain, td)[0], w, r, s) and cs == [] and pok is None
    data = cm.proof_bytes(ar, bs, krs)
    assert data == gm.proof_bytes(ar, bs, krs) and len(data) == 164
    assert cm.verify_trapdoor(data, inst, td, w, r, s) and gm.verify_trapdoor(data, plain, td, w, r, s)


REGIONS = [("Ar", 5), ("Bs", 40), ("Bs", 90), ("Krs", 100), ("count", 131), ("count", 128), ("C_0", 140), ("C_1", 172), ("C_2", 204), ("Pok", 230)]


@pytest.mark.parametrize("region,at", REGIONS)
def test_a_flipped_byte_is_rejected(three, region, at):
    inst, td, pk, w, r, s, data = three
    assert len(data) == 260 and cm.verify_trapdoor(data, inst, td, w, r, s)
    bad = bytearray(data)
    bad[at] ^= 0x04
    assert not cm.verify_trapdoor(bytes(bad), inst, td, w, r, s), region


def test_a_changed_hashed_public_input_is_rejected(three):
    inst, td, pk, w, r, s, data = three
    for wire in (1, 2):
        assert all(wire in c["public"] for c in inst.commitments)               # hashed_public = 3: every public wire is hashed
        public = list(w[1:inst.n_public])
        public[wire - 1] = (public[wire - 1] + 1) % R
        assert not cm.verify_trapdoor(data, inst, td, w, r, s, public=public)
    assert cm.verify_trapdoor(data, inst, td, w, r, s, public=list(w[1:inst.n_public]))


def test_pok_with_another_rho_is_rejected(three):
    inst, td, pk, w, r, s, data = three
    rho = cm.fold_challenge([w[c["wire"]] for c in inst.commitments])
    assert cm.proof_bytes(*cm.prove_by_logs(inst, td, w, r, s, rho=rho)) == data
    pts = cm.prove_by_logs(inst, td, w, r, s, rho=(rho + 1) % R)
    assert pts[:4] == cm.proof_from_bytes(data)[:4] and pts[4] != cm.proof_from_bytes(data)[4]
    assert not cm.verify_trapdoor(cm.proof_bytes(*pts), inst, td, w, r, s)
    assert cm.prove(inst, pk, w, r, s, rho=(rho + 1) % R)[4] == pts[4]        # the points prover folds the same way


def test_krs_that_includes_a_committed_wire_is_rejected(three):
    inst, td, pk, w, r, s, data = three
    a, b, c, _, _ = cm.proof_logs(inst, td, w, r, s)
    k_all = cm.k_logs(inst, td)
    for wire in (inst.commitments[0]["private"][0], inst.commitments[1]["wire"]):
        c_bad = (c + w[wire] * k_all[wire] % R * gm.inv(td.delta)) % R         # as if G1.K still held that wire's point
        assert c_bad != c
        ar, bs, krs, cs, pok = cm.proof_from_bytes(data)
        bad = cm.proof_bytes(ar, bs, gm.g1_gen_mul(c_bad), cs, pok)
        assert not cm.verify_trapdoor(bad, inst, td, w, r, s)                   # not the honest Krs
        assert not cm.verify_trapdoor(bad, inst, td, w, r, s, logs=(a, b, c_bad))   # and the pairing equation fails on it
    assert cm.verify_trapdoor(data, inst, td, w, r, s, logs=(a, b, c))
