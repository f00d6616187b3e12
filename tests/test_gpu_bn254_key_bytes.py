"""GPU: gnark's two containers of points through the device codec - kzg.SRS (bn254_plonk.srs_to_bytes / srs_from_bytes) and
groth16.ProvingKey (bn254_groth16.Setup.proving_key_bytes / ProvingKey.from_bytes) - against tools/gnark_bytes_model.py, the
place of record for both layouts.  Bytes equal the model's in both modes; what is read back proves the
same bytes as what was written; a corrupted or truncated file is refused naming the section (and the point)."""
import os
import random
import sys

import numpy as np
import pytest

import bn254_plonk_setup_cases as plonk_cases
import groth16_setup_cases as gc
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bytes_model as gb  # noqa: E402

pytestmark = pytest.mark.gpu
gm, cm, R = gc.gm, gc.cm, gc.R
E_INVAL = -1
K0_CASE = min(gc.CASE_NAMES, key=lambda name: gc.case(name)[0].n_constraints)            # the smallest k = 0 case
K1_CASE = min((n for n in gc.COMMITTED_NAMES if n.endswith("-k1")), key=lambda name: gc.case(name)[0].n_constraints)


def _g1(nlx, words):
    return [nlx.bn254_g1_unpack(w) for w in np.asarray(words).reshape(-1, 8)]


def _g2(nlx, words):
    return [nlx.bn254_g2_unpack(w) for w in np.asarray(words).reshape(-1, 16)]


# ---- kzg.SRS ----
@pytest.fixture(scope="module")
def srs(nlx, ctx):
    return nlx.bn254_plonk.kzg_srs(ctx, random.Random(83).randrange(1, R), (1 << 3) + 3)


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
def test_srs_bytes_equal_the_models_and_read_back(nlx, ctx, srs, raw):
    P = nlx.bn254_plonk
    g1, g2_one, g2_tau = srs
    data = P.srs_to_bytes(ctx, g1, g2_one, g2_tau, raw=raw)
    assert data == gb.srs_bytes(_g1(nlx, g1), _g2(nlx, g2_one)[0], _g2(nlx, g2_tau)[0], raw)
    import torch
    assert P.srs_to_bytes(ctx, torch.from_numpy(g1.view(np.int64)).to("cuda:0"), g2_one, g2_tau, raw=raw) == data
    for device in (None, "cuda:0"):
        r1, r2, r3 = P.srs_from_bytes(ctx, data, device=device)
        if device:
            assert r1.is_cuda
            r1 = r1.cpu().numpy().view(np.uint64)
        assert np.array_equal(r1, g1) and np.array_equal(r2, g2_one) and np.array_equal(r3, g2_tau)


def test_plonk_chain_on_the_decoded_srs_gives_the_same_proof(nlx, ctx, srs):
    """setup -> key -> wires -> prove -> verify at 2^3 gates, once on the SRS as made and once on the SRS read back from bytes"""
    P = nlx.bn254_plonk
    c = plonk_cases.case("n8")
    assert c.log_n == 3
    blinding = [random.Random(9).randrange(R) for _ in range(9)]
    decoded = P.srs_from_bytes(ctx, P.srs_to_bytes(ctx, *srs), device="cuda:0")
    proofs = []
    for g1, g2_one, g2_tau in (srs, decoded):
        key, s = P.setup(ctx, c.n_variables, c.n_public, c.constraints, c.coeffs, g1, commitments=c.sets)
        l, r, o = s.wires(c.complete())
        proof = P.prove_resident(key, l, r, o, c.public_inputs, blinding=blinding)
        vk = P.VerifyingKey.from_resident(key, g2_one, g2_tau, c.n_public)
        assert vk.verify(proof, c.public_inputs).accepted
        proofs.append(bytes(proof))
        for x in (vk, key, s):
            x.close()
    assert proofs[0] == proofs[1]


def test_srs_refusals_name_the_section(nlx, ctx, srs):
    P = nlx.bn254_plonk
    data = P.srs_to_bytes(ctx, *srs)
    for cut, section in ((2, "Pk.G1 count"), (4, "Pk.G1:"), (4 + 32 * 5 + 1, "Pk.G1:"), (4 + 32 * 11 + 10, "Vk.G2[0]"), (len(data) - 40, "Vk.G2[1]"), (len(data) - 1, "Vk.G1")):
        with pytest.raises(nlx.NlxError) as e:
            P.srs_from_bytes(ctx, data[:cut])
        assert e.value.code == E_INVAL and "truncated in " + section in str(e.value), (cut, str(e.value))
    with pytest.raises(nlx.NlxError) as e:
        P.srs_from_bytes(ctx, data + b"\x00")
    assert "SRS: 1 trailing" in str(e.value)
    bad = bytearray(data)
    bad[4 + 32 * 6] ^= 0x40                                                    # 10 <-> 11 picks -y: on the curve, no longer Pk.G1[6] ...
    r1, _, _ = P.srs_from_bytes(ctx, bytes(bad))
    assert not np.array_equal(r1[6], srs[0][6]) and np.array_equal(np.delete(r1, 6, 0), np.delete(srs[0], 6, 0))
    bad[4 + 32 * 6] &= 0x3F                                                    # ... and flag 00 in a compressed file is refused
    with pytest.raises(nlx.NlxError) as e:
        P.srs_from_bytes(ctx, bytes(bad))
    assert e.value.code == E_INVAL and "Pk.G1 point 6:" in str(e.value)


# ---- groth16.ProvingKey ----
def _trapdoor(g16, td):
    return g16.Trapdoor(td.tau, td.alpha, td.beta, td.gamma, td.delta, getattr(td, "sigma", None))


def _commitments(inst):
    return [dict(private=c["private"], public=c["public"], wire=c["wire"]) for c in getattr(inst, "commitments", [])] or None


@pytest.fixture(scope="module")
def setups(nlx, ctx):
    g16 = nlx.bn254_groth16
    made = {}

    def get(name):
        if name not in made:
            inst, td = gc.case(name)
            r1cs = gc.r1cs_arrays(np, g16.fr_pack, inst)
            s = g16.Setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, r1cs, _trapdoor(g16, td), _commitments(inst))
            made[name] = (inst, r1cs, s)
        return made[name]
    yield get
    for _, _, s in made.values():
        s.close()


def _model_key(nlx, inst, a):
    """the model's container input from Setup.arrays()"""
    return {"log_n": inst.log_n, "n_wires": inst.n_wires,
            "g1_alpha": _g1(nlx, a.g1_alpha)[0], "g1_beta": _g1(nlx, a.g1_beta)[0], "g1_delta": _g1(nlx, a.g1_delta)[0],
            "g2_beta": _g2(nlx, a.g2_beta)[0], "g2_delta": _g2(nlx, a.g2_delta)[0],
            "g1_a": _g1(nlx, a.g1_a), "g1_b": _g1(nlx, a.g1_b), "g1_z": _g1(nlx, a.g1_z), "g1_k": _g1(nlx, a.g1_k), "g2_b": _g2(nlx, a.g2_b),
            "infinity_a": [bool(x) for x in a.infinity_a], "infinity_b": [bool(x) for x in a.infinity_b],
            "commitments": [(_g1(nlx, c["basis"]), _g1(nlx, c["basis_exp_sigma"])) for c in a.commitments]}


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
@pytest.mark.parametrize("name", (K0_CASE, K1_CASE))
def test_proving_key_bytes_equal_the_models_container(nlx, setups, name, raw):
    inst, _, s = setups(name)
    data = s.proving_key_bytes(raw=raw)
    model = _model_key(nlx, inst, s.arrays())
    assert data == gb.key_bytes(model, raw)
    assert gb.key_parse(data) == model


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
@pytest.mark.parametrize("name", (K0_CASE, K1_CASE))
def test_a_key_read_from_bytes_proves_the_same_bytes(nlx, ctx, setups, name, raw):
    g16 = nlx.bn254_groth16
    inst, r1cs, s = setups(name)
    rng = random.Random("key-bytes-" + name)
    r, s_ = rng.randrange(R), rng.randrange(R)
    direct = s.key()
    read = g16.ProvingKey.from_bytes(ctx, s.proving_key_bytes(raw=raw), r1cs=r1cs, commitments=_commitments(inst))
    assert (read.log_n, read.n_wires, read.n_public, read.n_constraints) == (inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints)
    assert read.info()["terms"] == direct.info()["terms"]
    vk = s.verifying_key()
    if getattr(inst, "commitments", None):
        def challenge(j, partial):
            words = g16.fr_pack([x or 0 for x in partial])
            return g16.commitment_challenge(direct, j, g16.commit(direct, j, words), words)
        w = inst.solve(challenge)
        proofs = []
        for key in (direct, read):
            ar, bs, krs, cs, pok = g16.prove_committed(key, g16.fr_pack(w), r, s_)
            proofs.append(g16.proof_bytes(ar, bs, krs, cs, pok))
    else:
        w = inst.witness
        proofs = [g16.proof_bytes(*g16.prove(key, g16.fr_pack(w), r, s_)) for key in (direct, read)]
    assert proofs[0] == proofs[1]
    verdict = vk.verify(proofs[1], w[1:inst.n_public])
    assert verdict.accepted, str(verdict)
    for h in (direct, read, vk):
        h.close()


def _offset_of_k(model, raw):
    """where the G1.K slice's points begin in the container"""
    s1 = gb.G1_SIZE[raw]
    return gb.DOMAIN_BYTES + 3 * s1 + sum(4 + s1 * len(model[k]) for k in ("g1_a", "g1_b", "g1_z")) + 4


def test_corrupted_and_truncated_keys_are_refused(nlx, ctx, setups):
    g16 = nlx.bn254_groth16
    inst, r1cs, s = setups(K0_CASE)
    data = s.proving_key_bytes()
    model = _model_key(nlx, inst, s.arrays())
    assert len(model["g1_k"]) >= 3
    at = _offset_of_k(model, False) + 2 * 32
    assert data[at:at + 32] == gb.g1_encode(model["g1_k"][2])
    bad = bytearray(data)
    bad[at] &= 0x7F                                                            # flag 10 / 11 -> 00 / 01: refused in a compressed file
    with pytest.raises(nlx.NlxError) as e:
        g16.ProvingKey.from_bytes(ctx, bytes(bad), r1cs=r1cs)
    assert e.value.code == E_INVAL and "G1.K point 2:" in str(e.value), str(e.value)
    for cut, section in ((100, "domain"), (gb.DOMAIN_BYTES, "G1.Alpha"), (gb.DOMAIN_BYTES + 40, "G1.Beta"), (at + 5, "G1.K"), (len(data) - 2, "commitment keys count")):
        with pytest.raises(nlx.NlxError) as e:
            g16.ProvingKey.from_bytes(ctx, data[:cut], r1cs=r1cs)
        assert e.value.code == E_INVAL and "truncated in " + section in str(e.value), (cut, str(e.value))
    with pytest.raises(nlx.NlxError) as e:
        g16.ProvingKey.from_bytes(ctx, data + b"\x00", r1cs=r1cs)
    assert "proving key: 1 trailing" in str(e.value)
    with pytest.raises(nlx.NlxError) as e:                                     # a key with no commitment keys, one wire set given
        g16.ProvingKey.from_bytes(ctx, data, r1cs=r1cs, commitments=[dict(private=[2], public=[], wire=3)])
    assert "commitment keys count" in str(e.value)
    before = ctx.memory()[1]
    g16.ProvingKey.from_bytes(ctx, data, r1cs=r1cs).close()
    assert ctx.memory()[1] == before
