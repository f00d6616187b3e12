"""GPU: nlx_bn254_groth16_setup - gnark's groth16.Setup from a trapdoor on the device - against the big-integer models
(tools/groth16_model.py rule 3, tools/groth16_commit_model.py rule 1; recalled from gnark v0.9, unpinned).  Point by point on the
instances tests/test_groth16_setup_cases_cpu.py validates (up to 333 constraints, k = 0 .. 3); in the exponent, through the
library's MSM, at 2^12 constraints with ONE in every row (the wave-per-wire path) and at 2^14; end to end at 2^12 - setup, device
prover, device verifier: the first honest key of that size the two meet on; the key of nlx_bn254_groth16_setup_key against a key
built from the model's points; every refusal, with nothing left allocated.  Every comparison is exact."""
import functools
import random

import numpy as np
import pytest

import groth16_setup_cases as gc

pytestmark = pytest.mark.gpu
gm, cm, bn, R = gc.gm, gc.cm, gc.bn, gc.R
E_INVAL, E_RANGE = -1, -4


@pytest.fixture(scope="module")
def g16(nlx):
    return nlx.bn254_groth16


@functools.lru_cache(maxsize=None)
def _model(name):
    """(instance, trapdoor, pk, vk) of the model, once per module"""
    inst, td = gc.case(name)
    pk, vk = (cm if name in gc.COMMITTED_NAMES else gm).setup(inst, td)
    return inst, td, pk, vk


def _trapdoor(g16, td):
    return g16.Trapdoor(td.tau, td.alpha, td.beta, td.gamma, td.delta, getattr(td, "sigma", None))


def _commitments(inst):
    return [dict(private=c["private"], public=c["public"], wire=c["wire"]) for c in getattr(inst, "commitments", [])] or None


def _setup(g16, ctx, inst, td):
    return g16.Setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, gc.r1cs_arrays(np, g16.fr_pack, inst), _trapdoor(g16, td),
                     _commitments(inst))


def _g1(nlx, words):
    return [nlx.bn254_g1_unpack(w) for w in np.asarray(words).reshape(-1, 8)]


def _g2(nlx, words):
    return [nlx.bn254_g2_unpack(w) for w in np.asarray(words).reshape(-1, 16)]


def _check_points(nlx, a, inst, td, pk, vk):
    assert [bool(x) for x in a.infinity_a] == pk["infinity_a"] and [bool(x) for x in a.infinity_b] == pk["infinity_b"]
    for key in ("g1_a", "g1_b", "g1_k", "g1_z"):
        assert _g1(nlx, getattr(a, key)) == pk[key], key
    assert _g2(nlx, a.g2_b) == pk["g2_b"]
    for key in ("g1_alpha", "g1_beta", "g1_delta"):
        assert _g1(nlx, getattr(a, key)) == [pk[key]], key
    assert _g2(nlx, a.g2_beta) == [pk["g2_beta"]] and _g2(nlx, a.g2_delta) == [pk["g2_delta"]] and _g2(nlx, a.g2_gamma) == [vk["g2_gamma"]]
    assert _g1(nlx, a.ic) == vk["ic"]


@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_arrays_equal_model(nlx, ctx, g16, name):
    inst, td, pk, vk = _model(name)
    s = _setup(g16, ctx, inst, td)
    info = s.info()
    assert (info["g1_a"], info["g1_b"], info["g1_k"], info["g1_z"], info["ic"]) == (len(pk["g1_a"]), len(pk["g1_b"]), len(pk["g1_k"]), inst.n - 1, inst.n_public)
    assert info["commitments"] == 0 and info["committed_wires"] == 0
    a = s.arrays()
    _check_points(nlx, a, inst, td, pk, vk)
    assert a.commitments == [] and a.pedersen_g is None
    if name == "cancel":
        assert a.infinity_a[1] == 1 and inst.occurs("A")[1]              # the wire occurs, its terms cancel
    assert info["wave_wires"] == (1 if name == "one_every-100" else 0)  # ONE, 100 terms in A: the wave path
    s.close()


@pytest.mark.parametrize("name", gc.COMMITTED_NAMES)
def test_committed_arrays_equal_model(nlx, ctx, g16, name):
    inst, td, pk, vk = _model(name)
    s = _setup(g16, ctx, inst, td)
    info = s.info()
    assert info["commitments"] == inst.k and info["committed_wires"] == inst.n_committed and info["ic"] == inst.n_public + inst.k
    a = s.arrays()
    _check_points(nlx, a, inst, td, pk, vk)                              # ic's tail: the commitment wires' points
    assert len(a.commitments) == inst.k
    for got, want in zip(a.commitments, pk["commitments"]):
        assert _g1(nlx, got["basis"]) == want["basis"] and _g1(nlx, got["basis_exp_sigma"]) == want["basis_exp_sigma"]
    assert _g2(nlx, a.pedersen_g) == [bn.G2]
    assert _g2(nlx, a.pedersen_g_root_sigma_neg) == [gm.g2_gen_mul(R - td.sigma)]       # tools/bn254_pairing_model.py pedersen_vk
    # a device read of one array equals the host read
    dev = "cuda:%d" % ctx.device
    assert np.array_equal(s.read(g16.SETUP_G1_K, device=dev).cpu().numpy().view(np.uint64), a.g1_k)
    assert np.array_equal(s.read(g16.SETUP_INFINITY_B, device=dev).cpu().numpy(), a.infinity_b)
    s.close()


# ---- large instances, in the exponent: sum_i rho_i P_i = (sum_i rho_i log_i) G through the library's MSM ----
def _check_logs(nlx, ctx, a, lpk, lvk, seed):
    rng = random.Random(seed)

    def check(words, logs, g2=False):
        words = np.asarray(words).reshape(-1, 16 if g2 else 8)
        logs = logs if isinstance(logs, list) else [logs]
        assert len(words) == len(logs)
        if not logs:
            return
        rhos = [rng.getrandbits(128) for _ in logs]
        total = sum(r_ * x for r_, x in zip(rhos, logs)) % R
        rho_words = nlx.bn254_pack([rhos])[0]
        if g2:
            assert nlx.bn254_g2_unpack(nlx.bn254_msm_g2(ctx, words, rho_words)) == gm.g2_gen_mul(total)
        else:
            assert nlx.bn254_g1_unpack(nlx.bn254_msm_g1(ctx, words, rho_words)) == gm.g1_gen_mul(total)
    assert [bool(x) for x in a.infinity_a] == lpk["infinity_a"] and [bool(x) for x in a.infinity_b] == lpk["infinity_b"]   # log_i == 0
    for key in ("g1_a", "g1_b", "g1_k", "g1_z", "g1_alpha", "g1_beta", "g1_delta"):
        check(getattr(a, key), lpk[key])
    for key in ("g2_b", "g2_beta", "g2_delta"):
        check(getattr(a, key), lpk[key], g2=True)
    check(a.ic, lvk["ic"])
    check(a.g2_gamma, lvk["g2_gamma"], g2=True)
    # no point of a filtered query is the point at infinity
    assert np.asarray(a.g1_a).any(axis=1).all() and np.asarray(a.g2_b).any(axis=1).all()


def test_2_12_one_in_every_row(nlx, ctx, g16):
    rng = random.Random(4096)
    inst, td = gc.one_every_instance(1 << 12, rng, n_public=3), gm.Trapdoor.random(rng)
    s = _setup(g16, ctx, inst, td)
    assert s.info()["wave_wires"] >= 1 and inst.csr["A"][1].count(0) == 1 << 12
    _check_logs(nlx, ctx, s.arrays(), *gc.setup_logs(inst, td), seed=12)
    s.close()


def test_2_14_long_shape(nlx, ctx, g16):
    rng = random.Random(1 << 14)
    inst, td = gm.Instance(1 << 14, rng, **gm.SHAPES["long"]), gm.Trapdoor.random(rng)
    s = _setup(g16, ctx, inst, td)
    _check_logs(nlx, ctx, s.arrays(), *gc.setup_logs(inst, td), seed=14)
    s.close()


# ---- end to end at 2^12 constraints: setup -> device prover -> device verifier ----
def test_end_to_end_2_12(nlx, ctx, g16):
    rng = random.Random(212)
    inst = gm.Instance(1 << 12, rng, n_public=3)
    r1cs = gc.r1cs_arrays(np, g16.fr_pack, inst)
    td = _trapdoor(g16, gm.Trapdoor.random(rng))
    pk, vk, arrays = g16.setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, r1cs, trapdoor=td)
    w = inst.witness
    data = g16.proof_bytes(*g16.prove(pk, g16.fr_pack(w), rng.randrange(R), rng.randrange(R)))
    verdict = vk.verify(data, w[1:3])
    assert verdict.accepted, str(verdict)
    bad = vk.verify(data, [w[1], (w[2] + 1) % R])
    assert not bad.accepted and bad.reason == g16.VERIFY_PAIRING
    # another trapdoor's key rejects the proof; a trapdoor drawn by the library works as well
    pk2, vk2, _ = g16.setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, r1cs)
    other = vk2.verify(data, w[1:3])
    assert not other.accepted and other.reason == g16.VERIFY_PAIRING
    assert vk2.verify(g16.proof_bytes(*g16.prove(pk2, g16.fr_pack(w))), w[1:3]).accepted
    assert not np.array_equal(arrays.g1_alpha, np.zeros(8, dtype=np.uint64))
    for h in (pk, vk, pk2, vk2):
        h.close()


def test_end_to_end_2_12_committed(nlx, ctx, g16):
    rng = random.Random(2121)
    inst = cm.CommittedInstance(1 << 12, rng, [5], n_public=3)
    td = _trapdoor(g16, cm.Trapdoor.random(rng))
    r1cs = gc.r1cs_arrays(np, g16.fr_pack, inst)
    pk, vk, _ = g16.setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, r1cs, trapdoor=td, commitments=_commitments(inst))

    def challenge(j, partial):                                           # the solver's hint, on the device key
        words = g16.fr_pack([x or 0 for x in partial])
        return g16.commitment_challenge(pk, j, g16.commit(pk, j, words), words)
    w = inst.solve(challenge)
    assert inst.satisfied(w)
    data = g16.proof_bytes(*g16.prove_committed(pk, g16.fr_pack(w), rng.randrange(R), rng.randrange(R)))
    assert len(data) == 164 + 32
    verdict = vk.verify(data, w[1:3])
    assert verdict.accepted, str(verdict)
    bad = vk.verify(data, [(w[1] + 1) % R, w[2]])
    assert not bad.accepted and bad.reason == g16.VERIFY_PAIRING
    td2 = g16.Trapdoor.random()
    pk2, vk2, _ = g16.setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, r1cs, trapdoor=td2, commitments=_commitments(inst))
    assert not vk2.verify(data, w[1:3]).accepted
    for h in (pk, vk, pk2, vk2):
        h.close()


# ---- the key of nlx_bn254_groth16_setup_key against a key built from the model's points ----
def test_setup_key_equals_model_key(nlx, ctx, g16):
    inst, td, pk, vk = _model("unit-200")
    one = lambda p: nlx.bn254_g1_pack([p])[0]
    model_key = g16.ProvingKey(
        ctx, log_n=inst.log_n, n_wires=inst.n_wires, n_public=inst.n_public, n_constraints=inst.n_constraints,
        g1_a=nlx.bn254_g1_pack(pk["g1_a"]), g1_b=nlx.bn254_g1_pack(pk["g1_b"]), g2_b=nlx.bn254_g2_pack(pk["g2_b"]),
        g1_k=nlx.bn254_g1_pack(pk["g1_k"]), g1_z=nlx.bn254_g1_pack(pk["g1_z"]), infinity_a=np.array(pk["infinity_a"], dtype=np.uint8),
        infinity_b=np.array(pk["infinity_b"], dtype=np.uint8), g1_alpha=one(pk["g1_alpha"]), g1_beta=one(pk["g1_beta"]),
        g1_delta=one(pk["g1_delta"]), g2_beta=nlx.bn254_g2_pack([pk["g2_beta"]])[0], g2_delta=nlx.bn254_g2_pack([pk["g2_delta"]])[0],
        r1cs=gc.r1cs_arrays(np, g16.fr_pack, inst))
    s = _setup(g16, ctx, inst, td)
    key = s.key()
    s.close()                                                            # the key stands on its own
    rng = random.Random(200)
    r, s_ = rng.randrange(R), rng.randrange(R)
    w = g16.fr_pack(inst.witness)
    data = g16.proof_bytes(*g16.prove(key, w, r, s_))
    assert data == g16.proof_bytes(*g16.prove(model_key, w, r, s_))
    assert data == gm.proof_bytes(*gm.prove_by_logs(inst, td, inst.witness, r, s_)) and gm.verify_trapdoor(data, inst, td, inst.witness, r, s_)
    assert key.info()["terms"] == model_key.info()["terms"] and key.info()["resident_bytes"] == model_key.info()["resident_bytes"]
    key.close()
    model_key.close()


# ---- refusals: NLX_E_RANGE with the cause named, nothing left allocated ----
def _refused(nlx, g16, ctx, inst, td, needle, code=E_RANGE, r1cs=None, commitments=None, **sizes):
    kw = dict(log_n=inst.log_n, n_wires=inst.n_wires, n_public=inst.n_public, n_constraints=inst.n_constraints)
    kw.update(sizes)
    before = ctx.memory()[1]
    with pytest.raises(nlx.NlxError) as e:
        g16.Setup(ctx, kw["log_n"], kw["n_wires"], kw["n_public"], kw["n_constraints"], r1cs or gc.r1cs_arrays(np, g16.fr_pack, inst), td, commitments)
    assert e.value.code == code and needle in str(e.value), str(e.value)
    assert ctx.memory()[1] == before


def test_trapdoor_refusals(nlx, ctx, g16):
    inst, td, _, _ = _model("public3-13")
    good = dict(tau=td.tau, alpha=td.alpha, beta=td.beta, gamma=td.gamma, delta=td.delta)
    for name in good:
        for value, needle in ((0, "%s is zero" % name), (R, "%s is not below r" % name), ((1 << 256) - 1, "%s is not below r" % name)):
            _refused(nlx, g16, ctx, inst, g16.Trapdoor(**dict(good, **{name: value})), needle)
    for tau in (1, bn.root_of_unity(inst.log_n), pow(bn.root_of_unity(inst.log_n), 5, R)):
        _refused(nlx, g16, ctx, inst, g16.Trapdoor(**dict(good, tau=tau)), "tau^(2^log_n) = 1")
    # tau in a larger domain only is fine
    s = g16.Setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, gc.r1cs_arrays(np, g16.fr_pack, inst),
                  g16.Trapdoor(**dict(good, tau=bn.root_of_unity(inst.log_n + 1))))
    s.close()
    cinst, ctd, _, _ = _model(gc.COMMITTED_NAMES[0])
    cgood = dict(tau=ctd.tau, alpha=ctd.alpha, beta=ctd.beta, gamma=ctd.gamma, delta=ctd.delta)
    for value, needle in ((0, "sigma is zero"), (R + 1, "sigma is not below r")):
        _refused(nlx, g16, ctx, cinst, g16.Trapdoor(sigma=value, **cgood), needle, commitments=_commitments(cinst))


def test_size_and_id_refusals(nlx, ctx, g16):
    inst, td, _, _ = _model("public3-13")
    t = _trapdoor(g16, td)
    _refused(nlx, g16, ctx, inst, t, "log_n", log_n=0)
    _refused(nlx, g16, ctx, inst, t, "log_n", log_n=27)
    _refused(nlx, g16, ctx, inst, t, "n_constraints exceeds", log_n=3)
    _refused(nlx, g16, ctx, inst, t, "n_public", n_public=0)
    _refused(nlx, g16, ctx, inst, t, "n_public", n_public=inst.n_wires + 1)
    _refused(nlx, g16, ctx, inst, t, "wire", n_wires=inst.n_wires - 1)                      # the last wire's id is now out of range

    def r1cs(edit):
        out = gc.r1cs_arrays(np, g16.fr_pack, inst)
        edit(out)
        return out

    def bad_coeff_id(o):
        o["B"][2][0] = len(inst.coeffs)

    def decreasing(o):
        o["C"][0][3] = o["C"][0][4] + 1

    def not_from_zero(o):
        o["A"][0][0] = 1

    def coeff_not_below_r(o):
        o["coeffs"][1] = [(R >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]
    _refused(nlx, g16, ctx, inst, t, "coefficient %d of %d" % (len(inst.coeffs), len(inst.coeffs)), r1cs=r1cs(bad_coeff_id))
    _refused(nlx, g16, ctx, inst, t, "row pointers decrease at row 3", r1cs=r1cs(decreasing))
    _refused(nlx, g16, ctx, inst, t, "do not start at 0", r1cs=r1cs(not_from_zero))
    _refused(nlx, g16, ctx, inst, t, "coefficient 1 is not below r", r1cs=r1cs(coeff_not_below_r))
    before = ctx.memory()[1]
    with pytest.raises(nlx.NlxError) as e:
        g16.Setup(ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, gc.r1cs_arrays(np, g16.fr_pack, inst), t, flags=0)
    assert e.value.code == E_RANGE and "flags" in str(e.value) and ctx.memory()[1] == before


def test_commitment_refusals(nlx, ctx, g16):
    inst, td, _, _ = _model(gc.COMMITTED_NAMES[2])                       # k = 3
    t = _trapdoor(g16, td)
    base = _commitments(inst)
    free = [i for i in range(inst.n_public, inst.n_wires) if all(i != c["wire"] and i not in c["private"] for c in base)]

    def edited(j, **kw):
        out = [dict(c) for c in base]
        out[j].update(kw)
        return out
    _refused(nlx, g16, ctx, inst, t, "is not a private wire", commitments=edited(0, private=[0]))
    _refused(nlx, g16, ctx, inst, t, "is not a private wire", commitments=edited(0, private=[inst.n_wires]))
    _refused(nlx, g16, ctx, inst, t, "do not ascend", commitments=edited(1, private=[free[1], free[0]]))
    _refused(nlx, g16, ctx, inst, t, "committed twice", commitments=edited(0, private=[base[1]["private"][0]]))
    _refused(nlx, g16, ctx, inst, t, "committed or listed twice", commitments=edited(2, wire=base[1]["private"][0]))
    _refused(nlx, g16, ctx, inst, t, "committed or listed twice", commitments=edited(2, wire=base[0]["wire"]))
    _refused(nlx, g16, ctx, inst, t, "its wire 0 is not a private wire", commitments=edited(2, wire=0))
    _refused(nlx, g16, ctx, inst, t, "commitments", commitments=[dict(private=[], public=[0], wire=free[i]) for i in range(9)])
    _refused(nlx, g16, ctx, inst, t, "more committed and commitment wires than private wires",
             commitments=edited(0, private=list(range(inst.n_public, inst.n_wires))))
