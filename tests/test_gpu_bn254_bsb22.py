"""GPU: Bsb22 commitments in the gnark-shaped PLONK proof over BN254 - the quotient chain with NLX_BN254_PLONK_COMMIT
(nlx_bn254_plonk_quotient; csrc/bn254_plonk.hip) and whole proofs (near-light-client_amd/bn254_plonk.py prove_gnark on a key with
commitments) - against the big-integer model tools/gnark_bsb22_model.py, which states the protocol's rules (recalled from gnark,
unpinned: DESIGN.md section 18) and is tied to the frozen model oracle/bn254_py.py where there is no commitment."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bsb22_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu

bn = gm.bn
R = gm.R
NLX_E_INVAL, NLX_E_RANGE = -1, -4


def _pack(nlx, values):
    return nlx.bn254_pack([[bn.to_montgomery(v) for v in values]])[0]


def _ints(nlx, words):
    return [bn.from_montgomery(x) for x in nlx.bn254_unpack(np.ascontiguousarray(words).reshape(1, -1, 4))[0]]


def _quotient_case(log_n, k, seed, blinded):
    """a satisfying instance with its solved witness, z under random challenges, and the model's quotient"""
    rng = random.Random(seed)
    n_pi = 0 if (1 << log_n) < 2 * k + 3 else 2
    inst = gm.Instance(log_n, k, rng, n_pi=n_pi)
    n = inst.n
    tau = rng.randrange(1, R)
    (l, r, o), pi2, pi2_co, _, cs = gm.solve(inst, None, [rng.randrange(R) for _ in range(2 * k)], tau=tau)
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    z = gm.grand_product(l, r, o, inst.fixed, n, beta, gamma, inst.k1, inst.k2)
    pi = list(inst.public_inputs) + [0] * (n - n_pi)
    for j in range(k):
        pi[inst.commit_rows[j]] = cs[j]
    on_h = dict(inst.fixed, l=l, r=r, o=o, z=z, pi=pi)
    co = {name: bn.ntt(v, inverse=True) for name, v in on_h.items()}
    b = [rng.randrange(R) for _ in range(9)] if blinded else None
    if blinded:
        co.update(l=bn.blind_coeffs(co["l"], n, b[0:2]), r=bn.blind_coeffs(co["r"], n, b[2:4]), o=bn.blind_coeffs(co["o"], n, b[4:6]),
                  z=bn.blind_coeffs(co["z"], n, b[6:9]))
    for j in range(k):
        co["qcp%d" % j], co["pi2%d" % j] = bn.ntt(inst.qcp[j], inverse=True), pi2_co[j]
    want = gm.quotient(co, n, 5, inst.k1, inst.k2, alpha, beta, gamma, k)
    return inst, on_h, pi2, b, (alpha, beta, gamma), want


@pytest.mark.parametrize("blinded", [False, True])
@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_quotient_chain_with_commitments_equals_model(nlx, ctx, k, log_n, blinded):
    inst, on_h, pi2, b, (alpha, beta, gamma), want = _quotient_case(log_n, k, 7000 + 100 * k + 10 * log_n + blinded, blinded)
    n = inst.n
    keep = 3 * n + 6 if blinded else 3 * n
    assert not any(want[keep:]) and any(want[2 * n:keep])
    packed = {name: _pack(nlx, v) for name, v in on_h.items()}
    qcp = [_pack(nlx, q) for q in inst.qcp]
    p2 = [_pack(nlx, v) for v in pi2]
    sc = [bn.to_montgomery(x) for x in (5, inst.k1, inst.k2, alpha, beta, gamma)]
    blinding = [bn.to_montgomery(x) for x in b] if blinded else None
    t, ok = nlx.bn254_plonk_quotient(ctx, packed, *sc, blinding=blinding, qcp=qcp, pi2=p2)
    assert ok
    assert _ints(nlx, t) == (want if blinded else want[:3 * n])
    # the same from device-resident polynomials
    import torch
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    t2, ok2 = nlx.bn254_plonk_quotient(ctx, {name: dev(v) for name, v in packed.items()}, *sc, blinding=blinding,
                                       qcp=[dev(v) for v in qcp], pi2=[dev(v) for v in p2])
    assert ok2 and np.array_equal(t2, t)
    # one pi2 entry on a committed row changed: the rows no longer close, and the high chunk says so
    j = k - 1
    row = inst.committed[j][0]
    broken = list(pi2[j])
    broken[row] = (broken[row] + 1) % R
    p2_bad = list(p2)
    p2_bad[j] = _pack(nlx, broken)
    _, ok3 = nlx.bn254_plonk_quotient(ctx, packed, *sc, blinding=blinding, qcp=qcp, pi2=p2_bad)
    assert not ok3
    # and without the commitment term the same witness does not satisfy the gates either
    assert not nlx.bn254_plonk_quotient(ctx, packed, *sc, blinding=blinding)[1]


def _key(nlx, ctx, inst, srs_pts):
    return nlx.bn254_plonk.ProvingKey(ctx, inst.key_values(), nlx.bn254_g1_pack(srs_pts), inst.k1, inst.k2, commitments=inst.commitment_info())


@pytest.mark.parametrize("n_pi", [0, 3])
@pytest.mark.parametrize("log_n", [4, 6, 8, 10])
@pytest.mark.parametrize("k", [1, 2])
def test_proof_with_commitments_equals_model_bytes_and_verifies(nlx, ctx, k, log_n, n_pi):
    """k = 2 is a chain: a committed row of commitment 1 is copy-constrained to c_0, so the witness can only be completed between
    the commitments"""
    rng = random.Random(8000 + 100 * k + 10 * log_n + n_pi)
    inst = gm.Instance(log_n, k, rng, n_pi=n_pi, chain=True)
    n, pubs = inst.n, inst.public_inputs
    tau = rng.randrange(1, R)
    srs_pts = bn.kzg_srs(tau, n + 3)
    blind = [rng.randrange(R) for _ in range(9)]
    cblind = [rng.randrange(R) for _ in range(2 * k)]
    model, want = gm.prove(inst, srs_pts, blind, cblind, tau=tau)
    P = nlx.bn254_plonk
    pk = _key(nlx, ctx, inst, srs_pts)
    vk = gm.verifying_key(inst, srs_pts, tau)
    assert [nlx.bn254_g1_unpack(c) for c in pk.qcp_commitments] == vk["qcp"]
    assert {name: nlx.bn254_g1_unpack(pk.commitments[name]) for name in pk.NAMES} == {name: vk[name] for name in pk.NAMES}
    calls = []

    def witness(cs):
        calls.append(list(cs))
        return inst.complete(cs)
    got = P.prove_gnark(pk, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=witness)
    assert calls == [model["c"][:j] for j in range(k + 1)]
    assert len(got) == len(want) == 7 * 32 + 4 + 32 * k + 32 + 4 + 32 * (7 + k) + 64
    assert got == want
    verify = lambda data, pi=pubs: gm.verify_trapdoor(data, vk, n, tau, inst.k1, inst.k2, pi)
    assert verify(got)
    # the full-wires form, for a caller that knows every c_j already: the same bytes
    l, r, o = inst.complete(model["c"])
    assert P.prove_gnark(pk, l, r, o, pubs, blind, cblind) == got
    # random blinding (of the wires and of the commitments): other bytes, other c_j, the same verdict
    other = P.prove_gnark(pk, public_inputs=pubs, witness=inst.complete)
    assert other != got and other[224:228] == got[224:228] and verify(other)
    assert not verify(got, [(pubs[0] + 1) % R] + pubs[1:] if n_pi else [1])
    bad = bytearray(got)
    bad[gm.proof_regions(k)["bsb22_%d" % (k - 1)][0] + 31] ^= 1
    assert not verify(bytes(bad))
    if log_n > 6:
        return
    # a committed value changed after the commitment
    row = inst.committed[0][0]

    def changed(cs):
        l2, r2, o2 = inst.complete(cs)
        if len(cs) == k:
            l2 = list(l2)
            l2[row] = (l2[row] + 1) % R
        return l2, r2, o2
    with pytest.raises(ValueError):
        P.prove_gnark(pk, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=changed)
    # full wires whose commitment row does not hold the hash (the c_j of OTHER blinding scalars)
    with pytest.raises(ValueError):
        P.prove_gnark(pk, l, r, o, pubs, blind, [x + 1 for x in cblind])
    # a broken ordinary gate is still refused by the quotient's high chunk / the grand product
    bad_o = list(o)
    free_row = next(i for i in range(n) if inst.fixed["qo"][i])
    bad_o[free_row] = (bad_o[free_row] + 1) % R
    with pytest.raises(ValueError):
        P.prove_gnark(pk, l, r, bad_o, pubs, blind, cblind)
    with pytest.raises(ValueError):
        P.prove_gnark(pk, l, r, o, pubs, blind, cblind[:-1])                # 2 k scalars
    with pytest.raises(ValueError):
        P.prove_gnark(pk, l, r, o, pubs, blind, cblind, witness=witness)     # wires or a callable, not both


@pytest.mark.parametrize("log_n,n_pi", [(3, 0), (4, 2), (6, 3)])
def test_a_key_without_commitments_gives_the_frozen_models_bytes(nlx, ctx, log_n, n_pi):
    """nothing moved: the existing assertion of tests/test_gpu_bn254_plonk.py, through the new parameters"""
    rng = random.Random(9000 + log_n)
    inst = gm.Instance(log_n, 0, rng, n_pi=n_pi)
    n, pubs = inst.n, inst.public_inputs
    tau = rng.randrange(1, R)
    srs_pts = bn.kzg_srs(tau, n + 3)
    blind = [rng.randrange(R) for _ in range(9)]
    l, r, o = inst.complete([])
    _, want = bn.gnark_plonk_prove_model(dict(inst.fixed, l=l, r=r, o=o), srs_pts, inst.k1, inst.k2, pubs, blind)
    P = nlx.bn254_plonk
    for pk in (P.ProvingKey(ctx, inst.fixed, nlx.bn254_g1_pack(srs_pts), inst.k1, inst.k2),
               P.ProvingKey(ctx, inst.key_values(), nlx.bn254_g1_pack(srs_pts), inst.k1, inst.k2, commitments=[])):
        assert pk.qcp_commitments == [] and pk.bsb22 == []
        assert P.prove_gnark(pk, l, r, o, pubs, blind) == want
        assert P.prove_gnark(pk, l, r, o, pubs, blind, commit_blinding=[]) == want
        assert P.prove_gnark(pk, public_inputs=pubs, blinding=blind, commit_blinding=None, witness=inst.complete) == want
    vk = {name: nlx.bn254_g1_unpack(pk.commitments[name]) for name in pk.NAMES}
    assert bn.gnark_plonk_verify_trapdoor(want, vk, n, tau, inst.k1, inst.k2, pubs)
    assert len(want) == gm.proof_length(0) == 552


def _raw_quotient(nlx, ctx, packed, sc_words, flags, n_commit, qcp, pi2, out, blinding=None):
    """nlx_bn254_plonk_quotient with every field of the struct set by hand -> (return code, high_chunk_is_zero)"""
    args = nlx.batch._PlonkQuotientArgs()
    for name in ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z", "pi"):
        if name in packed:
            setattr(args, name, packed[name].ctypes.data)
    args.log_n = packed["l"].shape[0].bit_length() - 1
    args.flags = flags
    for name, w in zip(("coset_shift", "k1", "k2", "alpha", "beta", "gamma"), sc_words):
        setattr(args, name, w.ctypes.data)
    if blinding is not None:
        args.blinding = blinding.ctypes.data
    args.n_commit = n_commit
    args.qcp, args.pi2 = qcp, pi2
    ok = ctypes.c_int32(-7)
    rc = nlx.batch.dll.nlx_bn254_plonk_quotient(ctx.handle, ctypes.byref(args), out.ctypes.data, ctypes.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("blinded", [False, True])
def test_with_the_flag_clear_the_new_fields_are_not_read(nlx, ctx, blinded):
    """a caller compiled against the earlier struct leaves whatever lies behind it in n_commit, qcp, pi2"""
    log_n = 5
    rng = random.Random(31 + blinded)
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    p = bn.plonk_witness(log_n, rng, 5, 25, beta, gamma)
    n = 1 << log_n
    packed = {name: _pack(nlx, v) for name, v in p.items()}
    sc = [bn.to_montgomery(x) for x in (5, 5, 25, alpha, beta, gamma)]
    b = [bn.to_montgomery(rng.randrange(R)) for _ in range(9)] if blinded else None
    want, ok = nlx.bn254_plonk_quotient(ctx, packed, *sc, blinding=b)
    assert ok
    if not blinded:
        assert _ints(nlx, want) == bn.plonk_quotient(p, 5, 5, 25, alpha, beta, gamma)[:3 * n]
    sc_words = [nlx.batch._fr_words(x) for x in sc]
    bw = np.stack([nlx.batch._fr_words(x) for x in b]) if blinded else None
    junk = ctypes.cast(ctypes.c_void_p(0x10), ctypes.POINTER(ctypes.c_void_p))      # never a valid address: must not be read
    for n_commit in (0, 3, 0xDEADBEEF):
        out = np.zeros_like(want)
        rc, high = _raw_quotient(nlx, ctx, packed, sc_words, 1 | (0x100 if blinded else 0), n_commit, junk, junk, out, bw)
        assert rc == 0 and high == 1
        assert np.array_equal(out, want)


def test_refusals_with_the_commit_flag(nlx, ctx):
    inst, on_h, pi2, _, (alpha, beta, gamma), want = _quotient_case(4, 2, 77, False)
    n = inst.n
    packed = {name: _pack(nlx, v) for name, v in on_h.items()}
    qcp = [_pack(nlx, q) for q in inst.qcp]
    p2 = [_pack(nlx, v) for v in pi2]
    sc = [bn.to_montgomery(x) for x in (5, inst.k1, inst.k2, alpha, beta, gamma)]

    def refused(code, **kw):
        with pytest.raises(nlx.NlxError) as ei:
            nlx.bn254_plonk_quotient(ctx, packed, *sc, **kw)
        assert ei.value.code == code, kw.keys()
    refused(NLX_E_RANGE, qcp=[], pi2=[])                                       # n_commit = 0
    refused(NLX_E_RANGE, qcp=[qcp[0]] * 5, pi2=[p2[0]] * 5)                    # n_commit = 5
    refused(NLX_E_INVAL, qcp=[qcp[0], None], pi2=p2)                           # a NULL entry
    refused(NLX_E_INVAL, qcp=qcp, pi2=[None, p2[1]])
    with pytest.raises(ValueError):
        nlx.bn254_plonk_quotient(ctx, packed, *sc, qcp=qcp, pi2=p2[:1])
    # NULL arrays
    sc_words = [nlx.batch._fr_words(x) for x in sc]
    arr = (ctypes.c_void_p * 2)(qcp[0].ctypes.data, qcp[1].ctypes.data)
    null = ctypes.POINTER(ctypes.c_void_p)()
    out = np.zeros((3, n, 4), dtype=np.uint64)
    assert _raw_quotient(nlx, ctx, packed, sc_words, 1 | 0x200, 2, null, arr, out)[0] == NLX_E_INVAL
    assert _raw_quotient(nlx, ctx, packed, sc_words, 1 | 0x200, 2, arr, null, out)[0] == NLX_E_INVAL
    assert _raw_quotient(nlx, ctx, packed, sc_words, 1 | 0x400, 2, arr, arr, out)[0] not in (0, NLX_E_INVAL, NLX_E_RANGE)   # an unknown flag: unsupported
    # the context works afterwards
    t, ok = nlx.bn254_plonk_quotient(ctx, packed, *sc, qcp=qcp, pi2=p2)
    assert ok and _ints(nlx, t) == want[:3 * n]
