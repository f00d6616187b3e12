"""GPU: whole gnark-shaped PLONK proofs over BN254 from a key resident in HBM (nlx_bn254_plonk_key_create / _commit / _prove,
nlx_bn254_fr_eval_many; csrc/bn254_plonk_prove.hip, near-light-client_amd/bn254_plonk.py ResidentKey / prove_resident) against
the two models that pin prove_gnark: the frozen oracle/bn254_py.py gnark_plonk_prove_model / gnark_plonk_verify_trapdoor and
tools/gnark_bsb22_model.py.  Parity with gnark-produced bytes stays unpinned."""
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


def _mont_words(nlx, values):
    return nlx.bn254_pack([[bn.to_montgomery(v) for v in values]])[0]


def _plain_instance(log_n, n_pi, seed):
    """the instance of tests/test_gpu_bn254_plonk.py's byte test: a satisfying witness, public inputs moved out of qk"""
    rng = random.Random(seed)
    p = bn.plonk_witness(log_n, rng, 5, 25, 11, 13)
    p.pop("z")
    tau = rng.randrange(1, R)
    pis = [rng.randrange(R) for _ in range(n_pi)]
    p["qk"] = [(a - (pis[i] if i < n_pi else 0)) % R for i, a in enumerate(p["qk"])]
    blind = [rng.randrange(R) for _ in range(9)]
    return p, tau, pis, blind


@pytest.mark.parametrize("log_n,n_pi", [(3, 0), (4, 2), (6, 3), (8, 1), (10, 5)])
def test_bytes_without_commitments_equal_models(nlx, ctx, log_n, n_pi):
    n = 1 << log_n
    p, tau, pis, blind = _plain_instance(log_n, n_pi, 190 + log_n)
    srs_pts = _power_srs(tau, n + 3)
    srs = nlx.bn254_g1_pack(srs_pts)
    _, want = bn.gnark_plonk_prove_model(p, srs_pts, 5, 25, pis, blind)
    P = nlx.bn254_plonk
    pk = P.ProvingKey(ctx, p, srs, 5, 25)
    assert P.prove_gnark(pk, p["l"], p["r"], p["o"], pis, blind) == want
    vk = {k: nlx.bn254_g1_unpack(pk.commitments[k]) for k in pk.NAMES}
    verify = lambda data, pi=pis: bn.gnark_plonk_verify_trapdoor(data, vk, n, tau, 5, 25, pi)
    proofs = []
    for coset in (False, True):
        key = P.ResidentKey(ctx, p, srs, 5, 25, coset=coset)
        assert key.proof_bytes == 552
        got = P.prove_resident(key, p["l"], p["r"], p["o"], pis, blind)
        assert len(got) == 552 and got == want, coset
        proofs.append(got)
        other = P.prove_resident(key, p["l"], p["r"], p["o"], pis)          # random blinding: other bytes, the same verdict
        assert other != got and len(other) == 552 and verify(other)
        key.close()
    assert verify(want)
    if n_pi:
        assert not verify(want, [(pis[0] + 1) % R] + pis[1:])
    bad = bytearray(want)
    bad[-1] ^= 1
    assert not verify(bytes(bad))
    assert proofs[0] == proofs[1]
    # wires as (n, 4) device tensors of fr.Element words
    import torch
    key = P.ResidentKey(ctx, p, srs, 5, 25)
    dev = [torch.from_numpy(_mont_words(nlx, p[c]).view(np.int64)).cuda() for c in "lro"]
    assert P.prove_resident(key, dev[0], dev[1], dev[2], pis, blind) == want
    key.close()


def _keys(nlx, ctx, inst, srs, coset):
    return nlx.bn254_plonk.ResidentKey(ctx, inst.key_values(), srs, inst.k1, inst.k2, commitments=inst.commitment_info(), coset=coset)


def _commit_case(nlx, ctx, k, log_n, n_pi):
    rng = random.Random(18000 + 100 * k + 10 * log_n + n_pi)
    inst = gm.Instance(log_n, k, rng, n_pi=n_pi, chain=True)
    n, pubs = inst.n, inst.public_inputs
    tau = rng.randrange(1, R)
    srs_pts = bn.kzg_srs(tau, n + 3)
    blind = [rng.randrange(R) for _ in range(9)]
    cblind = [rng.randrange(R) for _ in range(2 * k)]
    model, want = gm.prove(inst, srs_pts, blind, cblind, tau=tau)
    assert len(want) == 552 + 64 * k
    P = nlx.bn254_plonk
    srs = nlx.bn254_g1_pack(srs_pts)
    vk = gm.verifying_key(inst, srs_pts, tau)
    verify = lambda data, pi=pubs: gm.verify_trapdoor(data, vk, n, tau, inst.k1, inst.k2, pi)
    for coset in (False, True):
        key = _keys(nlx, ctx, inst, srs, coset)
        assert key.proof_bytes == 552 + 64 * k
        # the hint, driven by hand: c_j from the wires as far as they are solved
        cs = []
        for j in range(k):
            point, c = P.commit_resident(key, j, inst.complete(cs)[0], cblind[2 * j:2 * j + 2])
            assert c == model["c"][j] == gm.hash_to_field(P.g1_marshal(point))
            cs.append(c)
        calls = []

        def witness(cs):
            calls.append(list(cs))
            return inst.complete(cs)
        got = P.prove_resident(key, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=witness)
        assert calls == [model["c"][:j] for j in range(k + 1)]
        assert got == want, coset
        assert verify(got)
        l, r, o = inst.complete(model["c"])
        assert P.prove_resident(key, l, r, o, pubs, blind, cblind) == got       # the full-wires form
        if not coset:
            other = P.prove_resident(key, public_inputs=pubs, witness=inst.complete)
            assert other != got and len(other) == len(got) and verify(other)
            assert not verify(got, [(pubs[0] + 1) % R] + pubs[1:] if n_pi else [1])
        key.close()
    return inst, srs, pubs, blind, cblind, model, want


@pytest.mark.parametrize("n_pi", [0, 3])
@pytest.mark.parametrize("log_n", [4, 6, 8])
@pytest.mark.parametrize("k", [1, 2])
def test_bytes_with_commitments_equal_model(nlx, ctx, k, log_n, n_pi):
    _commit_case(nlx, ctx, k, log_n, n_pi)


def test_bytes_with_four_commitments(nlx, ctx):
    """k = 4 at log_n = 6: Instance builds that shape (64 rows hold 4 commitment rows and their sets)"""
    _commit_case(nlx, ctx, 4, 6, 3)


_G_TABLE = []    # [window][byte] * 256^window * G, built on first use


def _power_srs(tau, size):
    """bn.kzg_srs(tau, size) - the points tau^i G - through a fixed-base table of G (byte windows, mixed Jacobian additions from
    the model's own group law): a second of big-integer work at 2^12 where one double-and-add per point takes eleven"""
    if size <= 128:
        return bn.kzg_srs(tau, size)
    table, base = _G_TABLE, bn.G1
    while len(table) < 32:
        row, acc = [None], None
        for _ in range(255):
            acc = bn.g1_add(acc, base)
            row.append(acc)
        table.append(row)
        base = bn.g1_add(acc, base)        # 256 * base
    out, x = [], 1
    for _ in range(size):
        acc = (1, 1, 0)
        for w in range(32):
            d = (x >> (8 * w)) & 0xFF
            if d:
                acc = bn._jac_add_affine(acc, table[w][d])
        zi = pow(acc[2], bn.Q - 2, bn.Q)
        out.append((acc[0] * zi * zi % bn.Q, acc[1] * zi * zi * zi % bn.Q))
        x = x * tau % R
    return out


@pytest.fixture(scope="module")
def srs_4099():
    tau = random.Random(1200).randrange(1, R)
    pts = _power_srs(tau, (1 << 12) + 3)
    assert pts[:3] + pts[-1:] == bn.kzg_srs(tau, 3) + [bn.g1_mul(pow(tau, (1 << 12) + 2, R), bn.G1)]
    return tau, pts


@pytest.mark.parametrize("k", [0, 1])
def test_one_size_past_the_models(nlx, ctx, srs_4099, k):
    """log_n = 12: the first size where MSM, scan and NTT all run more than one block per stage.  No big-integer prover here:
    prove_gnark (pinned up to 2^10) is the reference for the bytes, the model's trapdoor verifier the judge."""
    log_n, n_pi = 12, 2
    rng = random.Random(1200 + k)
    inst = gm.Instance(log_n, k, rng, n_pi=n_pi, chain=True)
    n, pubs = inst.n, inst.public_inputs
    tau, srs_pts = srs_4099
    srs = nlx.bn254_g1_pack(srs_pts)
    blind = [rng.randrange(R) for _ in range(9)]
    cblind = [rng.randrange(R) for _ in range(2 * k)]
    P = nlx.bn254_plonk
    pk = P.ProvingKey(ctx, inst.key_values(), srs, inst.k1, inst.k2, commitments=inst.commitment_info())
    want = P.prove_gnark(pk, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=inst.complete)
    for coset in (False, True):
        key = _keys(nlx, ctx, inst, srs, coset)
        assert P.prove_resident(key, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=inst.complete) == want
        key.close()
    vk = {name: nlx.bn254_g1_unpack(pk.commitments[name]) for name in pk.NAMES}
    vk["qcp"] = [nlx.bn254_g1_unpack(c) for c in pk.qcp_commitments]
    vk["commit_rows"] = list(inst.commit_rows)
    assert gm.verify_trapdoor(want, vk, n, tau, inst.k1, inst.k2, pubs)
    assert not gm.verify_trapdoor(want, vk, n, tau, inst.k1, inst.k2, [(pubs[0] + 1) % R] + pubs[1:])


@pytest.mark.parametrize("k", [0, 2])
def test_key_commitments_and_resident_bytes(nlx, ctx, k):
    log_n = 5
    rng = random.Random(50 + k)
    inst = gm.Instance(log_n, k, rng, n_pi=1)
    n = inst.n
    srs = nlx.bn254_g1_pack(bn.kzg_srs(rng.randrange(1, R), n + 3))
    P = nlx.bn254_plonk
    pk = P.ProvingKey(ctx, inst.key_values(), srs, inst.k1, inst.k2, commitments=inst.commitment_info())
    plain, with_coset = _keys(nlx, ctx, inst, srs, False), _keys(nlx, ctx, inst, srs, True)
    want = [pk.commitments[name] for name in ("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk")] + list(pk.qcp_commitments)
    for key in (plain, with_coset):
        got = key.key_commitments()
        assert got.shape == (8 + k, 8)
        for a, b in zip(got, want):
            assert nlx.bn254_g1_unpack(a) == nlx.bn254_g1_unpack(b)
    a, b = plain.info(), with_coset.info()
    assert (a["n"], a["k"], a["coset"]) == (n, k, False) and (b["n"], b["k"], b["coset"]) == (n, k, True)
    assert a["committed_rows"] == b["committed_rows"] == sum(len(c) for c in inst.committed)
    assert b["resident_bytes"] - a["resident_bytes"] == (8 + k) * 4 * n * 32
    plain.close()
    with_coset.close()


# ---- eval_many ----
EVAL_LENGTHS = [2, 3, 63, 64, 65, 4096, 4097, 8197, (1 << 15) + 321]


@pytest.fixture(scope="module")
def eval_pool():
    """one pool of random coefficients, shared and left unchanged: polynomial i of length m is pool[i : i + m]"""
    rng = random.Random(77)
    return [rng.randrange(R) for _ in range((1 << 15) + 321 + 3 + 16)]


@pytest.fixture(scope="module")
def eval_words(nlx, eval_pool):
    return _mont_words(nlx, eval_pool)


def _horner(coeffs, z):
    if z in (0, 1):
        return coeffs[0] if z == 0 else sum(coeffs) % R
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


@pytest.mark.parametrize("m", EVAL_LENGTHS)
def test_eval_many_equals_horner_and_kzg_open(nlx, ctx, eval_pool, eval_words, m):
    import torch
    P = nlx.bn254_plonk
    rng = random.Random(m)
    for count in (1, 7, 11, 16):
        # ragged: m, m + 2, m + 3 in one call, each from its own offset of the pool
        shapes = [(i, m + (0, 2, 3)[i % 3]) for i in range(count)]
        host = [eval_words[i:i + length] for i, length in shapes]
        polys = [torch.from_numpy(np.ascontiguousarray(h).view(np.int64)).cuda() if i % 2 else np.ascontiguousarray(h) for i, h in enumerate(host)]
        for z in (0, 1, rng.randrange(R)):
            got = P.eval_many(ctx, polys, z)
            assert got == [_horner(eval_pool[i:i + length], z) for i, length in shapes], (count, z)
    z = rng.randrange(R)
    y = nlx.bn254_kzg_open(ctx, np.ascontiguousarray(eval_words[:m]), bn.to_montgomery(z), want_quotient=False)[0]
    assert P.eval_many(ctx, [np.ascontiguousarray(eval_words[:m])], z) == [bn.from_montgomery(nlx.bn254_unpack(y[None, None, :])[0][0])]


def test_eval_many_refusals(nlx, ctx, eval_words):
    P = nlx.bn254_plonk
    one = np.ascontiguousarray(eval_words[:5])
    with pytest.raises(nlx.NlxError) as ei:
        P.eval_many(ctx, [one] * 17, 3)
    assert ei.value.code == NLX_E_RANGE
    with pytest.raises(nlx.NlxError) as ei:
        P.eval_many(ctx, [], 3)
    assert ei.value.code == NLX_E_RANGE
    assert P.eval_many(ctx, [one] * 16, 1) == [sum(bn.from_montgomery(x) for x in nlx.bn254_unpack(one[None])[0]) % R] * 16


# ---- refusals ----
def _raw_prove(nlx, ctx, key, wires, pubs, blind, cblind, cap=None):
    """nlx_bn254_plonk_prove by hand -> (return code, the output buffer, the length written)"""
    B = nlx.batch
    words = lambda xs: np.stack([B._fr_words(bn.to_montgomery(x)) for x in xs]) if len(xs) else None
    w = [_mont_words(nlx, c) for c in wires]
    pw, bw, cw = words(pubs), words(blind), words(cblind) if cblind is not None else None
    cap = key.proof_bytes if cap is None else cap
    out = np.full(key.proof_bytes + 8, 0xA5, dtype=np.uint8)
    got = ctypes.c_size_t(12345)
    rc = nlx.lib.dll.nlx_bn254_plonk_prove(ctx.handle, key.handle, w[0].ctypes.data, w[1].ctypes.data, w[2].ctypes.data,
                                           pw.ctypes.data if pw is not None else None, len(pubs), bw.ctypes.data,
                                           cw.ctypes.data if cw is not None else None, out.ctypes.data, cap, ctypes.byref(got))
    return rc, out, got.value


def test_refusals(nlx, ctx):
    log_n, k = 4, 2
    rng = random.Random(404)
    inst = gm.Instance(log_n, k, rng, n_pi=2, chain=True)
    n, pubs = inst.n, inst.public_inputs
    tau = rng.randrange(1, R)
    srs_pts = bn.kzg_srs(tau, n + 3)
    srs = nlx.bn254_g1_pack(srs_pts)
    blind = [rng.randrange(R) for _ in range(9)]
    cblind = [rng.randrange(R) for _ in range(2 * k)]
    model, want = gm.prove(inst, srs_pts, blind, cblind, tau=tau)
    P = nlx.bn254_plonk
    key = _keys(nlx, ctx, inst, srs, False)
    l, r, o = inst.complete(model["c"])
    untouched = lambda out: bool((out == 0xA5).all())
    last = lambda: nlx.lib.dll.nlx_last_error(ctx.handle).decode()
    rc, out, length = _raw_prove(nlx, ctx, key, (l, r, o), pubs, blind, cblind)
    assert rc == 0 and length == len(want) and out[:length].tobytes() == want and untouched(out[length:])
    # a broken gate
    bad_o = list(o)
    free_row = next(i for i in range(n) if inst.fixed["qo"][i])
    bad_o[free_row] = (bad_o[free_row] + 1) % R
    rc, out, _ = _raw_prove(nlx, ctx, key, (l, r, bad_o), pubs, blind, cblind)
    assert rc == NLX_E_INVAL and untouched(out) and last()
    with pytest.raises(ValueError):
        P.prove_resident(key, l, r, bad_o, pubs, blind, cblind)
    # a committed value changed after the hint
    row = inst.committed[0][0]
    bad_l = list(l)
    bad_l[row] = (bad_l[row] + 1) % R
    rc, out, _ = _raw_prove(nlx, ctx, key, (bad_l, r, o), pubs, blind, cblind)
    assert rc == NLX_E_INVAL and untouched(out) and "commitment" in last()

    def changed(cs):
        l2, r2, o2 = inst.complete(cs)
        if len(cs) == k:
            l2 = list(l2)
            l2[row] = (l2[row] + 1) % R
        return l2, r2, o2
    with pytest.raises(ValueError):
        P.prove_resident(key, public_inputs=pubs, blinding=blind, commit_blinding=cblind, witness=changed)
    # a commitment row holding another blinding's c_j
    other = [x + 1 for x in cblind]
    rc, out, _ = _raw_prove(nlx, ctx, key, (l, r, o), pubs, blind, other)
    assert rc == NLX_E_INVAL and untouched(out) and "commitment" in last()
    with pytest.raises(ValueError):
        P.prove_resident(key, l, r, o, pubs, blind, other)
    # commit_blinding of the wrong length; wires and a callable
    with pytest.raises(ValueError):
        P.prove_resident(key, l, r, o, pubs, blind, cblind[:-1])
    with pytest.raises(ValueError):
        P.prove_resident(key, l, r, o, pubs, blind, cblind, witness=inst.complete)
    assert _raw_prove(nlx, ctx, key, (l, r, o), pubs, blind, None)[0] == NLX_E_INVAL          # k = 2 and no commit_blinding
    # proof_cap one byte short
    rc, out, _ = _raw_prove(nlx, ctx, key, (l, r, o), pubs, blind, cblind, cap=len(want) - 1)
    assert rc == NLX_E_RANGE and untouched(out)
    # the hint: j >= k
    b2 = np.stack([nlx.batch._fr_words(1), nlx.batch._fr_words(2)])
    lw = _mont_words(nlx, l)
    pt, c = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    assert nlx.lib.dll.nlx_bn254_plonk_commit(ctx.handle, key.handle, k, lw.ctypes.data, b2.ctypes.data, pt.ctypes.data, c.ctypes.data) == NLX_E_RANGE
    # a key without commitments: no hint, and commit_blinding must be NULL
    plain = P.ResidentKey(ctx, inst.fixed, srs, inst.k1, inst.k2)
    assert nlx.lib.dll.nlx_bn254_plonk_commit(ctx.handle, plain.handle, 0, lw.ctypes.data, b2.ctypes.data, pt.ctypes.data, c.ctypes.data) == NLX_E_INVAL
    assert _raw_prove(nlx, ctx, plain, (l, r, o), pubs, blind, cblind)[0] == NLX_E_INVAL
    with pytest.raises(ValueError):
        P.prove_resident(plain, l, r, o, pubs, blind, cblind)
    with pytest.raises(ValueError):
        P.commit_resident(plain, 0, l, [1, 2])
    plain.close()
    # creation: an SRS of n + 2 points, a qcp with a stray 1, rows that do not ascend, a row outside H
    with pytest.raises(nlx.NlxError) as ei:
        P.ResidentKey(ctx, inst.key_values(), srs[:n + 2], inst.k1, inst.k2, commitments=inst.commitment_info())
    assert ei.value.code == NLX_E_RANGE
    values = inst.key_values()
    stray = list(values["qcp1"])
    stray[next(i for i in range(n) if not stray[i])] = 1
    with pytest.raises(ValueError) as ei:
        P.ResidentKey(ctx, dict(values, qcp1=stray), srs, inst.k1, inst.k2, commitments=inst.commitment_info())
    assert "qcp" in str(ei.value)
    two = list(values["qcp0"])
    two[inst.committed[0][0]] = 2
    with pytest.raises(ValueError):
        P.ResidentKey(ctx, dict(values, qcp0=two), srs, inst.k1, inst.k2, commitments=inst.commitment_info())
    info = inst.commitment_info()
    if len(info[0]["committed"]) > 1:
        info[0] = dict(info[0], committed=info[0]["committed"][::-1])
        with pytest.raises(nlx.NlxError) as ei:
            P.ResidentKey(ctx, values, srs, inst.k1, inst.k2, commitments=info)
        assert ei.value.code == NLX_E_RANGE
    info = inst.commitment_info()
    info[1] = dict(info[1], row=n)
    with pytest.raises(nlx.NlxError) as ei:
        P.ResidentKey(ctx, values, srs, inst.k1, inst.k2, commitments=info)
    assert ei.value.code == NLX_E_RANGE
    # the context and the key work afterwards
    assert P.prove_resident(key, l, r, o, pubs, blind, cblind) == want
    key.close()
