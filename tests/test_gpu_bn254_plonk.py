"""GPU parity tests of row f.4's third piece - the PLONK prover's quotient chain and a KZG opening over BN254's scalar field
(nlx_bn254_plonk_quotient, nlx_bn254_kzg_open; csrc/bn254_plonk.hip) - against the pure-Python big-integer model
(oracle/bn254_py.py: plonk_quotient, kzg_open, plonk_witness).  gnark is Go and not in /root/reference: the model restates
the published protocol, parity unpinned as for the rest of row f.4."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bn():
    import bn254_py
    return bn254_py


def _mont(bn, values):
    return [bn.to_montgomery(v) for v in values]


@pytest.mark.parametrize("log_n,with_pi", [(2, False), (3, True), (5, False), (8, True), (10, False)])
def test_quotient_chain_equals_model(nlx, ctx, bn, log_n, with_pi):
    rng = random.Random(100 + log_n)
    u = 5                                                  # gnark's coset generator; k1 = u, k2 = u^2
    k1, k2 = u, u * u % bn.R
    alpha, beta, gamma = (rng.randrange(bn.R) for _ in range(3))
    p = bn.plonk_witness(log_n, rng, k1, k2, beta, gamma)
    n = 1 << log_n
    if with_pi:
        # a public-input polynomial that keeps the gates satisfied: move part of qk into it
        p["pi"] = [rng.randrange(bn.R) if i < 3 else 0 for i in range(n)]
        p["qk"] = [(a - b) % bn.R for a, b in zip(p["qk"], p["pi"])]
    want = bn.plonk_quotient(p, u, k1, k2, alpha, beta, gamma)
    assert not any(want[3 * n:]) and any(want[2 * n:3 * n])
    packed = {k: nlx.bn254_pack([_mont(bn, v)])[0] for k, v in p.items()}
    sc = [bn.to_montgomery(x) for x in (u, k1, k2, alpha, beta, gamma)]
    t, ok = nlx.bn254_plonk_quotient(ctx, packed, *sc)
    assert ok
    got = [bn.from_montgomery(x) for chunk in nlx.bn254_unpack(t) for x in chunk]
    assert got == want[:3 * n]
    # the same from device-resident inputs
    import torch
    dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in packed.items()}
    t2, ok2 = nlx.bn254_plonk_quotient(ctx, dev, *sc)
    assert ok2 and np.array_equal(t2, t)
    # the chain transforms a copy of its own: a caller's device-resident polynomials are not modified
    for k, v in packed.items():
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint64), v), k
    # the identity the verifier checks, at a random point: (gate + alpha perm + alpha^2 L1 (z - 1))(zeta) = t(zeta) Z_H(zeta)
    zeta = rng.randrange(bn.R)
    co = {k: bn.ntt(v, inverse=True) for k, v in p.items()}
    e = {k: bn.eval_poly(c, zeta) for k, c in co.items()}
    zw = bn.eval_poly(co["z"], zeta * bn.root_of_unity(log_n) % bn.R)
    R = bn.R
    gate = (e["ql"] * e["l"] + e["qr"] * e["r"] + e["qm"] * e["l"] * e["r"] + e["qo"] * e["o"] + e["qk"] + e.get("pi", 0)) % R
    f = (e["l"] + beta * zeta + gamma) * (e["r"] + beta * k1 * zeta + gamma) * (e["o"] + beta * k2 * zeta + gamma) * e["z"] % R
    g = (e["l"] + beta * e["s1"] + gamma) * (e["r"] + beta * e["s2"] + gamma) * (e["o"] + beta * e["s3"] + gamma) * zw % R
    zh = (pow(zeta, n, R) - 1) % R
    l1 = zh * pow(n * (zeta - 1) % R, R - 2, R) % R
    assert (gate + alpha * (f - g) + alpha * alpha * l1 * (e["z"] - 1)) % R == bn.eval_poly(got, zeta) * zh % R


def test_a_witness_that_breaks_a_gate_is_reported(nlx, ctx, bn):
    rng = random.Random(7)
    alpha, beta, gamma = (rng.randrange(bn.R) for _ in range(3))
    p = bn.plonk_witness(6, rng, 5, 25, beta, gamma, satisfied=False)
    packed = {k: nlx.bn254_pack([_mont(bn, v)])[0] for k, v in p.items()}
    t, ok = nlx.bn254_plonk_quotient(ctx, packed, *[bn.to_montgomery(x) for x in (5, 5, 25, alpha, beta, gamma)])
    assert not ok
    want = bn.plonk_quotient(p, 5, 5, 25, alpha, beta, gamma)
    assert [bn.from_montgomery(x) for chunk in nlx.bn254_unpack(t) for x in chunk] == want[:3 * 64] and any(want[3 * 64:])
    del packed["z"]
    with pytest.raises(ValueError):
        nlx.bn254_plonk_quotient(ctx, packed, 1, 1, 1, 1, 1, 1)


@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 127, 4096, 4097, 64 * 64 * 2 + 5, (1 << 15) + 321])
def test_kzg_open_equals_model(nlx, ctx, bn, m):
    """the synthetic division as a three-phase scan: one run, exactly full runs, a short last run, two and three levels"""
    rng = random.Random(m)
    coeffs = [rng.randrange(bn.R) for _ in range(m)]
    zeta = rng.randrange(bn.R)
    y, q = bn.kzg_open(coeffs, zeta)
    gy, gq, _ = nlx.bn254_kzg_open(ctx, nlx.bn254_pack([_mont(bn, coeffs)])[0], bn.to_montgomery(zeta))
    assert bn.from_montgomery(nlx.bn254_unpack(gy[None, None, :])[0][0]) == y == bn.eval_poly(coeffs, zeta)
    assert [bn.from_montgomery(x) for x in nlx.bn254_unpack(gq[None])[0]] == q


def test_kzg_opening_proof_is_the_commitment_of_the_quotient(nlx, ctx, bn):
    rng = random.Random(11)
    m = 40
    coeffs = [rng.randrange(bn.R) for _ in range(m)]
    zeta = rng.randrange(bn.R)
    srs = nlx.bn254_g1_multiples(ctx, bn.G1, m - 1)     # 1 G, 2 G, ...: any distinct points do
    y, q, proof = nlx.bn254_kzg_open(ctx, nlx.bn254_pack([_mont(bn, coeffs)])[0], bn.to_montgomery(zeta), srs=srs)
    _, want_q = bn.kzg_open(coeffs, zeta)
    pts = [nlx.bn254_g1_unpack(w) for w in srs]
    assert nlx.bn254_g1_unpack(proof) == bn.msm_g1(want_q, pts)
    # and it is what the MSM entry point gives for the returned quotient
    assert np.array_equal(proof, nlx.bn254_msm_g1(ctx, srs, q, montgomery=True))


def _instance(bn, log_n, seed, k1=5, k2=25):
    rng = random.Random(seed)
    p = bn.plonk_witness(log_n, rng, k1, k2, 11, 13)
    p.pop("z")
    tau = rng.randrange(1, bn.R)
    return p, tau


@pytest.mark.parametrize("log_n", [3, 5, 7])
def test_grand_product_and_lincomb_equal_model(nlx, ctx, bn, log_n):
    import torch
    rng = random.Random(log_n)
    n, k1, k2 = 1 << log_n, 5, 25
    beta, gamma = rng.randrange(bn.R), rng.randrange(bn.R)
    p = bn.plonk_witness(log_n, rng, k1, k2, beta, gamma)       # its z is the model's grand product under these challenges
    P = nlx.bn254_plonk
    dev = {k: torch.from_numpy(nlx.bn254_pack([_mont(bn, p[k])])[0].view(np.int64)).cuda() for k in ("l", "r", "o", "s1", "s2", "s3")}
    z = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    assert P.grand_product(ctx, log_n, dev["l"], dev["r"], dev["o"], dev["s1"], dev["s2"], dev["s3"], beta, gamma, k1, k2, z)
    assert [bn.from_montgomery(x) for x in nlx.bn254_unpack(z.cpu().numpy().view(np.uint64)[None])[0]] == p["z"]
    # host arrays in and out, and a permutation the wires do not respect
    z_host = np.zeros((n, 4), dtype=np.uint64)
    host = {k: v.cpu().numpy().view(np.uint64) for k, v in dev.items()}
    assert not P.grand_product(ctx, log_n, host["l"], host["r"], host["o"], host["s2"], host["s1"], host["s3"], beta, gamma, k1, k2, z_host)
    # lincomb
    scal = [rng.randrange(bn.R) for _ in range(5)]
    cols = [[rng.randrange(bn.R) for _ in range(n)] for _ in range(5)]
    polys = [torch.from_numpy(nlx.bn254_pack([_mont(bn, c)])[0].view(np.int64)).cuda() for c in cols]
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    P.lincomb(ctx, polys, scal, out)
    want = [sum(s * c[i] for s, c in zip(scal, cols)) % bn.R for i in range(n)]
    assert [bn.from_montgomery(x) for x in nlx.bn254_unpack(out.cpu().numpy().view(np.uint64)[None])[0]] == want


@pytest.mark.parametrize("log_n", [3, 6])
def test_whole_plonk_proof_equals_model_and_verifies(nlx, ctx, bn, log_n):
    """the five rounds on the device (near-light-client_amd/bn254_plonk.py) against the big-integer prover: nine commitments and
    six evaluations equal, and the verifier's two opening equations hold (pairing replaced by the test SRS's trapdoor)"""
    n, k1, k2 = 1 << log_n, 5, 25
    p, tau = _instance(bn, log_n, 40 + log_n)
    srs_pts = bn.kzg_srs(tau, n)
    want = bn.plonk_prove_model(p, srs_pts, k1, k2)
    P = nlx.bn254_plonk
    pk = P.ProvingKey(ctx, p, nlx.bn254_g1_pack(srs_pts), k1, k2)
    got = P.prove(pk, p["l"], p["r"], p["o"])
    for k in ("a", "b", "c", "z", "t_lo", "t_mid", "t_hi", "w_zeta", "w_zeta_omega"):
        assert nlx.bn254_g1_unpack(got[k]) == want[k], k
    assert got["evals"] == want["evals"]
    vk = {k: nlx.bn254_g1_unpack(pk.commitments[k]) for k in pk.NAMES}
    vk["n"] = n
    as_points = dict({k: nlx.bn254_g1_unpack(got[k]) for k in got if k != "evals"}, evals=got["evals"])
    assert bn.plonk_verify_trapdoor(as_points, vk, tau, k1, k2)
    assert not bn.plonk_verify_trapdoor(dict(as_points, evals=dict(got["evals"], zw=(got["evals"]["zw"] + 1) % bn.R)), vk, tau, k1, k2)
    # a witness with a broken gate / a broken copy is refused before anything is committed to t
    bad_o = list(p["o"])
    bad_o[1] = (bad_o[1] + 1) % bn.R
    with pytest.raises(ValueError):
        P.prove(pk, p["l"], p["r"], bad_o)


@pytest.mark.parametrize("log_n", [1, 4, 9, 12])
def test_groth16_quotient_equals_model(nlx, ctx, bn, log_n):
    """h = (a b - c) / Z_H for c = a b on H (an R1CS the witness satisfies): equal to the model's, a polynomial of degree < n - 1,
    and a b - c = h Z_H at a random point"""
    rng = random.Random(70 + log_n)
    n = 1 << log_n
    a = [rng.randrange(bn.R) for _ in range(n)]
    b = [rng.randrange(bn.R) for _ in range(n)]
    c = [x * y % bn.R for x, y in zip(a, b)]
    pack = lambda v: nlx.bn254_pack([_mont(bn, v)])[0]
    got = [bn.from_montgomery(x) for x in nlx.bn254_unpack(nlx.bn254_plonk.groth16_quotient(ctx, pack(a), pack(b), pack(c))[None])[0]]
    assert got == bn.groth16_quotient(a, b, c) and got[-1] == 0
    if log_n in (1, 4):
        # the same from device-resident a, b, c - which the call leaves as they were (it transforms a copy of its own)
        import torch
        host = [pack(v) for v in (a, b, c)]
        dev = [torch.from_numpy(v.view(np.int64)).cuda() for v in host]
        h_dev = nlx.bn254_plonk.groth16_quotient(ctx, *dev)
        assert [bn.from_montgomery(x) for x in nlx.bn254_unpack(h_dev[None])[0]] == got
        for d, v in zip(dev, host):
            assert np.array_equal(d.cpu().numpy().view(np.uint64), v)
    zeta = rng.randrange(bn.R)
    A, Bp, C = (bn.eval_poly(bn.ntt(v, inverse=True), zeta) for v in (a, b, c))
    assert (A * Bp - C) % bn.R == bn.eval_poly(got, zeta) * (pow(zeta, n, bn.R) - 1) % bn.R


def test_a_coset_shift_inside_the_subgroup_and_scalars_above_r_are_refused(nlx, ctx, bn):
    """Z_H vanishes on a coset whose shift lies in the evaluation subgroup (size 4n for the PLONK chain, n for Groth16's H):
    NLX_E_INVAL with a message instead of a quotient built on inv(0) = 0; a host scalar that is not below r is not an
    fr.Element: NLX_E_RANGE"""
    log_n = 3
    rng = random.Random(5)
    k1, k2 = 5, 25
    alpha, beta, gamma = (rng.randrange(bn.R) for _ in range(3))
    p = bn.plonk_witness(log_n, rng, k1, k2, beta, gamma)
    packed = {k: nlx.bn254_pack([_mont(bn, v)])[0] for k, v in p.items()}
    good = [bn.to_montgomery(x) for x in (5, k1, k2, alpha, beta, gamma)]
    assert nlx.bn254_plonk_quotient(ctx, packed, *good)[1]
    bad_shift = bn.root_of_unity(log_n + 2)                  # an element of the size-4n subgroup
    with pytest.raises(nlx.NlxError) as ei:
        nlx.bn254_plonk_quotient(ctx, packed, bn.to_montgomery(bad_shift), *good[1:])
    assert ei.value.code == -1 and "evaluation subgroup" in str(ei.value)
    for pos in range(6):
        sc = list(good)
        sc[pos] = bn.R + 3                                   # words of a number >= r
        with pytest.raises(nlx.NlxError) as ei:
            nlx.bn254_plonk_quotient(ctx, packed, *sc)
        assert ei.value.code == -4
    assert nlx.bn254_plonk_quotient(ctx, packed, *good)[1]   # the context still works
    n = 1 << log_n
    a = [rng.randrange(bn.R) for _ in range(n)]
    b = [rng.randrange(bn.R) for _ in range(n)]
    c = [x * y % bn.R for x, y in zip(a, b)]
    pack = lambda v: nlx.bn254_pack([_mont(bn, v)])[0]
    with pytest.raises(nlx.NlxError) as ei:
        nlx.bn254_plonk.groth16_quotient(ctx, pack(a), pack(b), pack(c), coset_shift=bn.root_of_unity(log_n))
    assert ei.value.code == -1 and "evaluation subgroup" in str(ei.value)
    nlx.bn254_plonk.groth16_quotient(ctx, pack(a), pack(b), pack(c))


@pytest.mark.parametrize("log_n,n_pi", [(3, 0), (4, 2), (6, 3), (8, 1), (10, 5)])
def test_gnark_shaped_proof_bytes_equal_model_and_verify(nlx, ctx, bn, log_n, n_pi):
    """The proof in gnark's shape (its fiat-shamir with the named challenges gamma, beta, alpha, zeta over SHA-256, blinded
    l r o z, the quotient cut into h1 h2 h3 of n + 2 coefficients, BatchOpenSinglePoint with the hashed combiner, Proof.WriteTo's
    byte layout): the device prover's BYTES equal the big-integer model's for the same blinding scalars, and the model's verifier
    (pairing replaced by the test SRS's trapdoor) accepts them, with and without public inputs.  Parity with gnark itself stays
    unpinned (Go, no vector in the reference): both sides restate the published protocol."""
    n, k1, k2 = 1 << log_n, 5, 25
    p, tau = _instance(bn, log_n, 90 + log_n)
    rng = random.Random(7 * log_n)
    pis = [rng.randrange(bn.R) for _ in range(n_pi)]
    p["qk"] = [(a - (pis[i] if i < n_pi else 0)) % bn.R for i, a in enumerate(p["qk"])]   # the statement's qk leaves the public inputs out
    blind = [rng.randrange(bn.R) for _ in range(9)]
    srs_pts = bn.kzg_srs(tau, n + 3)
    _, want = bn.gnark_plonk_prove_model(p, srs_pts, k1, k2, pis, blind)
    P = nlx.bn254_plonk
    pk = P.ProvingKey(ctx, p, nlx.bn254_g1_pack(srs_pts), k1, k2)
    got = P.prove_gnark(pk, p["l"], p["r"], p["o"], pis, blind)
    assert len(got) == len(want) == 7 * 32 + 4 + 32 + 4 + 7 * 32 + 32 + 32
    assert got == want
    vk = {k: nlx.bn254_g1_unpack(pk.commitments[k]) for k in pk.NAMES}
    assert bn.gnark_plonk_verify_trapdoor(got, vk, n, tau, k1, k2, pis)
    if n_pi:
        assert not bn.gnark_plonk_verify_trapdoor(got, vk, n, tau, k1, k2, [(pis[0] + 1) % bn.R] + pis[1:])
    bad = bytearray(got)
    bad[-1] ^= 1                                                # z(w zeta)
    assert not bn.gnark_plonk_verify_trapdoor(bytes(bad), vk, n, tau, k1, k2, pis)
    # random blinding: other bytes, same verdict; a broken witness is refused
    other = P.prove_gnark(pk, p["l"], p["r"], p["o"], pis)
    assert other != got and bn.gnark_plonk_verify_trapdoor(other, vk, n, tau, k1, k2, pis)
    if log_n == 4:
        bad_o = list(p["o"])
        bad_o[1] = (bad_o[1] + 1) % bn.R
        with pytest.raises(ValueError):
            P.prove_gnark(pk, p["l"], p["r"], bad_o, pis, blind)
        with pytest.raises(ValueError):
            P.prove(pk, p["l"], p["r"], p["o"], pis)               # the paper-shaped prover constrains no public inputs
