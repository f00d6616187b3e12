"""CPU: the big-integer model of gnark-shaped PLONK proofs WITH Bsb22 commitments (tools/gnark_bsb22_model.py) - hash_to_field's
known answers, byte equality with the frozen model (oracle/bn254_py.py gnark_plonk_prove_model) when there is no commitment, and
the trapdoor verifier's verdicts on proofs with one and two (chained) commitments.  Needs no GPU and no library."""
import os
import random
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bsb22_model as gm  # noqa: E402

bn = gm.bn
R = gm.R


def test_expand_message_xmd_reproduces_the_rfc_vectors():
    """RFC 9380 appendix K.1 (SHA-256, DST QUUX-V01-CS02-with-expander-SHA256-128), 32 bytes out"""
    dst = b"QUUX-V01-CS02-with-expander-SHA256-128"
    assert gm.expand_message_xmd(b"", dst, 32).hex() == "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"
    assert gm.expand_message_xmd(b"abc", dst, 32).hex() == "d8ccab23b5985ccea865c6c97b6e5b8350e794e603b4b97902f53a8a0d605615"


def test_hash_to_field_of_the_point_at_infinity():
    assert gm.hash_to_field(bytes([0x40]) + bytes(63), b"BSB22-Plonk") == \
        11312129566162852380451934810540774124391616623240378709706326400922366027385
    assert gm.hash_to_field(bn.g1_marshal(None)) == gm.hash_to_field(bytes([0x40]) + bytes(63), b"BSB22-Plonk")


def _product_hash_to_field():
    """The product's own hash_to_field without loading the library (importing the package loads libnlx.so, which a CPU test
    must not need): the function's source, run on its own.  This relies on the function using nothing but hashlib, R and
    BSB22_DST; if it ever grows a helper, the NameError raised here means: add that helper to `keep` below."""
    import ast
    import hashlib
    path = os.path.join(ROOT, "near-light-client_amd", "bn254_plonk.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    keep = [node for node in tree.body if (isinstance(node, ast.FunctionDef) and node.name == "hash_to_field")
            or (isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "BSB22_DST")]
    assert len(keep) == 2
    scope = {"hashlib": hashlib, "R": R}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), scope)
    return scope["hash_to_field"]


def test_the_products_hash_to_field_equals_the_models():
    h = _product_hash_to_field()
    rng = random.Random(22)
    for size in (0, 1, 31, 32, 63, 64, 65, 200):
        msg = bytes(rng.randrange(256) for _ in range(size))
        assert h(msg) == gm.hash_to_field(msg)
        assert h(msg, b"another-dst") == gm.hash_to_field(msg, b"another-dst")
    with open(os.path.join(ROOT, "near-light-client_amd", "bn254_plonk.py")) as f:   # the product imports nothing of the test side
        imports = [line for line in f if line.lstrip().startswith(("import ", "from "))]
    assert imports and not any(word in line for line in imports for word in ("oracle", "bn254_py", "gnark_bsb22_model"))


@pytest.mark.parametrize("log_n,n_pi", [(3, 0), (4, 2), (6, 3)])
def test_without_commitments_the_bytes_equal_the_frozen_models(log_n, n_pi):
    rng = random.Random(300 + log_n)
    inst = gm.Instance(log_n, 0, rng, n_pi=n_pi)
    tau = rng.randrange(1, R)
    srs = bn.kzg_srs(tau, inst.n + 3)
    blind = [rng.randrange(R) for _ in range(9)]
    l, r, o = inst.complete([])
    p = dict(inst.fixed, l=l, r=r, o=o)
    _, want = bn.gnark_plonk_prove_model(p, srs, inst.k1, inst.k2, inst.public_inputs, blind)
    _, got = gm.prove(inst, srs, blind)
    assert got == want and len(got) == gm.proof_length(0)
    assert gm.prove(inst, srs, blind, tau=tau)[1] == want        # commitments as p(tau) G: the same points
    vk = gm.verifying_key(inst, srs)
    assert gm.verify_trapdoor(got, vk, inst.n, tau, inst.k1, inst.k2, inst.public_inputs)
    assert bn.gnark_plonk_verify_trapdoor(got, vk, inst.n, tau, inst.k1, inst.k2, inst.public_inputs)


@pytest.mark.parametrize("n_pi", [0, 3])
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
@pytest.mark.parametrize("k", [1, 2])
def test_proofs_with_commitments_verify_and_every_change_is_rejected(k, log_n, n_pi):
    """k = 2 is a chain: a committed row of commitment 1 is copy-constrained to the L wire of commitment 0's row (c_0)"""
    rng = random.Random(1000 * k + 10 * log_n + n_pi)
    inst = gm.Instance(log_n, k, rng, n_pi=n_pi, chain=True)
    n = inst.n
    if k == 2:
        assert inst.cells[0][inst.committed[1][0]] == inst.cells[0][inst.commit_rows[0]]
    tau = rng.randrange(1, R)
    srs = bn.kzg_srs(tau, n + 3)
    blind = [rng.randrange(R) for _ in range(9)]
    cblind = [rng.randrange(R) for _ in range(2 * k)]
    proof, data = gm.prove(inst, srs, blind, cblind)
    if log_n <= 4:
        assert gm.prove(inst, srs, blind, cblind, tau=tau)[1] == data and gm.verifying_key(inst, srs, tau) == gm.verifying_key(inst, srs)
    assert len(data) == 7 * 32 + 4 + 32 * k + 32 + 4 + 32 * (7 + k) + 64
    parsed = gm.proof_from_bytes(data)
    assert parsed["bsb22"] == proof["bsb22"] and parsed["batched"]["values"] == proof["batched"]["values"] and len(parsed["bsb22"]) == k
    assert any(proof["quotient"][3 * n:3 * n + 6]) and not any(proof["quotient"][3 * n + 6:])
    vk = gm.verifying_key(inst, srs)
    pubs = inst.public_inputs
    verify = lambda d, pi=pubs: gm.verify_trapdoor(d, vk, n, tau, inst.k1, inst.k2, pi)
    assert verify(data)
    # other blinding of the commitments: other points, other c_j, still accepted
    _, data2 = gm.prove(inst, srs, blind, [x + 1 for x in cblind])
    assert data2 != data and verify(data2)
    # a flipped byte in every region: each Bsb22 point, each claimed value (the qcp_j(zeta) among them), Z, the hs, both openings
    regions = gm.proof_regions(k)
    assert {"bsb22_%d" % j for j in range(k)} | {"qcp%d_zeta" % j for j in range(k)} <= set(regions)
    for name, (off, length) in regions.items():
        bad = bytearray(data)
        bad[off + length - 1] ^= 1
        assert not verify(bytes(bad)), name
    for j in range(k):                   # and a Bsb22 point replaced by another point of the curve
        off = regions["bsb22_%d" % j][0]
        other = bn.g1_compress(bn.g1_mul(7 + j, bn.G1))
        assert not verify(data[:off] + other + data[off + 32:]), j
    # the k-count word altered
    off = regions["bsb22_count"][0]
    for other_k in (k - 1, k + 1, 0):
        if other_k != k:
            assert not verify(data[:off] + other_k.to_bytes(4, "big") + data[off + 4:])
    # a commitment dropped consistently (count, point and claimed value): still a well-formed proof, still rejected
    lo, hi = regions["bsb22_%d" % (k - 1)], regions["qcp%d_zeta" % (k - 1)]
    cut = bytearray(data[:lo[0]] + data[lo[0] + 32:hi[0]] + data[hi[0] + 32:])
    cut[off:off + 4] = (k - 1).to_bytes(4, "big")
    cc = regions["claimed_count"][0] - 32
    cut[cc:cc + 4] = (7 + k - 1).to_bytes(4, "big")
    assert len(gm.proof_from_bytes(bytes(cut))["bsb22"]) == k - 1 and not verify(bytes(cut))
    # a changed public input
    if n_pi:
        assert not verify(data, [(pubs[0] + 1) % R] + pubs[1:])
        assert not verify(data, pubs[:-1])
    else:
        assert not verify(data, [1])


def test_the_model_needs_the_commitment_term():
    """the quotient without sum_j qcp_j pi2_j does not divide: the committed rows' gates read - l + pi2_j = 0"""
    rng = random.Random(5)
    inst = gm.Instance(4, 1, rng, n_pi=1)
    n = inst.n
    srs = bn.kzg_srs(rng.randrange(1, R), n + 3)
    (l, r, o), pi2, pi2_co, _, cs = gm.solve(inst, srs, [3, 4])
    assert l[inst.commit_rows[0]] == cs[0] and pi2[0][inst.commit_rows[0]] == 3 and pi2[0][inst.last_row] == 4
    assert all(pi2[0][i] == l[i] for i in inst.committed[0])
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    co = {name: bn.ntt(v, inverse=True) for name, v in inst.fixed.items()}
    co.update(l=bn.ntt(l, inverse=True), r=bn.ntt(r, inverse=True), o=bn.ntt(o, inverse=True),
              z=bn.ntt(gm.grand_product(l, r, o, inst.fixed, n, beta, gamma, inst.k1, inst.k2), inverse=True))
    pi = list(inst.public_inputs) + [0] * (n - 1)
    pi[inst.commit_rows[0]] = cs[0]
    co["pi"] = bn.ntt(pi, inverse=True)
    assert any(gm.quotient(co, n, 5, inst.k1, inst.k2, alpha, beta, gamma)[3 * n:])
    co["qcp0"], co["pi20"] = bn.ntt(inst.qcp[0], inverse=True), pi2_co[0]
    assert not any(gm.quotient(co, n, 5, inst.k1, inst.k2, alpha, beta, gamma, 1)[3 * n:])
    # and a pi2 that does not close its rows is seen
    broken = list(pi2[0])
    broken[inst.committed[0][0]] = (broken[inst.committed[0][0]] + 1) % R
    co["pi20"] = bn.ntt(broken, inverse=True)
    assert any(gm.quotient(co, n, 5, inst.k1, inst.k2, alpha, beta, gamma, 1)[3 * n:])
