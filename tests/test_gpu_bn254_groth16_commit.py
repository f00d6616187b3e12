"""GPU: Groth16 over BN254 on keys with Bsb22 / Pedersen commitments (nlx_bn254_groth16_key_create_committed,
nlx_bn254_groth16_commit, nlx_bn254_groth16_prove_committed) against the big-integer model tools/groth16_commit_model.py: whole
164 + 32 k-byte proofs equal to the model's which its verifier accepts, the committed-set sizes at which the gather kernel
could go wrong, a structured key with about 3 000 committed wires, the solver's hint, the refusals, and the path without
commitments unchanged.  Every comparison is exact."""
import random
import sys
import os

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_commit_model as cm  # noqa: E402
import groth16_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu
bn, R = gm.bn, gm.R
E_INVAL, E_RANGE, E_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def g16(nlx):
    return nlx.bn254_groth16


def _r1cs(g16, inst):
    out = {m: (np.array(inst.csr[m][0], dtype=np.uint64), np.array(inst.csr[m][1], dtype=np.uint32), np.array(inst.csr[m][2], dtype=np.uint32))
           for m in "ABC"}
    out["coeffs"] = g16.fr_pack(inst.coeffs)
    return out


def _key_args(nlx, g16, inst, pk):
    """ProvingKey's keywords for a model key (cm.setup's or gm.setup's pk)"""
    one = lambda p: nlx.bn254_g1_pack([p])[0]
    kw = dict(log_n=inst.log_n, n_wires=inst.n_wires, n_public=inst.n_public, n_constraints=inst.n_constraints,
              g1_a=nlx.bn254_g1_pack(pk["g1_a"]), g1_b=nlx.bn254_g1_pack(pk["g1_b"]), g2_b=nlx.bn254_g2_pack(pk["g2_b"]),
              g1_k=nlx.bn254_g1_pack(pk["g1_k"]), g1_z=nlx.bn254_g1_pack(pk["g1_z"]), infinity_a=np.array(pk["infinity_a"], dtype=np.uint8),
              infinity_b=np.array(pk["infinity_b"], dtype=np.uint8), g1_alpha=one(pk["g1_alpha"]), g1_beta=one(pk["g1_beta"]),
              g1_delta=one(pk["g1_delta"]), g2_beta=nlx.bn254_g2_pack([pk["g2_beta"]])[0], g2_delta=nlx.bn254_g2_pack([pk["g2_delta"]])[0],
              r1cs=_r1cs(g16, inst))
    if "commitments" in pk:
        kw["commitments"] = [dict(private=c["private"], public=c["public"], wire=c["wire"], basis=nlx.bn254_g1_pack(c["basis"]),
                                  basis_exp_sigma=nlx.bn254_g1_pack(c["basis_exp_sigma"])) for c in pk["commitments"]]
    return kw


def _points(nlx, ar, bs, krs, cs, pok):
    return nlx.bn254_g1_unpack(ar), nlx.bn254_g2_unpack(bs), nlx.bn254_g1_unpack(krs), [nlx.bn254_g1_unpack(c) for c in cs], nlx.bn254_g1_unpack(pok)


def _model(n_constraints, counts, seed, shape="common", prepare=None, **kw):
    rng = random.Random(seed)
    inst = cm.CommittedInstance(n_constraints, rng, counts, **dict(gm.SHAPES[shape], **kw))
    td = cm.Trapdoor.random(rng)
    pk, _ = cm.setup(inst, td)
    if prepare:
        prepare(inst)
    w = cm.solve(inst, td=td)
    return inst, td, pk, w, rng.randrange(R), rng.randrange(R)


def _check_proof(nlx, g16, ctx, key, inst, td, w, r, s):
    """device points and bytes = the model's; the model's verifier accepts the device's bytes"""
    got = g16.prove_committed(key, g16.fr_pack(w), r, s)
    want = cm.prove_by_logs(inst, td, w, r, s)
    assert _points(nlx, *got) == want
    data = g16.proof_bytes(*got)
    assert data == cm.proof_bytes(*want) and len(data) == 164 + 32 * inst.k
    assert cm.verify_trapdoor(data, inst, td, w, r, s)
    return data


# ---- whole proofs: 2^3 .. 2^10 constraints, k = 1, 2, 3, eight generator shapes ----
PROVE_CASES = [("common", 8, [2]), ("public3", 13, [3, 1]), ("empty", 50, [4, 0, 3]), ("absent", 100, [5, 5]), ("long", 128, [3, 2, 2]),
               ("all_b", 250, [7]), ("unit", 512, [10, 20]), ("general", 1024, [30, 1, 40])]


@pytest.mark.parametrize("shape,n_constraints,counts", PROVE_CASES)
def test_committed_proof_bytes_equal_model_and_verify(nlx, ctx, g16, shape, n_constraints, counts):
    import torch
    kw = {"long_len": 70} if shape == "long" else {}
    inst, td, pk, w, r, s = _model(n_constraints, counts, 7000 + n_constraints, shape, **kw)
    key = g16.ProvingKey(ctx, **_key_args(nlx, g16, inst, pk))
    info = key.info()
    assert info["committed_wires"] == sum(counts) and info["commitments"] == len(counts)
    data = _check_proof(nlx, g16, ctx, key, inst, td, w, r, s)
    if n_constraints <= 16:
        assert cm.prove(inst, pk, w, r, s) == cm.prove_by_logs(inst, td, w, r, s)         # the honest sums over the key's points
    # the solver's a, b, c handed in; then the witness and a, b, c as device tensors
    packed = g16.fr_pack(w)
    abc = [g16.fr_pack(v) for v in inst.abc(w)]
    assert g16.proof_bytes(*g16.prove_committed(key, packed, r, s, abc=abc)) == data
    dev = "cuda:%d" % ctx.device
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    assert g16.proof_bytes(*g16.prove_committed(key, d_w, r, s)) == data
    assert g16.proof_bytes(*g16.prove_committed(key, d_w, r, s, abc=[torch.from_numpy(v.view(np.int64)).to(dev) for v in abc])) == data
    key.close()


# ---- committed-set sizes at which the gather kernel can go wrong (one lane per committed entry, 256-lane blocks) ----
def _zeros_and_top(inst):
    """set 0: every scalar zero; set 1: one committed wire holds r - 1"""
    for i in inst.commitments[0]["private"]:
        inst.free[i] = 0
    inst.free[inst.commitments[1]["private"][0]] = R - 1


SIZE_CASES = [([1], None), ([63], None), ([64], None), ([65], None), ([255], None), ([256], None), ([257], None),
              ([40, 0, 30], None),                 # an empty set between two others: a segment offset repeats
              ([3, 4], _zeros_and_top)]


@pytest.mark.parametrize("counts,prepare", SIZE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else ("edge-values" if v else "random"))
def test_committed_set_sizes(nlx, ctx, g16, counts, prepare):
    """few constraints, many secret wires to commit: the sets are drawn from the secret wires"""
    m = sum(counts)
    inst, td, pk, w, r, s = _model(12, counts, 8000 + m, n_secret=m + 3, secret_only=True, dependent=False, prepare=prepare)
    assert [len(c["private"]) for c in inst.commitments] == counts
    key = g16.ProvingKey(ctx, **_key_args(nlx, g16, inst, pk))
    _check_proof(nlx, g16, ctx, key, inst, td, w, r, s)
    got = g16.prove_committed(key, g16.fr_pack(w), r, s)
    for j, count in enumerate(counts):
        if count == 0:
            assert not got[3][j].any()                                    # the point at infinity as (0, 0) words
            assert not g16.commit(key, j, g16.fr_pack(w)).any()
    if prepare:
        assert not got[3][0].any() and not g16.commit(key, 0, g16.fr_pack(w)).any()       # all-zero scalars
        assert w[inst.commitments[1]["private"][0]] == R - 1 and got[3][1].any()
    key.close()


# ---- a structured key at 2^12 constraints with about 3 000 committed wires: the multi-block gather ----
def test_structured_key_with_3000_committed_wires(nlx, ctx, g16):
    """Not a valid key: every query and both Pedersen bases are tiled from 64 points, so C_j, Pok and Krs are regrouped scalar
    sums times those points (a proof is linear algebra over whatever points the key holds)."""
    rng = random.Random(1 << 12)
    g1 = [gm.g1_gen_mul(rng.randrange(1, R)) for _ in range(64)]
    g2 = [gm.g2_gen_mul(rng.randrange(1, R)) for _ in range(16)]
    counts = [900, 0, 2100]
    inst = cm.CommittedInstance(1 << 12, rng, counts, long_rows=2, long_len=100)
    assert inst.log_n == 12 and inst.n_committed == 3000
    p1, p2 = nlx.bn254_g1_pack(g1), nlx.bn254_g2_pack(g2)
    nw, n = inst.n_wires, inst.n
    mask_a, mask_b = [not x for x in inst.occurs("A")], [not x for x in inst.occurs("B")]
    wires = np.arange(nw)
    keep_a, keep_b, kept = wires[~np.array(mask_a)], wires[~np.array(mask_b)], np.array(inst.k_wires())
    basis_at = lambda j, i: (7 * i + j) % 64
    sigma_at = lambda j, i: (11 * i + 5 + j) % 64
    comm = [dict(private=c["private"], public=c["public"], wire=c["wire"],
                 basis=p1[[basis_at(j, i) for i in c["private"]]].reshape(-1, 8),
                 basis_exp_sigma=p1[[sigma_at(j, i) for i in c["private"]]].reshape(-1, 8)) for j, c in enumerate(inst.commitments)]
    key = g16.ProvingKey(ctx, inst.log_n, nw, inst.n_public, inst.n_constraints, p1[keep_a % 64], p1[(keep_b + 7) % 64], p2[keep_b % 16],
                         p1[(3 * kept + 1) % 64], p1[(5 * np.arange(n - 1) + 2) % 64], np.array(mask_a, dtype=np.uint8),
                         np.array(mask_b, dtype=np.uint8), p1[1], p1[2], p1[3], p2[1], p2[2], r1cs=_r1cs(g16, inst), commitments=comm)
    assert key.info()["committed_wires"] == 3000 and key.info()["commitments"] == 3

    def c_point(j, w):
        sums = [0] * 64
        for i in inst.commitments[j]["private"]:
            sums[basis_at(j, i)] += w[i]
        return bn.msm_g1(sums, g1)

    w = inst.solve(lambda j, w_: cm.commitment_challenge(c_point(j, w_), [w_[i] for i in inst.commitments[j]["public"]]))
    assert inst.satisfied(w)
    a, b, c = inst.abc(w)
    h = bn.groth16_quotient(a, b, c, gm.COSET_SHIFT)
    r, s = rng.randrange(R), rng.randrange(R)
    got = _points(nlx, *g16.prove_committed(key, g16.fr_pack(w), r, s))
    # the expected points: regrouped sums
    sa, sb1, sb2, sk, sz, sp = [0] * 64, [0] * 64, [0] * 16, [0] * 64, [0] * 64, [0] * 64
    for i, x in enumerate(w):
        if not mask_a[i]:
            sa[i % 64] += x
        if not mask_b[i]:
            sb1[(i + 7) % 64] += x
            sb2[i % 16] += x
    for i in kept:
        sk[(3 * int(i) + 1) % 64] += w[int(i)]
    for i in range(n - 1):
        sz[(5 * i + 2) % 64] += h[i]
    rho = cm.fold_challenge([w[c_["wire"]] for c_ in inst.commitments])
    for j, c_ in enumerate(inst.commitments):
        for i in c_["private"]:
            sp[sigma_at(j, i)] += w[i] * pow(rho, j, R)
    alpha, beta, delta = g1[1], g1[2], g1[3]
    ar = bn.g1_add(bn.g1_add(bn.msm_g1(sa, g1), alpha), bn.g1_mul(r, delta))
    bs1 = bn.g1_add(bn.g1_add(bn.msm_g1(sb1, g1), beta), bn.g1_mul(s, delta))
    bs = bn.g2_add(bn.g2_add(gm.msm_g2(sb2, g2), g2[1]), gm.g2_mul(s, g2[2]))
    krs = bn.g1_add(bn.msm_g1(sk, g1), bn.msm_g1(sz, g1))
    krs = bn.g1_add(bn.g1_add(krs, bn.g1_mul(s, ar)), bn.g1_mul(r, bs1))
    krs = bn.g1_add(krs, bn.g1_neg(bn.g1_mul(r * s % R, delta)))
    assert got[0] == ar, "Ar"
    assert got[1] == bs, "Bs"
    assert got[2] == krs, "Krs"
    assert got[3] == [c_point(j, w) for j in range(3)] and got[3][1] is None, "C_j"
    assert got[4] == bn.msm_g1(sp, g1), "Pok"
    key.close()


# ---- the solver's hint ----
def test_commit_is_the_hint_and_a_solve_loop_reproduces_the_model(nlx, ctx, g16):
    inst, td, pk, w, r, s = _model(60, [6, 5, 4], 9001, "public3", hashed_public=2)
    key = g16.ProvingKey(ctx, **_key_args(nlx, g16, inst, pk))
    got = g16.prove_committed(key, g16.fr_pack(w), r, s)
    for j, c in enumerate(inst.commitments):
        only = [w[i] if i in c["private"] else 0 for i in range(inst.n_wires)]     # zero outside PrivateCommitted_j
        point = g16.commit(key, j, g16.fr_pack(only))
        assert np.array_equal(point, got[3][j]) and nlx.bn254_g1_unpack(point) == cm.commit(pk, j, w)
        assert g16.commitment_challenge(key, j, point, g16.fr_pack(w)) == w[c["wire"]]
    # commit, hash, fill the wire, re-solve, next commitment - on the host and with the partial witness on the device
    import torch
    dev = "cuda:%d" % ctx.device

    def hint(on_device):
        def challenge(j, partial):
            packed = g16.fr_pack([0 if v is None else v for v in partial])
            if on_device:
                packed = torch.from_numpy(packed.view(np.int64)).to(dev)
            return g16.commitment_challenge(key, j, g16.commit(key, j, packed), packed)
        return challenge

    assert inst.solve(hint(False)) == w
    assert inst.solve(hint(True)) == w
    key.close()


# ---- refusals ----
def test_refusals(nlx, ctx, g16):
    inst, td, pk, w, r, s = _model(40, [4, 3], 9002, "public3")
    args = _key_args(nlx, g16, inst, pk)
    key = g16.ProvingKey(ctx, **args)
    packed = g16.fr_pack(w)
    want = _check_proof(nlx, g16, ctx, key, inst, td, w, r, s)
    dll = nlx.lib.dll
    # a commitment wire that holds a wrong value: the circuit is still satisfied where the wire is not used further on
    for j in (1, 0):
        bad = list(w)
        bad[inst.commitments[j]["wire"]] = (bad[inst.commitments[j]["wire"]] + 1) % R
        if not inst.satisfied(bad):
            abc = [g16.fr_pack(v) for v in inst.abc(w)]                 # the honest a, b, c: only the wire's value is wrong
        else:
            abc = None
        with pytest.raises(nlx.NlxError, match="commitment %d" % j) as e:
            g16.prove_committed(key, g16.fr_pack(bad), r, s, abc=abc)
        assert e.value.code == E_INVAL

    # the descriptor
    def refused(code, commitments=None, **override):
        kw = dict(args, **override)
        if commitments is not None:
            kw["commitments"] = commitments
        with pytest.raises(nlx.NlxError) as e:
            g16.ProvingKey(ctx, **kw)
        assert e.value.code == code, (override.keys(), e.value)

    def changed(j, **fields):
        out = [dict(c) for c in args["commitments"]]
        out[j].update(fields)
        return out

    c0, c1 = args["commitments"]
    refused(E_RANGE, changed(0, private=[inst.n_public - 1] + c0["private"][1:]))                  # a public wire
    refused(E_RANGE, changed(1, private=c1["private"][:-1] + [inst.n_wires]))                      # past the wires
    refused(E_RANGE, changed(0, private=[c0["private"][1], c0["private"][0]] + c0["private"][2:]))  # not ascending
    refused(E_RANGE, changed(0, private=[c0["private"][0]] * 2 + c0["private"][2:]))                # twice in one set
    refused(E_RANGE, changed(1, private=sorted(c1["private"][:-1] + [c0["private"][0]])))           # the sets overlap
    refused(E_RANGE, changed(1, wire=c0["private"][0]))                                            # a commitment wire that is committed
    refused(E_RANGE, changed(1, wire=c0["wire"]))                                                  # listed twice
    refused(E_RANGE, changed(0, wire=0))                                                           # a public wire
    refused(E_RANGE, changed(0, wire=inst.n_wires))
    refused(E_RANGE, n_commitments=1)                                                              # the two descriptors disagree
    refused(E_RANGE, n_commitments=0)
    refused(E_RANGE, g1_k=args["g1_k"][:-1])                                                       # G1.K's count
    refused(E_RANGE, g1_k=nlx.bn254_g1_pack(gm.setup(inst, td)[0]["g1_k"]))                        # G1.K over every private wire
    refused(E_RANGE, [dict(c0, public=[], wire=inst.k_wires()[j]) for j in range(9)])              # nine commitments
    refused(E_RANGE, [], n_commitments=0)                                                          # none
    refused(E_RANGE, flags=0)
    plain_args = {k_: v for k_, v in args.items() if k_ != "commitments"}
    with pytest.raises(nlx.NlxError) as e:
        g16.ProvingKey(ctx, **dict(plain_args, n_commitments=2))                                   # the entry without bases, as before
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(ValueError):
        g16.ProvingKey(ctx, **dict(args, commitments=changed(0, basis=c0["basis"][:-1])))           # a basis of the wrong length

    # the raw entries: rho not below r, the wrong kind of key, NULL - and no output is touched
    p = lambda a: None if a is None else a.ctypes.data
    fresh = lambda: [np.full(8, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64),
                     np.full((2, 8), 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64)]
    untouched = lambda outs: all((o == 7).all() for o in outs)
    rw, sw, big = g16.fr_words(r), g16.fr_words(s), np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    modulus = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def raw(key_, w_, rho, outs):
        return dll.nlx_bn254_groth16_prove_committed(ctx.handle, key_.handle, p(w_), None, None, None, p(rw), p(sw), p(rho), *[p(o) for o in outs])

    outs = fresh()
    assert raw(key, packed, big, outs) == E_RANGE and untouched(outs)
    assert raw(key, packed, modulus, outs) == E_RANGE and untouched(outs)
    assert raw(key, packed, None, outs) == E_INVAL and untouched(outs)
    assert raw(key, None, rw, outs) == E_INVAL and untouched(outs)
    assert raw(key, packed, rw, outs[:3] + [None, outs[4]]) == E_INVAL and untouched(outs)
    assert raw(key, g16.fr_pack(inst.unsatisfied_witness()), rw, outs) == E_INVAL and untouched(outs)
    assert "row" in dll.nlx_last_error(ctx.handle).decode()
    assert raw(key, g16.fr_pack([2] + w[1:]), rw, outs) == E_INVAL and untouched(outs)
    assert "constant wire" in dll.nlx_last_error(ctx.handle).decode()
    three = fresh()[:3]
    assert dll.nlx_bn254_groth16_prove(ctx.handle, key.handle, p(packed), None, None, None, p(rw), p(sw), *[p(o) for o in three]) == E_INVAL
    assert untouched(three) and "nlx_bn254_groth16_prove_committed" in dll.nlx_last_error(ctx.handle).decode()
    plain_inst = gm.Instance(40, random.Random(1), n_public=3)
    plain_pk, _ = gm.setup(plain_inst, td)
    plain = g16.ProvingKey(ctx, **_key_args(nlx, g16, plain_inst, plain_pk))
    assert raw(plain, g16.fr_pack(plain_inst.witness), rw, outs) == E_INVAL and untouched(outs)
    assert "nlx_bn254_groth16_prove" in dll.nlx_last_error(ctx.handle).decode()
    point = np.full(8, 7, dtype=np.uint64)
    assert dll.nlx_bn254_groth16_commit(ctx.handle, plain.handle, 0, p(packed), p(point)) == E_INVAL and (point == 7).all()
    assert dll.nlx_bn254_groth16_commit(ctx.handle, key.handle, 2, p(packed), p(point)) == E_RANGE and (point == 7).all()
    assert dll.nlx_bn254_groth16_commit(ctx.handle, key.handle, 0, None, p(point)) == E_INVAL and (point == 7).all()
    with pytest.raises(nlx.NlxError) as e:
        g16.prove(key, packed, r, s)
    assert e.value.code == E_INVAL
    with pytest.raises(nlx.NlxError) as e:
        g16.prove_committed(plain, g16.fr_pack(plain_inst.witness), r, s)
    assert e.value.code == E_INVAL
    # r1cs_eval serves both kinds of key; the context and the key are still good
    for k_, i_, w_ in ((key, inst, w), (plain, plain_inst, plain_inst.witness)):
        out = g16.r1cs_eval(k_, g16.fr_pack(w_))
        assert [g16.fr_unpack(out[m]) for m in range(3)] == list(i_.abc(w_))
    assert g16.proof_bytes(*g16.prove_committed(key, packed, r, s)) == want
    plain.close()
    key.close()


# ---- the path without commitments ----
def test_plain_key_is_unchanged(nlx, ctx, g16):
    rng = random.Random(9003)
    inst = gm.Instance(100, rng, **gm.SHAPES["public3"])
    td = gm.Trapdoor.random(rng)
    pk, _ = gm.setup(inst, td)
    key = g16.ProvingKey(ctx, **_key_args(nlx, g16, inst, pk))
    assert key.commitments == [] and key.info()["commitments"] == 0 and key.info()["committed_wires"] == 0
    r, s = rng.randrange(R), rng.randrange(R)
    pts = g16.prove(key, g16.fr_pack(inst.witness), r, s)
    want = gm.proof_bytes(*gm.prove_by_logs(inst, td, inst.witness, r, s))
    assert g16.proof_bytes(*pts) == want and g16.proof_bytes(*pts, commitments=(), pok=None) == want and len(want) == 164
    assert gm.verify_trapdoor(want, inst, td, inst.witness, r, s)
    key.close()
