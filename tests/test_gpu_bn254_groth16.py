"""GPU: Groth16 over BN254 from a resident proving key (nlx_bn254_groth16_key_create, nlx_bn254_r1cs_eval,
nlx_bn254_groth16_prove) against the big-integer model tools/groth16_model.py: the SpMV on every generator shape, whole proofs
whose bytes equal the model's and which the trapdoor verifier accepts, the refusals, and one full-size structured case.  Every
comparison is exact."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu
bn = gm.bn
R = gm.R
E_INVAL, E_RANGE, E_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def g16(nlx):
    return nlx.bn254_groth16


@pytest.fixture(scope="module")
def bases():
    """64 distinct G1 points and 16 distinct G2 points for structured keys"""
    rng = random.Random(64)
    return [gm.g1_gen_mul(rng.randrange(1, R)) for _ in range(64)], [gm.g2_gen_mul(rng.randrange(1, R)) for _ in range(16)]


def _r1cs(g16, inst):
    out = {m: (np.array(inst.csr[m][0], dtype=np.uint64), np.array(inst.csr[m][1], dtype=np.uint32), np.array(inst.csr[m][2], dtype=np.uint32))
           for m in "ABC"}
    out["coeffs"] = g16.fr_pack(inst.coeffs)
    return out


class StructuredKey:
    """Not a valid key: every query is tiled from a few distinct points (wire i holds G1 base (i + shift) mod 64, G2 base i mod
    16), masked where the wire does not occur in A / B.  A proof is linear algebra over whatever points the key holds, so the
    expected points are regrouped scalar sums times the bases."""

    def __init__(self, nlx, inst, bases):
        self.inst, (self.g1, self.g2) = inst, bases
        nw, n = inst.n_wires, inst.n
        self.mask_a = [not x for x in inst.occurs("A")]
        self.mask_b = [not x for x in inst.occurs("B")]
        p1, p2 = nlx.bn254_g1_pack(self.g1), nlx.bn254_g2_pack(self.g2)
        wires = np.arange(nw)
        keep_a, keep_b = wires[~np.array(self.mask_a)], wires[~np.array(self.mask_b)]
        self.arrays = dict(
            g1_a=p1[keep_a % 64], g1_b=p1[(keep_b + 7) % 64], g2_b=p2[keep_b % 16], g1_k=p1[(3 * wires[inst.n_public:] + 1) % 64],
            g1_z=p1[(5 * np.arange(n - 1) + 2) % 64], infinity_a=np.array(self.mask_a, dtype=np.uint8), infinity_b=np.array(self.mask_b, dtype=np.uint8),
            g1_alpha=p1[1], g1_beta=p1[2], g1_delta=p1[3], g2_beta=p2[1], g2_delta=p2[2])

    def create(self, g16, ctx, r1cs=True, **override):
        inst = self.inst
        kw = dict(self.arrays)
        kw.update(log_n=inst.log_n, n_wires=inst.n_wires, n_public=inst.n_public, n_constraints=inst.n_constraints)
        if r1cs:                                       # True: the instance's own matrices; a dict: those
            kw["r1cs"] = _r1cs(g16, inst) if r1cs is True else r1cs
        kw.update(override)
        return g16.ProvingKey(ctx, **kw)

    def expected(self, witness, h, r, s):
        inst = self.inst
        sa, sb1, sb2, sk, sz = [0] * 64, [0] * 64, [0] * 16, [0] * 64, [0] * 64
        for i, w in enumerate(witness):
            if not self.mask_a[i]:
                sa[i % 64] += w
            if not self.mask_b[i]:
                sb1[(i + 7) % 64] += w
                sb2[i % 16] += w
            if i >= inst.n_public:
                sk[(3 * i + 1) % 64] += w
        for i in range(inst.n - 1):
            sz[(5 * i + 2) % 64] += h[i]
        alpha, beta, delta, beta2, delta2 = self.g1[1], self.g1[2], self.g1[3], self.g2[1], self.g2[2]
        ar = bn.g1_add(bn.g1_add(bn.msm_g1(sa, self.g1), alpha), bn.g1_mul(r, delta))
        bs1 = bn.g1_add(bn.g1_add(bn.msm_g1(sb1, self.g1), beta), bn.g1_mul(s, delta))
        bs = bn.g2_add(bn.g2_add(gm.msm_g2(sb2, self.g2), beta2), gm.g2_mul(s, delta2))
        krs = bn.g1_add(bn.msm_g1(sk, self.g1), bn.msm_g1(sz, self.g1))
        krs = bn.g1_add(bn.g1_add(krs, bn.g1_mul(s, ar)), bn.g1_mul(r, bs1))
        return ar, bs, bn.g1_add(krs, bn.g1_neg(bn.g1_mul(r * s % R, delta)))


def _model_key(nlx, g16, ctx, inst, pk, r1cs=True):
    return g16.ProvingKey(
        ctx, inst.log_n, inst.n_wires, inst.n_public, inst.n_constraints, nlx.bn254_g1_pack(pk["g1_a"]), nlx.bn254_g1_pack(pk["g1_b"]),
        nlx.bn254_g2_pack(pk["g2_b"]), nlx.bn254_g1_pack(pk["g1_k"]), nlx.bn254_g1_pack(pk["g1_z"]),
        np.array(pk["infinity_a"], dtype=np.uint8), np.array(pk["infinity_b"], dtype=np.uint8), nlx.bn254_g1_pack([pk["g1_alpha"]])[0],
        nlx.bn254_g1_pack([pk["g1_beta"]])[0], nlx.bn254_g1_pack([pk["g1_delta"]])[0], nlx.bn254_g2_pack([pk["g2_beta"]])[0],
        nlx.bn254_g2_pack([pk["g2_delta"]])[0], r1cs=_r1cs(g16, inst) if r1cs else None)


def _points(nlx, ar, bs, krs):
    return nlx.bn254_g1_unpack(ar), nlx.bn254_g2_unpack(bs), nlx.bn254_g1_unpack(krs)


# ---- the SpMV ----
# every generator shape at 2^3 .. 2^12 constraints, powers of two and not
EVAL_CASES = [("common", 8), ("public3", 13), ("empty", 50), ("absent", 100), ("all_a", 200), ("all_b", 333), ("long", 777), ("unit", 1024),
              ("general", 1500), ("long", 2048), ("common", 4096), ("absent", 3000)]


def _check_eval(g16, key, inst, witness, device=None):
    w = g16.fr_pack(witness)
    if device is not None:
        import torch
        w = torch.from_numpy(w.view(np.int64)).to(device)
    out = g16.r1cs_eval(key, w)
    if device is not None:
        out = out.cpu().numpy().view(np.uint64)
    want = inst.abc(witness)
    for m in range(3):
        assert g16.fr_unpack(out[m]) == want[m], "ABC"[m]


@pytest.mark.parametrize("shape,n_constraints", EVAL_CASES)
def test_r1cs_eval_equals_model(nlx, ctx, g16, bases, shape, n_constraints):
    rng = random.Random(3000 + n_constraints)
    inst = gm.Instance(n_constraints, rng, **gm.SHAPES[shape])
    assert inst.satisfied()
    key = StructuredKey(nlx, inst, bases).create(g16, ctx)
    info = key.info()
    assert info["lane_rows"] + info["wave_rows"] == 3 * n_constraints and info["terms"] == sum(len(inst.csr[m][1]) for m in "ABC")
    units = sum(1 for m in "ABC" for c in inst.csr[m][2] if inst.coeffs[c] in (1, R - 1))
    assert info["unit_terms"] == units
    if shape == "unit":
        assert units == info["terms"]                    # every coefficient is 1 or -1: no product
    if shape == "general":
        assert units == 0                                # none is
    if shape in ("long", "all_a", "all_b"):
        assert info["wave_rows"] >= 1                    # the wave-per-row path ran
    long_rows = sum(1 for m in "ABC" for row in inst.rows[m] if len(row) > info["long_row_threshold"])
    assert info["wave_rows"] == long_rows
    _check_eval(g16, key, inst, inst.witness)                                   # host pointers
    _check_eval(g16, key, inst, inst.witness, device="cuda:%d" % ctx.device)    # device pointers
    other = [1] + [rng.randrange(R) for _ in range(inst.n_wires - 1)]           # any vector, edge values included
    other[-1], other[1] = R - 1, 0
    _check_eval(g16, key, inst, other)
    key.close()


def test_r1cs_eval_a_row_over_all_of_4096_wires(nlx, ctx, g16, bases):
    """one row touches every one of 2^12 wires: the wave-per-row path, asserted from the key's reported row split"""
    rng = random.Random(4096)
    inst = gm.Instance(4096 - 4 + 1, rng, all_wires="a", n_secret=3)     # 4 free wires + 4092 defined ones = 2^12 wires
    assert inst.n_wires == 4096 and len(inst.rows["A"][-1]) == 4096 and inst.log_n == 12
    key = StructuredKey(nlx, inst, bases).create(g16, ctx)
    info = key.info()
    assert info["wave_rows"] == 1 and info["lane_rows"] == 3 * inst.n_constraints - 1 and info["long_row_threshold"] < 4096
    _check_eval(g16, key, inst, inst.witness)
    _check_eval(g16, key, inst, inst.witness, device="cuda:%d" % ctx.device)
    key.close()


# ---- whole proofs ----
PROVE_CASES = [("common", 8), ("public3", 13), ("absent", 32), ("empty", 50), ("all_a", 100), ("long", 128), ("all_b", 250), ("unit", 300),
               ("general", 512), ("public3", 1024)]


@pytest.mark.parametrize("shape,n_constraints", PROVE_CASES)
def test_proof_bytes_equal_model_and_verify(nlx, ctx, g16, shape, n_constraints):
    """2^3 .. 2^10 constraints: device bytes = model bytes for the same r, s; the trapdoor verifier accepts; abc= given or computed
    gives the same bytes; a second witness on the same key is proved right (no state leaks between calls)"""
    rng = random.Random(5000 + n_constraints)
    kw = dict(gm.SHAPES[shape])
    if shape == "long":
        kw["long_len"] = 70
    inst = gm.Instance(n_constraints, rng, **kw)
    td = gm.Trapdoor.random(rng)
    pk, _ = gm.setup(inst, td)
    key = _model_key(nlx, g16, ctx, inst, pk)
    r, s = rng.randrange(R), rng.randrange(R)
    w = g16.fr_pack(inst.witness)
    got = g16.prove(key, w, r, s)
    want = gm.prove_by_logs(inst, td, inst.witness, r, s)
    if n_constraints <= 32:
        assert want == gm.prove(inst, pk, inst.witness, r, s)          # the honest sums over the key's points
    assert _points(nlx, *got) == want
    data = g16.proof_bytes(*got)
    assert data == gm.proof_bytes(*want) and len(data) == 164
    assert gm.verify_trapdoor(data, inst, td, inst.witness, r, s)
    # the solver's a, b, c handed in: host arrays, then device tensors
    import torch
    abc = [g16.fr_pack(v) for v in inst.abc()]
    assert g16.proof_bytes(*g16.prove(key, w, r, s, abc=abc)) == data
    dev = "cuda:%d" % ctx.device
    d_abc = [torch.from_numpy(v.view(np.int64)).to(dev) for v in abc]
    d_w = torch.from_numpy(w.view(np.int64)).to(dev)
    assert g16.proof_bytes(*g16.prove(key, d_w, r, s, abc=d_abc)) == data
    # another witness of the same circuit: the same rows with other free wires
    inst2 = gm.Instance(n_constraints, random.Random(5000 + n_constraints), **kw)
    w2 = list(inst2.witness)
    assert inst2.csr == inst.csr and w2 == inst.witness
    free = inst.n_public + kw.get("n_secret", 3)
    w2[1:free] = [rng.randrange(R) for _ in range(free - 1)]
    for j in range(inst.n_constraints):                               # re-solve the internal wires in order
        rc = inst.rows["C"][j]
        if not rc:
            continue
        new = max(i for i, _ in rc)
        val = lambda terms: sum(inst.coeffs[c] * w2[i] for i, c in terms) % R
        rest = [(i, c) for i, c in rc if i != new]
        k = [c for i, c in rc if i == new][0]
        w2[new] = (val(inst.rows["A"][j]) * val(inst.rows["B"][j]) - val(rest)) * gm.inv(inst.coeffs[k]) % R
    assert inst.satisfied(w2) and w2 != inst.witness
    r2, s2 = rng.randrange(R), rng.randrange(R)
    data2 = g16.proof_bytes(*g16.prove(key, g16.fr_pack(w2), r2, s2))
    assert data2 == gm.proof_bytes(*gm.prove_by_logs(inst, td, w2, r2, s2)) and gm.verify_trapdoor(data2, inst, td, w2, r2, s2)
    assert g16.proof_bytes(*g16.prove(key, w, r, s)) == data         # and the first one again
    key.close()


@pytest.mark.parametrize("r,s", [(0, 0), (R - 1, R - 1)])
def test_extreme_blinding_scalars(nlx, ctx, g16, r, s):
    rng = random.Random(99)
    inst = gm.Instance(20, rng, n_public=3)
    td = gm.Trapdoor.random(rng)
    pk, _ = gm.setup(inst, td)
    key = _model_key(nlx, g16, ctx, inst, pk)
    data = g16.proof_bytes(*g16.prove(key, g16.fr_pack(inst.witness), r, s))
    assert data == gm.proof_bytes(*gm.prove(inst, pk, inst.witness, r, s)) and gm.verify_trapdoor(data, inst, td, inst.witness, r, s)
    ar, bs, krs = g16.prove(key, g16.fr_pack(inst.witness))            # r, s from `secrets`: a valid point triple, different each time
    assert g16.proof_bytes(ar, bs, krs) != data and len(gm.proof_from_bytes(g16.proof_bytes(ar, bs, krs))) == 3
    key.close()


def _raw_prove(nlx, g16, ctx, key, w, r, s, outs, abc=(None, None, None)):
    p = lambda a: None if a is None else a.ctypes.data
    return nlx.lib.dll.nlx_bn254_groth16_prove(ctx.handle, key.handle, p(w), p(abc[0]), p(abc[1]), p(abc[2]), p(g16.fr_words(r)),
                                               p(g16.fr_words(s)), p(outs[0]), p(outs[1]), p(outs[2]))


def test_bad_witnesses_and_refusals(nlx, ctx, g16, bases):
    """an unsatisfied witness and w[0] = 2 return NLX_E_INVAL and write no output; every refusal returns its code; the context
    stays usable: a good proof after all of them"""
    rng = random.Random(404)
    inst = gm.Instance(40, rng, n_public=3)
    td = gm.Trapdoor.random(rng)
    pk, _ = gm.setup(inst, td)
    key = _model_key(nlx, g16, ctx, inst, pk)
    w = g16.fr_pack(inst.witness)
    r, s = rng.randrange(R), rng.randrange(R)
    fresh = lambda: [np.full(8, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64)]
    untouched = lambda outs: all((o == 7).all() for o in outs)
    # the unsatisfied variant (one witness entry changed), with a, b, c computed and with the bad values handed in
    w_bad = inst.unsatisfied_witness()
    a, b, c = inst.abc(w_bad)
    first = min(i for i in range(inst.n) if a[i] * b[i] % R != c[i])
    outs = fresh()
    assert _raw_prove(nlx, g16, ctx, key, g16.fr_pack(w_bad), r, s, outs) == E_INVAL and untouched(outs)
    assert ("row %d" % first) in nlx.lib.dll.nlx_last_error(ctx.handle).decode()
    assert _raw_prove(nlx, g16, ctx, key, w, r, s, outs, abc=[g16.fr_pack(v) for v in (a, b, c)]) == E_INVAL and untouched(outs)
    with pytest.raises(nlx.NlxError) as e:
        g16.prove(key, g16.fr_pack(w_bad), r, s)
    assert e.value.code == E_INVAL
    # w[0] = 2
    w2 = [2] + inst.witness[1:]
    assert _raw_prove(nlx, g16, ctx, key, g16.fr_pack(w2), r, s, outs, abc=[g16.fr_pack(v) for v in inst.abc()]) == E_INVAL and untouched(outs)
    assert "constant wire" in nlx.lib.dll.nlx_last_error(ctx.handle).decode()
    # NULL pointers
    assert _raw_prove(nlx, g16, ctx, key, None, r, s, outs) == E_INVAL
    assert _raw_prove(nlx, g16, ctx, key, w, r, s, [None, outs[1], outs[2]]) == E_INVAL
    assert _raw_prove(nlx, g16, ctx, key, w, r, s, outs, abc=[g16.fr_pack(inst.abc()[0]), None, None]) == E_INVAL and untouched(outs)
    assert nlx.lib.dll.nlx_bn254_groth16_prove(ctx.handle, None, w.ctypes.data, None, None, None, w.ctypes.data, w.ctypes.data,
                                               outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data) == E_INVAL
    assert nlx.lib.dll.nlx_bn254_groth16_key_create(ctx.handle, None, ctypes.byref(ctypes.c_void_p())) == E_INVAL
    assert nlx.lib.dll.nlx_bn254_r1cs_eval(ctx.handle, key.handle, None, w.ctypes.data, w.ctypes.data, w.ctypes.data) == E_INVAL
    # a key without matrices: no r1cs_eval, no proof without a, b, c - but a proof with them
    bare = _model_key(nlx, g16, ctx, inst, pk, r1cs=False)
    assert _raw_prove(nlx, g16, ctx, bare, w, r, s, outs) == E_INVAL and untouched(outs)
    with pytest.raises(nlx.NlxError) as e:
        g16.r1cs_eval(bare, w)
    assert e.value.code == E_INVAL
    want = gm.proof_bytes(*gm.prove_by_logs(inst, td, inst.witness, r, s))
    assert g16.proof_bytes(*g16.prove(bare, w, r, s, abc=[g16.fr_pack(v) for v in inst.abc()])) == want
    bare.close()
    # the descriptor's refusals
    sk = StructuredKey(nlx, inst, bases)
    r1cs = _r1cs(g16, inst)

    def refused(code, **override):
        with pytest.raises(nlx.NlxError) as e:
            sk.create(g16, ctx, **override)
        assert e.value.code == code, (override.keys(), e.value)

    refused(E_RANGE, log_n=0)
    refused(E_RANGE, log_n=27)
    refused(E_RANGE, log_n=5)                                          # n_constraints = 40 > 2^5
    refused(E_RANGE, flags=0)
    refused(E_RANGE, flags=3)
    refused(E_UNSUPPORTED, n_commitments=1)
    mask = sk.arrays["infinity_a"].copy()
    mask[int(np.flatnonzero(mask == 0)[0])] = 1
    refused(E_RANGE, infinity_a=mask)                                  # one clear entry fewer than G1.A holds points
    refused(E_RANGE, g1_b=sk.arrays["g1_b"][:-1], g2_b=sk.arrays["g2_b"][:-1])
    refused(E_RANGE, g2_b=sk.arrays["g2_b"][:-1])
    refused(E_RANGE, g1_k=sk.arrays["g1_k"][:-1])
    refused(E_RANGE, g1_z=sk.arrays["g1_z"][:-1])
    for m in "ABC":
        row_ptr, wire, cid = r1cs[m]
        bad_wire = wire.copy()
        bad_wire[len(wire) // 2] = inst.n_wires
        refused(E_RANGE, r1cs=dict(r1cs, **{m: (row_ptr, bad_wire, cid)}))
        bad_cid = cid.copy()
        bad_cid[0] = len(inst.coeffs)
        refused(E_RANGE, r1cs=dict(r1cs, **{m: (row_ptr, wire, bad_cid)}))
        bad_ptr = row_ptr.copy()
        bad_ptr[3], bad_ptr[4] = bad_ptr[4] + 1, bad_ptr[3]
        refused(E_RANGE, r1cs=dict(r1cs, **{m: (bad_ptr, wire, cid)}))
    # r, s not below the group order
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    outs = fresh()
    assert nlx.lib.dll.nlx_bn254_groth16_prove(ctx.handle, key.handle, w.ctypes.data, None, None, None, big.ctypes.data, g16.fr_words(s).ctypes.data,
                                               outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data) == E_RANGE and untouched(outs)
    # the context and the key are still good
    assert g16.proof_bytes(*g16.prove(key, w, r, s)) == want
    assert gm.verify_trapdoor(want, inst, td, inst.witness, r, s)
    key.close()


def test_full_size_structured_proof(nlx, ctx, g16, bases):
    """2^18 constraints, about 2^18 wires, the queries tiled from 64 G1 and 16 G2 points: Ar, Bs, Krs pinned exactly by regrouped
    scalar sums and 64 / 16 model multiplications; a, b, c computed on the device from the matrices (and compared in full)"""
    import torch
    rng = random.Random(1 << 18)
    inst = gm.Instance(1 << 18, rng, long_rows=3, long_len=300, empty_rows=5)
    assert inst.log_n == 18 and inst.n_constraints == inst.n
    sk = StructuredKey(nlx, inst, bases)
    key = sk.create(g16, ctx)
    a, b, c = inst.abc()
    assert all(x * y % R == z for x, y, z in zip(a, b, c))             # a o b = c holds: c's rows are products the generator solved for
    dev = "cuda:%d" % ctx.device
    d_w = torch.from_numpy(g16.fr_pack(inst.witness).view(np.int64)).to(dev)
    got_abc = g16.r1cs_eval(key, d_w).cpu().numpy().view(np.uint64)
    for m, want in enumerate((a, b, c)):
        assert np.array_equal(got_abc[m], g16.fr_pack(want)), "ABC"[m]
    h = bn.groth16_quotient(a, b, c, gm.COSET_SHIFT)
    r, s = rng.randrange(R), rng.randrange(R)
    got = _points(nlx, *g16.prove(key, d_w, r, s))
    want = sk.expected(inst.witness, h, r, s)
    assert got[0] == want[0], "Ar"
    assert got[1] == want[1], "Bs"
    assert got[2] == want[2], "Krs"
    key.close()
