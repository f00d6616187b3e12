"""GPU: the PLONK verifier over BN254 on the device (nlx_bn254_plonk_vk_create, nlx_bn254_plonk_verify, _verify_batch) on the
instances and proofs of tools/gnark_bsb22_model.py: the model prover's bytes accepted, the DEVICE prover's bytes accepted (no
trapdoor arithmetic has touched the verifier's side of those), every named tamper rejected with the reason and index the model
with real pairings (tools/gnark_plonk_verify_model.py) gives, single-bit flips judged as that model judges them, batches equal
to single calls, the refusals.  Exact."""
import ctypes
import random

import numpy as np
import pytest

from bn254_plonk_verify_cases import ACCEPT, ALGEBRAIC, MALFORMED, PAIRING, R, bn, case, gm, parser_refuses, pm

pytestmark = pytest.mark.gpu
E_INVAL, E_RANGE = -1, -4


def _verdict(v):
    return int(v.accepted), int(v.reason), int(v.index)


@pytest.mark.parametrize("log_n,k", [(3, 0), (3, 1), (3, 2), (5, 0), (5, 1), (5, 2), (5, 4)])
def test_accepts_the_model_provers_proofs(nlx, ctx, log_n, k):
    c = case(log_n, k)
    assert len(c.proof) == 552 + 64 * k
    vk = c.verifying_key(nlx, ctx)
    v = vk.verify(c.proof, c.public)
    assert _verdict(v) == (1, ACCEPT, 0), str(v)
    assert v.raise_if_rejected() is v and str(v) == "accepted" and bool(v)
    vk.close()


@pytest.mark.parametrize("k", [0, 1])
def test_accepts_the_device_provers_proofs(nlx, ctx, k):
    """prove and verify on the device: bytes from prove_resident on a ResidentKey, the verifying key from the same key.  A changed
    public input changes gamma and PI(zeta): the relation fails before any pairing, as in the model."""
    P = nlx.bn254_plonk
    c = case(4, k)
    inst = c.inst
    key = P.ResidentKey(ctx, inst.key_values(), nlx.bn254_g1_pack(c.srs), inst.k1, inst.k2, commitments=inst.commitment_info())
    data = P.prove_resident(key, public_inputs=c.public, witness=inst.complete)          # random blinding
    g2 = lambda p: nlx.bn254_g2_pack([p])[0]
    vk = P.VerifyingKey.from_resident(key, g2(c.g2), g2(c.g2_tau), len(c.public))
    assert vk.k == k and c.trapdoor_accepts(data)
    assert _verdict(vk.verify(data, c.public)) == (1, ACCEPT, 0)
    changed = [(c.public[0] + 1) % R] + c.public[1:]
    assert c.model_verdict(data, changed) == (0, ALGEBRAIC, 0)
    v = vk.verify(data, changed)
    assert _verdict(v) == (0, ALGEBRAIC, 0) and str(v) == "rejected: the algebraic relation fails"
    vk.close()
    key.close()


@pytest.mark.parametrize("log_n,k", [(3, 0), (3, 1), (4, 2)])
def test_named_tampers(nlx, ctx, log_n, k):
    c = case(log_n, k)
    vk = c.verifying_key(nlx, ctx)
    tampers = c.tampers()
    got = vk.verify_many([t[1] for t in tampers], [t[2] for t in tampers])
    seen = set()
    for (label, data, public, reason, index), v in zip(tampers, got):
        want = c.model_verdict(data, public)
        print(label, want, _verdict(v))
        assert want[0] == 0 and (reason is None or want == (0, reason, index)), label
        assert _verdict(v) == want, (label, str(v))
        assert not c.trapdoor_accepts(data, public), label
        with pytest.raises(nlx.NlxError):
            v.raise_if_rejected()
        seen.add(want[1])
    assert {PAIRING, ALGEBRAIC, MALFORMED} <= seen
    names = {t[0]: str(v) for t, v in zip(tampers, got)}
    assert names["H2: x with no y"] == "rejected: malformed at H2" and names["Z: x = q"] == "rejected: malformed at Z"
    assert names["batched H replaced"] == "rejected: the pairing equation fails"
    assert names["l_zeta + 1"] == "rejected: the algebraic relation fails"
    assert names["claimed value 2 = r"] == "rejected: malformed at claimed value 2"
    assert names["one byte short"] == "rejected: malformed at the length or a count"
    vk.close()


def test_malformed_points_and_values_by_index(nlx, ctx):
    """every point and value field in turn: a flag byte of 0b00 on a point, r on a value; and the compressed point at infinity,
    which is a valid point (the verdict is then the model's)"""
    k = 2
    c = case(4, k)
    vk = c.verifying_key(nlx, ctx)
    points = ["l", "r", "o", "z", "h1", "h2", "h3"] + ["bsb22_%d" % j for j in range(k)] + ["batched_h", "z_shifted_h"]
    values = ["folded_h", "lin", "l_zeta", "r_zeta", "o_zeta", "s1_zeta", "s2_zeta"] + ["qcp%d_zeta" % j for j in range(k)] + ["z_shifted_value"]
    datas, want = [], []
    for i, name in enumerate(points):
        off = c.reg[name][0]
        b = bytearray(c.proof[off:off + 32])
        b[0] &= 0x3F
        datas.append(c.with_bytes(name, b))
        want.append((0, MALFORMED, i))
    for i, name in enumerate(values):
        datas.append(c.with_bytes(name, R.to_bytes(32, "big")))
        want.append((0, MALFORMED, 9 + k + i))
    for name in ("h3", "bsb22_1", "z_shifted_h"):
        datas.append(c.with_bytes(name, bytes([0x40]) + bytes(31)))
        want.append(c.model_verdict(datas[-1]))
        assert want[-1][1] != MALFORMED
        datas.append(c.with_bytes(name, bytes([0x40]) + bytes(30) + b"\x01"))
        want.append((0, MALFORMED, points.index(name)))
    got = vk.verify_many(datas, [c.public] * len(datas))
    assert [_verdict(v) for v in got] == want
    assert [c.model_verdict(d) for d in datas] == want
    vk.close()


@pytest.mark.parametrize("k", [0, 1])
def test_single_bit_flips_are_judged_as_the_model_judges_them(nlx, ctx, k):
    c = case(3, k)
    flips = c.bit_flips(24, 3300 + k)
    vk = c.verifying_key(nlx, ctx)
    got = vk.verify_many([d for _, d in flips], [c.public] * len(flips))
    vk.close()
    for (bit, data), v in zip(flips, got):
        if parser_refuses(data):
            assert (int(v.accepted), int(v.reason)) == (0, MALFORMED), bit
        assert _verdict(v) == c.model_verdict(data), (bit, str(v))


def _three_proofs(c):
    out = [c.proof]
    for _ in range(2):
        blinding = [c.rng.randrange(R) for _ in range(9)]
        out.append(gm.prove(c.inst, c.srs, blinding, [c.rng.randrange(R) for _ in range(2 * c.k)], tau=c.tau)[1])
    assert len(set(out)) == 3
    return out


@pytest.mark.parametrize("k", [0, 1])
def test_batches_equal_single_calls(nlx, ctx, k):
    c = case(3, k)
    vk = c.verifying_key(nlx, ctx)
    proofs = _three_proofs(c)
    tampers = {t[0]: t for t in c.tampers()}
    first, last, mid = tampers["batched H replaced"], tampers["H2: x with no y"], tampers["l_zeta + 1"]
    single = {}

    def one(data, public):
        key = (data, tuple(public))
        if key not in single:
            single[key] = _verdict(vk.verify(data, public))
        return single[key]

    for n in (1, 2, 64, 65):
        batch = [(proofs[i % 3], c.public) for i in range(n)]
        batch[0] = (first[1], first[2])
        if n > 1:
            batch[n - 1] = (last[1], last[2])
        if n > 2:
            batch[n // 2] = (mid[1], mid[2])
        got = vk.verify_many([b[0] for b in batch], [b[1] for b in batch])
        text = nlx.lib.dll.nlx_last_error(ctx.handle).decode()
        assert text.startswith("proof 0 rejected: the pairing equation fails"), text
        want = [one(*b) for b in batch]
        assert [_verdict(v) for v in got] == want, n
        assert want[0] == (0, PAIRING, 0) and sum(w[0] for w in want) == n - min(n, 3)
    # a batch whose first rejection is not at position 0
    got = vk.verify_many([proofs[0], proofs[1], last[1], first[1]], [c.public] * 4)
    assert [_verdict(v) for v in got] == [(1, 0, 0), (1, 0, 0), (0, MALFORMED, 5), (0, PAIRING, 0)]
    assert nlx.lib.dll.nlx_last_error(ctx.handle).decode().startswith("proof 2 rejected: malformed")
    vk.close()


def test_refusals(nlx, ctx):
    dll = nlx.lib.dll
    P = nlx.bn254_plonk
    c = case(3, 1)
    vk = c.verifying_key(nlx, ctx)
    verdict = P.Verdict(7, 7, 7)
    pub = nlx.bn254_pack([[bn.to_montgomery(x) for x in c.public]])[0]
    buf = ctypes.create_string_buffer(c.proof, len(c.proof))
    assert dll.nlx_bn254_plonk_verify(None, buf, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    assert dll.nlx_bn254_plonk_verify(vk.handle, None, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    assert dll.nlx_bn254_plonk_verify(vk.handle, buf, len(c.proof), pub.ctypes.data, None) == E_INVAL
    assert dll.nlx_bn254_plonk_verify(vk.handle, buf, len(c.proof), None, ctypes.byref(verdict)) == E_INVAL
    assert (verdict.accepted, verdict.reason, verdict.index) == (0, 0, 0)          # zero-filled first
    assert dll.nlx_bn254_plonk_verify_batch(vk.handle, None, None, 1, pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    h = ctypes.c_void_p()
    assert dll.nlx_bn254_plonk_vk_create(ctx.handle, None, ctypes.byref(h)) == E_INVAL
    assert dll.nlx_bn254_plonk_vk_create(None, None, ctypes.byref(h)) == E_INVAL
    dll.nlx_bn254_plonk_vk_destroy(None)
    assert dll.nlx_bn254_plonk_verify(vk.handle, buf, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == 0 and verdict.accepted == 1
    # a public scalar = r names the proof and the input
    with pytest.raises(nlx.NlxError) as e:
        vk.verify(c.proof, [c.public[0], R])
    assert e.value.code == E_RANGE and "proof 0, public input 1" in str(e.value)
    for x in (-1, (1 << 256) + 5):                                                 # never masked down to four words
        with pytest.raises(nlx.NlxError) as e:
            vk.verify(c.proof, [c.public[0], x])
        assert e.value.code == E_RANGE
        with pytest.raises(nlx.NlxError) as e:
            c.verifying_key(nlx, ctx, k1=x)
        assert e.value.code == E_RANGE
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, k2=R)
    assert e.value.code == E_RANGE
    # a G2 point outside the subgroup, a commitment off the curve, a row = n, too many public inputs, log_n out of range
    outside = nlx.bn254_g2_pack([pm.twist_point_outside_subgroup(random.Random(5))])[0]
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, g2_tau=outside)
    assert e.value.code == E_RANGE and "g2_tau) 1:" in str(e.value) and "subgroup" in str(e.value)
    bad = nlx.bn254_g1_pack(c.key_commitments())
    bad[3, 4] ^= np.uint64(1)
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, commitments=bad)
    assert e.value.code == E_RANGE and "g1) 3:" in str(e.value) and "curve" in str(e.value)
    for override in (dict(commit_rows=[c.n]), dict(n_public=c.n + 1), dict(log_n=2), dict(log_n=27)):
        with pytest.raises(nlx.NlxError) as e:
            c.verifying_key(nlx, ctx, **override)
        assert e.value.code == E_RANGE, override
    # verify after close() raises, and the context still answers
    vk.close()
    with pytest.raises(nlx.NlxError):
        vk.verify(c.proof, c.public)
    vk2 = c.verifying_key(nlx, ctx)
    assert vk2.verify(c.proof, c.public).accepted == 1
    vk2.close()
