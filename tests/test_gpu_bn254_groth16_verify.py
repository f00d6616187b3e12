"""GPU: the Groth16 verifier on the device (nlx_bn254_groth16_vk_create, nlx_bn254_groth16_verify, _verify_batch) on the keys
and proofs of tools/groth16_model.py and tools/groth16_commit_model.py: honest proofs of every shape accepted, proofs of the
DEVICE prover accepted (no trapdoor arithmetic has touched those), every named tamper rejected with its reason and point,
single-bit flips judged as the model's pairing verifier judges them, batches equal to single calls, the refusals.  Exact."""
import ctypes
import random

import numpy as np
import pytest

from groth16_verify_cases import ACCEPT, MALFORMED, PAIRING, R, Case, case, cm, gm

pytestmark = pytest.mark.gpu
E_INVAL, E_RANGE = -1, -4


def _verdict(v):
    return int(v.accepted), int(v.reason), int(v.index)


@pytest.mark.parametrize("n_constraints", [8, 64])
@pytest.mark.parametrize("shape", sorted(gm.SHAPES))
def test_accepts_honest_proofs(nlx, ctx, shape, n_constraints):
    for k in range(4):
        c = case(shape, n_constraints, k)
        assert len(c.proof) == 164 + 32 * k
        vk = c.verifying_key(nlx, ctx)
        v = vk.verify(c.proof, c.public)
        assert _verdict(v) == (1, ACCEPT, 0), (k, str(v))
        assert v.raise_if_rejected() is v and str(v) == "accepted" and bool(v)
        vk.close()


@pytest.mark.parametrize("k", [0, 1])
def test_accepts_the_device_provers_proofs(nlx, ctx, k):
    """prove and verify on the device: bytes from nlx_bn254_groth16_prove(_committed) through proof_bytes"""
    from test_gpu_bn254_groth16_commit import _key_args
    g16 = nlx.bn254_groth16
    c = case("public3", 8, k)
    key = g16.ProvingKey(ctx, **_key_args(nlx, g16, c.inst, c.pk))
    if k == 0:
        data = g16.proof_bytes(*g16.prove(key, g16.fr_pack(c.w), c.r, c.s))
    else:
        data = g16.proof_bytes(*g16.prove_committed(key, g16.fr_pack(c.w), c.r, c.s))
    key.close()
    vk = c.verifying_key(nlx, ctx)
    assert _verdict(vk.verify(data, c.public)) == (1, ACCEPT, 0)
    changed = list(c.public)
    changed[0] = (changed[0] + 1) % R
    assert _verdict(vk.verify(data, changed))[:2] == (0, PAIRING)
    vk.close()


@pytest.mark.parametrize("shape,k", [("public3", 0), ("all_b", 1), ("common", 2), ("public3", 3)])
def test_named_tampers(nlx, ctx, shape, k):
    c = case(shape, 8, k)
    vk = c.verifying_key(nlx, ctx)
    tampers = c.tampers()
    got = vk.verify_many([t[1] for t in tampers], [t[2] for t in tampers])
    for (label, data, public, reason, index), v in zip(tampers, got):
        assert _verdict(v) == (0, reason, index), (label, str(v))
        assert not c.trapdoor_accepts(data, public), label
        with pytest.raises(nlx.NlxError):
            v.raise_if_rejected()
        assert str(v).startswith("rejected: ")
    names = {t[0]: str(v) for t, v in zip(tampers, got)}
    assert names["Bs outside the subgroup"] == "rejected: malformed at Bs" and names["Krs: x with no y"] == "rejected: malformed at Krs"
    assert "pairing" in names["Ar replaced"] and (k == 0 or "Pedersen" in names["Pok replaced"])
    assert names["Pok: x = q"] == "rejected: malformed at Pok"                     # the verdict knows the key's k
    vk.close()


@pytest.mark.parametrize("k", [0, 1])
def test_single_bit_flips_are_judged_as_the_model_judges_them(nlx, ctx, k):
    c = case("public3", 8, k)
    rng = random.Random(3200 + k)
    flipped = []
    for _ in range(32):
        data = bytearray(c.proof)
        bit = rng.randrange(8 * len(data))
        data[bit >> 3] ^= 1 << (bit & 7)
        flipped.append(bytes(data))
    vk = c.verifying_key(nlx, ctx)
    got = vk.verify_many(flipped, [c.public] * len(flipped))
    vk.close()
    for data, v in zip(flipped, got):
        try:
            cm.proof_from_bytes(data)
            decodes = True
        except (AssertionError, ValueError):
            decodes = False
        if not decodes:
            assert (int(v.accepted), int(v.reason)) == (0, MALFORMED)
        else:
            assert bool(v.accepted) == c.model_accepts(data), str(v)


def _three_proofs(c):
    out = [c.proof]
    for _ in range(2):
        r, s = c.rng.randrange(R), c.rng.randrange(R)
        pts = gm.prove_by_logs(c.inst, c.td, c.w, r, s) + ([], None) if c.k == 0 else cm.prove_by_logs(c.inst, c.td, c.w, r, s)
        out.append(Case.bytes_of(list(pts)))
    assert len(set(out)) == 3
    return out


@pytest.mark.parametrize("k", [0, 1])
def test_batches_equal_single_calls(nlx, ctx, k):
    c = case("public3", 8, k)
    vk = c.verifying_key(nlx, ctx)
    proofs = _three_proofs(c)
    tampers = {t[0]: t for t in c.tampers()}
    first = tampers["Ar replaced"]
    last = tampers["Pok replaced" if k else "Krs: x with no y"]
    changed = tampers["public input changed"]
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
            batch[n // 2] = (changed[1], changed[2])
        got = vk.verify_many([b[0] for b in batch], [b[1] for b in batch])
        text = nlx.lib.dll.nlx_last_error(ctx.handle).decode()
        assert text.startswith("proof 0 rejected: the pairing equation fails"), text
        want = [one(*b) for b in batch]
        assert [_verdict(v) for v in got] == want, n
        assert want[0] == (0, PAIRING, 0) and sum(w[0] for w in want) == n - min(n, 3)
    # a batch whose first rejection is not at position 0
    got = vk.verify_many([proofs[0], proofs[1], last[1]], [c.public] * 3)
    assert [int(v.accepted) for v in got] == [1, 1, 0]
    assert nlx.lib.dll.nlx_last_error(ctx.handle).decode().startswith("proof 2 rejected")
    vk.close()


def test_refusals(nlx, ctx):
    dll = nlx.lib.dll
    c = case("public3", 8, 1)
    vk = c.verifying_key(nlx, ctx)
    verdict = nlx.bn254_groth16.Verdict(7, 7, 7)
    pub = nlx.bn254_groth16.fr_pack(c.public)
    buf = ctypes.create_string_buffer(c.proof, len(c.proof))
    assert dll.nlx_bn254_groth16_verify(None, buf, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    assert dll.nlx_bn254_groth16_verify(vk.handle, None, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    assert dll.nlx_bn254_groth16_verify(vk.handle, buf, len(c.proof), pub.ctypes.data, None) == E_INVAL
    assert dll.nlx_bn254_groth16_verify(vk.handle, buf, len(c.proof), None, ctypes.byref(verdict)) == E_INVAL
    assert (verdict.accepted, verdict.reason, verdict.index) == (0, 0, 0)          # zero-filled first
    assert dll.nlx_bn254_groth16_verify_batch(vk.handle, None, None, 1, pub.ctypes.data, ctypes.byref(verdict)) == E_INVAL
    h = ctypes.c_void_p()
    assert dll.nlx_bn254_groth16_vk_create(ctx.handle, None, ctypes.byref(h)) == E_INVAL
    assert dll.nlx_bn254_groth16_vk_create(None, None, ctypes.byref(h)) == E_INVAL
    dll.nlx_bn254_groth16_vk_destroy(None)
    assert dll.nlx_bn254_groth16_verify(vk.handle, buf, len(c.proof), pub.ctypes.data, ctypes.byref(verdict)) == 0 and verdict.accepted == 1
    # a public scalar = r
    with pytest.raises(nlx.NlxError) as e:
        vk.verify(c.proof, [c.public[0], R])
    assert e.value.code == E_RANGE and "public input 2" in str(e.value)
    for x in (-1, (1 << 256) + 5):                                                 # never masked down to four words
        with pytest.raises(nlx.NlxError) as e:
            vk.verify(c.proof, [c.public[0], x])
        assert e.value.code == E_RANGE
    # a verifying key whose ic count disagrees, an id outside the public wires, a point off the curve
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, n_ic=len(c.vk["ic"]) - 1)
    assert e.value.code == E_RANGE
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, commitments=[{"public": [c.inst.n_public]}])
    assert e.value.code == E_RANGE
    bad_ic = nlx.bn254_g1_pack(c.vk["ic"])
    bad_ic[1, 4] ^= np.uint64(1)
    with pytest.raises(nlx.NlxError) as e:
        c.verifying_key(nlx, ctx, ic=bad_ic)
    assert e.value.code == E_RANGE and "ic) 2:" in str(e.value)           # alpha is point 0, ic[1] point 2
    # verify after close() raises, and the context still answers
    vk.close()
    with pytest.raises(nlx.NlxError):
        vk.verify(c.proof, c.public)
    vk2 = c.verifying_key(nlx, ctx)
    assert vk2.verify(c.proof, c.public).accepted == 1
    vk2.close()
