"""CPU: how a PoseidonBN128 digest meets the Goldilocks transcript (rule 2 of tools/bn128_config_model.py): the limb split of the
model, and the library's host entry nlx_challenger_observe_hash against the model feeding the oracle's Challenger.  Needs no GPU."""
import ctypes
import os
import random
import sys

import numpy as np

from conftest import ROOT, P

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn128_config_model as cm  # noqa: E402

R = cm.R
NLX_E_RANGE = -4
GOLD, BN = 0, 1


def _words(v):
    return np.array(cm.m.to_words(v), dtype=np.uint64)


def test_limb_split_round_trip_and_bounds():
    rng = random.Random(5)
    for v in [0, 1, R - 1, R - 2, (1 << 56) - 1, 1 << 56, (1 << 224) - 1, 1 << 224] + [rng.randrange(R) for _ in range(200)]:
        limbs = cm.digest_limbs(v)
        assert len(limbs) == 5
        assert all(x < (1 << 56) for x in limbs[:4]) and limbs[4] < (1 << 32)
        assert all(x < P for x in limbs)                     # every limb is a canonical Goldilocks element
        assert cm.digest_from_limbs(limbs) == v
        assert sum(x << (56 * k) for k, x in enumerate(limbs)) == v
    assert cm.digest_limbs(R - 1)[4] == (R - 1) >> 224
    assert cm.flatten([1, R - 1]) == cm.digest_limbs(1) + cm.digest_limbs(R - 1)


class _Ch(ctypes.Structure):
    _fields_ = [("state", ctypes.c_uint64 * 12), ("in_buf", ctypes.c_uint64 * 8), ("n_in", ctypes.c_uint32), ("pad0", ctypes.c_uint32),
                ("out_buf", ctypes.c_uint64 * 8), ("n_out", ctypes.c_uint32), ("pad1", ctypes.c_uint32)]


def _same_state(a, b):
    return bytes(a) == bytes(b)


def test_observe_hash_equals_model_on_random_patterns(nlx, orc):
    dll = nlx.lib.dll
    rng = random.Random(6)
    edges = [0, 1, R - 1, R - 2, (1 << 224) - 1, 1 << 224, (1 << 56) - 1]
    for trial in range(40):
        c = _Ch()
        dll.nlx_challenger_init(ctypes.byref(c))
        ref = orc.Challenger()
        for _ in range(rng.randrange(1, 10)):
            k = rng.randrange(0, 20)
            ds = [rng.choice(edges) if trial % 3 == 0 and rng.random() < 0.4 else rng.randrange(R) for _ in range(k)]
            if k:
                w = np.concatenate([_words(d) for d in ds])
                assert dll.nlx_challenger_observe_hash(ctypes.byref(c), w.ctypes.data, k, BN) == 0
                for d in ds:
                    for x in cm.digest_limbs(d):
                        ref.observe(x)
            else:
                assert dll.nlx_challenger_observe_hash(ctypes.byref(c), None, 0, BN) == 0
            if rng.random() < 0.5:   # plain elements in between, as the transcript has them
                xs = np.array([rng.randrange(P) for _ in range(rng.randrange(1, 9))], dtype=np.uint64)
                assert dll.nlx_challenger_observe(ctypes.byref(c), xs.ctypes.data, xs.size) == 0
                for x in xs:
                    ref.observe(int(x))
            n = rng.randrange(0, 11)
            out = np.zeros(max(n, 1), dtype=np.uint64)
            assert dll.nlx_challenger_challenge(ctypes.byref(c), out.ctypes.data, n) == 0
            assert [int(v) for v in out[:n]] == [ref.challenge() for _ in range(n)]


def test_observe_hash_goldilocks_is_observe_of_the_four_words(nlx):
    dll = nlx.lib.dll
    rng = np.random.default_rng(7)
    a, b = _Ch(), _Ch()
    dll.nlx_challenger_init(ctypes.byref(a))
    dll.nlx_challenger_init(ctypes.byref(b))
    for k in (1, 3, 16, 5):
        d = rng.integers(0, P, (k, 4), dtype=np.uint64)
        assert dll.nlx_challenger_observe_hash(ctypes.byref(a), d.ctypes.data, k, GOLD) == 0
        assert dll.nlx_challenger_observe(ctypes.byref(b), d.ctypes.data, 4 * k) == 0
        assert _same_state(a, b)
        oa, ob = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
        dll.nlx_challenger_challenge(ctypes.byref(a), oa.ctypes.data, 3)
        dll.nlx_challenger_challenge(ctypes.byref(b), ob.ctypes.data, 3)
        assert np.array_equal(oa, ob)
    bad = np.array([[1, 2, P, 3]], dtype=np.uint64)   # a Goldilocks digest word must be canonical, as in nlx_challenger_observe
    assert dll.nlx_challenger_observe_hash(ctypes.byref(a), bad.ctypes.data, 1, GOLD) == NLX_E_RANGE


def test_observe_hash_refuses_digests_not_below_r_and_unknown_hashers(nlx):
    dll = nlx.lib.dll
    c = _Ch()
    dll.nlx_challenger_init(ctypes.byref(c))
    ok = _words(R - 1)
    assert dll.nlx_challenger_observe_hash(ctypes.byref(c), ok.ctypes.data, 1, BN) == 0
    before = bytes(c)
    for v in (R, R + 1, (1 << 256) - 1):
        w = np.concatenate([_words(5), np.array(cm.m.to_words(v), dtype=np.uint64)])   # the second of two digests is bad
        assert dll.nlx_challenger_observe_hash(ctypes.byref(c), w.ctypes.data, 2, BN) == NLX_E_RANGE
        assert bytes(c) == before                                                      # nothing observed
    assert dll.nlx_challenger_observe_hash(ctypes.byref(c), ok.ctypes.data, 1, 7) == NLX_E_RANGE
    assert bytes(c) == before


def test_python_mirror_observe_hash(nlx, orc):
    ch = nlx.plonk.Challenger()
    ref = orc.Challenger()
    ds = [3, R - 1, 1 << 200]
    ch.observe_hash(np.array([cm.m.to_words(d) for d in ds], dtype=np.uint64), "poseidon_bn128")
    for x in cm.flatten(ds):
        ref.observe(x)
    assert [int(v) for v in ch.challenges(4)] == [ref.challenge() for _ in range(4)]
    try:
        ch.observe_hash(np.array([cm.m.to_words(R)], dtype=np.uint64), "poseidon_bn128")
    except nlx.NlxError as e:
        assert e.code == NLX_E_RANGE
    else:
        raise AssertionError("a digest equal to r was observed")


def test_circuit_digest_rule_uses_five_limbs_per_digest():
    """rule 4 in the model: the preimage is 5 limbs per cap digest, 5 for the domain separator's digest, then degree_bits"""
    cap = [7, R - 1, 1 << 130, 12345]
    inner = cm.m.hash_no_pad(cm.DOMAIN_SEPARATOR_PADDED)
    pre = cm.flatten(cap) + cm.digest_limbs(inner) + [9]
    assert len(pre) == 5 * len(cap) + 5 + 1
    assert cm.circuit_digest(cap, 9) == cm.m.hash_no_pad(pre)
    assert cm.circuit_digest(cap, 9) != cm.circuit_digest(cap, 10)
