"""The model of the device field multiply (tests/field_mul_model.py: the product chain whose third multiply-add may overflow,
and both reductions) against exact arithmetic, and the reach of the aimed operand set.  No GPU."""
import random

import field_mul_model as fm

P = fm.P


def test_known_hits_are_in_their_classes():
    assert len(fm.KNOWN_HITS) == len(fm.KNOWN_CLASSES) == len(set(fm.KNOWN_CLASSES)) == 9
    for (a, b), cls in zip(fm.KNOWN_HITS, fm.KNOWN_CLASSES):
        assert fm.classify(a, b) == cls, (hex(a), hex(b))
    # 0xffffffff00000002 * (2^64 - 1): w0 == w3 and w1 == 0, so the subtraction borrows because of k alone
    w0, w1, _, w3, k = fm.mul_chain(0xFFFFFFFF00000002, fm.M64)
    assert w0 == w3 and w1 == 0 and k == 1 and fm.classify(0xFFFFFFFF00000002, fm.M64)[1] == 1


def test_model_equals_exact_product_on_the_aimed_set():
    for a, b in fm.aimed_pairs():
        want = a * b % P
        r8, c8 = fm.mul8(a, b)
        r7, c7 = fm.mul7(a, b)
        assert r8 % P == want and r7 % P == want and fm.mul_parent(a, b) % P == want, (hex(a), hex(b))
        assert c8[:3] == c7[:3]
        # the two reductions differ only in the multiplier of EPS, and only where there was a borrow
        assert c8[1] == 1 or (r8 == r7 and c8 == c7)


def test_aimed_set_reaches_every_class_a_seeded_search_reaches():
    aimed = {fm.classify(a, b) for a, b in fm.aimed_pairs()}
    aimed8 = {fm.classify8(a, b) for a, b in fm.aimed_pairs()}
    assert set(fm.KNOWN_CLASSES) <= aimed
    for seed in (1, 2):
        found = fm.search_classes(100_000, seed)
        for cls, (a, b) in found.items():
            assert fm.mul7(a, b)[0] % P == a * b % P and fm.mul8(a, b)[0] % P == a * b % P
            assert cls in aimed, "the search reached %r at %#x * %#x and the aimed set does not" % (cls, a, b)
            assert fm.classify8(a, b) in aimed8
    # what is known to be reachable: k x borrow x final carry, and the rare case (w2 = 0 with a borrow) with k = 0
    assert {(k, b, 0, c) for k in (0, 1) for b in (0, 1) for c in (0, 1)} | {(0, 1, 1, 1)} <= aimed


def test_model_equals_exact_product_on_random_operands():
    rng = random.Random(7)
    for _ in range(50_000):
        a, b = rng.getrandbits(64), rng.getrandbits(64)
        want = a * b % P
        assert fm.mul8(a, b)[0] % P == want and fm.mul7(a, b)[0] % P == want


def test_reductions_on_any_limbs():
    """reduce160's use: four arbitrary limbs, with and without a k (w3 + k may then exceed 32 bits: the borrow chain takes it)"""
    rng = random.Random(11)
    words = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
    cases = [(a, b, c, d, k) for a in words for b in words for c in words for d in words for k in (0, 1)]
    cases += [tuple(rng.getrandbits(32) for _ in range(4)) + (rng.getrandbits(1),) for _ in range(20_000)]
    for w0, w1, w2, w3, k in cases:
        want = (w0 + (w1 << 32) + (w2 << 64) + ((w3 + k) << 96)) % P
        assert fm.reduce8(w0, w1, w2, w3, k)[0] % P == want
        assert fm.reduce7(w0, w1, w2, w3, k)[0] % P == want


def test_extension_product_on_the_chain():
    rng = random.Random(13)
    ops = [(a, b) for a, b in fm.aimed_pairs()[:400]]
    for i in range(3000):
        x = ops[rng.randrange(len(ops))] if i % 2 else (fm.structured(rng), fm.structured(rng))
        y = ops[rng.randrange(len(ops))] if i % 3 else (fm.structured(rng), fm.structured(rng))
        want = fm.ext_mul_exact(x, y)
        assert fm.ext_mul(x, y, fm.reduce8) == want and fm.ext_mul(x, y, fm.reduce7) == want
