"""The lazily reduced field forms of csrc/gl.hpp and GateAcc's fold, as Python integers (tests/lazy_field_model.py): no
intermediate outgrows its register, every result is congruent to the exact value, canonical where the device says so."""
import random

import lazy_field_model as m

P = m.P


def _check_ext(x, y):
    want = m.ext_mul_exact(x, y)
    got = m.ext_mul(x, y)
    assert got == want and got[0] < P and got[1] < P, (x, y)
    loose = m.ext_mul(x, y, canonical=False)
    assert loose[0] < (1 << 64) and loose[1] < (1 << 64) and (loose[0] % P, loose[1] % P) == want, (x, y)


def _check_reduce(w):
    want = m.reduce160_exact(w)
    assert m.reduce160(w) == want
    loose = m.reduce160(w, canonical=False)
    assert loose < (1 << 64) and loose % P == want


def test_extension_product_on_every_aimed_combination():
    cases = m.aimed_operands()
    assert len(cases) == 4096
    for a0, a1, b0, b1 in cases:
        _check_ext((a0, a1), (b0, b1))
        _check_ext((a0, a1), (b0, 0))          # the product by a base element, as an extension element


def test_reduce160_on_every_aimed_limb_pattern():
    for a0, a1, _b0, b1 in m.aimed_operands():
        _check_reduce(m.limbs_of(a0, a1, b1))
    for w in ([m.M32] * 5, [0, 0, 0, 0, m.M32], [0, 0, m.M32, 0, 0], [0, 0, 0, m.M32, 0], [1, 0, 0, m.M32, m.M32], [0] * 5):
        _check_reduce(w)


def test_random_loose_operands():
    rng = random.Random(160)
    for _ in range(4000):
        a0, a1, b0, b1 = (rng.getrandbits(64) for _ in range(4))
        _check_ext((a0, a1), (b0, b1))
        _check_reduce([rng.getrandbits(32) for _ in range(5)])
    for _ in range(1000):                        # loose operands just above p: the values a skipped reduction leaves behind
        a0, a1, b0, b1 = (P + rng.getrandbits(31) for _ in range(4))
        _check_ext((a0, a1), (b0, b1))


def test_accumulator_of_1024_all_ones_terms():
    acc = m.GateAccModel()
    for _ in range(1024):
        acc.mac(m.M64, m.M64)
    assert acc.fold() == (1024 * m.M64 * m.M64) % P
    assert max(acc.k) <= 1024


def test_three_limb_accumulator_takes_1024_all_ones_terms_without_carry_counters():
    acc = m.GateAcc3Model()
    ones = [(1 << 22) - 1] * 3                    # every limb all ones (the third limb of a real power has 20 bits: this is above it)
    for _ in range(m.GateAcc3Model.MAX_TERMS):
        acc.mac(m.M64, ones)                      # fits() inside asserts that no column outgrows its 64-bit pair
    assert max(acc.a) < 1 << 64
    assert acc.fold() == acc.exact % P
    try:                                          # and 1 024 is the bound: 64 more terms of the same size do overflow a column
        for _ in range(64):
            acc.mac(m.M64, ones)
        overflowed = False
    except AssertionError:
        overflowed = True
    assert overflowed


def test_three_limb_accumulator_on_random_terms():
    rng = random.Random(22)
    acc = m.GateAcc3Model()
    for n in range(1, 1025):
        b = rng.randrange(P)
        limbs = m.GateAcc3Model.limbs(b)
        assert sum(l << (22 * j) for j, l in enumerate(limbs)) == b and limbs[2] < 1 << 20
        acc.mac(rng.getrandbits(64), limbs)
        if n in (1, 2, 123, 1024):
            assert acc.fold() == acc.exact % P


def test_accumulator_on_random_terms():
    rng = random.Random(7)
    acc = m.GateAccModel()
    for n in range(1, 200):
        acc.mac(rng.getrandbits(64), rng.randrange(P))
        if n in (1, 2, 22, 123, 199):
            assert acc.fold() == acc.exact % P


# Run in a child interpreter, as build.py runs the generator (it stubs the package's ctypes layer).  The walker below knows the
# instruction words only: it folds one random value per emitted constraint by Horner, as the interpreter does, and compares the
# sum with the generator's exponents (airgen.segment_exponents) applied to the same values.
_EXPONENT_CHECK = r'''
import random, sys
sys.path.insert(0, %r)
import airgen
P = 0xFFFFFFFF00000001
rng = random.Random(3)
total = 0
for name, words in airgen.fixed_programs():
    words = airgen.canonical_words(words)
    for lo, hi in airgen._segments(words):
        alpha, acc, vals, i = rng.randrange(P), 0, [], lo
        while i < hi:
            w = int(words[i]); op = w & 0xFF
            n = {airgen.EMIT: 1, airgen.EMIT_FIRST: 1, airgen.EMIT_LAST: 1, airgen.EMIT_TRANSITION: 1, airgen.EMIT_LOGUP: 2,
                 airgen.EMIT_BOOL: ((w >> 40) & 0xFFFF) or 1}.get(op, 0)
            for _ in range(n):
                c = rng.randrange(P)
                acc = (acc * alpha + c) %% P
                vals.append(c)
            i += 2 if op == airgen.CONST else 1
        ex = airgen.segment_exponents(words, lo, hi)
        assert len(ex) == len(vals), (name, lo)
        assert sum(pow(alpha, e, P) * c for e, c in zip(ex, vals)) %% P == acc, (name, lo)
        assert not ex or max(ex) == len(ex) - 1
        total += len(ex)
print("constraints", total)
'''


def test_generator_exponents_reproduce_horner():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, "-c", _EXPONENT_CHECK % os.path.join(ROOT, "near-light-client_amd")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # 2 048 (SHA-256, tagged and untagged) + 4 952 (SHA-512) + 2 596 (Ed25519) constraints
    assert int(r.stdout.split()[-1]) == 2 * 2048 + 4952 + 2596
