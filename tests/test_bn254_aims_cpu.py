"""CPU: the aimed inputs of tests/bn254_aims.py are what they claim - checked with the big-integer model alone (oracle/bn254_py.py),
so that tests/test_gpu_bn254_aims.py compares the device with inputs that really reach the cases they name."""
import random

import pytest

import bn254_aims as aims

bn = aims.bn
R = aims.R
SHIFT, K1, K2 = 5, 5, 25


def test_word_aims_and_packing():
    assert len(aims.WORD_AIMS) == 10 and len({w for _, w in aims.WORD_AIMS}) == 10
    for (_, w), v in zip(aims.WORD_AIMS, aims.AIM_VALUES):
        assert bn.to_montgomery(v) == w
    limbs = aims.to_limbs((1 << 253) - 1)
    assert limbs[:8] == [(1 << 29) - 1] * 8 and aims.to_limbs(1 << 232) == [0] * 8 + [1]
    words = [w for _, w in aims.WORD_AIMS] + [(1 << 256) - 1]
    assert aims.unpack(aims.pack(words)) == words
    assert aims.unpack_mont(aims.pack_mont(aims.AIM_VALUES)) == aims.AIM_VALUES
    big = (1 << 261) - 12345
    assert aims.from_limbs(aims.to_limbs(big)) == (big, 1) and aims.from_limbs([1 << 29] + [0] * 8) == (1 << 29, 0)


@pytest.mark.parametrize("log_n", [3, 6])
def test_on_class_targets_appear_at_their_positions(log_n):
    """on_class: the polynomial has degree < n, and the 4n-coset evaluation the prover makes holds the chosen values at 4 k + c"""
    rng = random.Random(log_n)
    n = 1 << log_n
    for c in range(4):
        for shift in (SHIFT, rng.randrange(2, R)):
            chosen = [aims.aim_value(k + c) if k % 3 else rng.randrange(R) for k in range(n)]
            on_h = aims.on_class(chosen, c, log_n, shift)
            ev = bn.coset_evals(on_h, shift)
            assert [ev[4 * k + c] for k in range(n)] == chosen
            assert ev[4 * 1 + c] == bn.eval_poly(bn.ntt(on_h, inverse=True), aims.class_point(c, 1, log_n, shift))


@pytest.mark.parametrize("variant", ["plain", "pi", "blinded", "commit"])
@pytest.mark.parametrize("log_n", [3, 6])
def test_quotient_aims_hold_what_they_name(log_n, variant):
    rng = random.Random(10 * log_n + len(variant))
    n = 1 << log_n
    assert aims.coset_is_defined(log_n, SHIFT)                    # Z_H and x - 1 never vanish: the model divides by both
    assert not aims.coset_is_defined(log_n, bn.root_of_unity(log_n + 2))
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    for c in range(4):
        for aim in aims.QUOTIENT_AIMS:
            on_h, rows, k0 = aims.quotient_inputs(aim, variant, c, log_n, SHIFT, K1, K2, beta, gamma)
            assert len(on_h) == {"plain": 12, "pi": 13, "blinded": 12, "commit": 15}[variant]
            ev = {name: bn.coset_evals(v, SHIFT) for name, v in on_h.items()}
            i = 4 * k0 + c
            for name in on_h:
                assert [ev[name][4 * k + c] for k in range(n)] == rows[name], (aim, name)
            x = aims.class_point(c, k0, log_n, SHIFT)
            at = {name: ev[name][i] for name in on_h}
            z_next = ev["z"][(i + 4) % (4 * n)]
            f = [(at["l"] + beta * x + gamma) % R, (at["r"] + beta * K1 * x + gamma) % R, (at["o"] + beta * K2 * x + gamma) % R]
            h = [(at[w] + beta * at[s] + gamma) % R for w, s in (("l", "s1"), ("r", "s2"), ("o", "s3"))]
            if aim == "all zero":
                assert not any(at.values())
            elif aim == "all words r-1":
                assert {bn.to_montgomery(v) for v in at.values()} == {R - 1}
            elif aim == "l = -(beta x + gamma)":
                assert f[0] == 0 and h[0] != 0
            elif aim == "l = -(beta s1 + gamma)":
                assert h[0] == 0 and f[0] != 0
            elif aim.startswith("f = h"):
                assert f == h and at["z"] == z_next and all(f)
                assert (k0 == n - 1) == ("wraps" in aim) and (k0 < n - 1 or (i + 4) % (4 * n) == c)
            elif aim == "z = 1":
                assert at["z"] == 1
            elif aim == "z = 0":
                assert at["z"] == 0
            elif aim == "gate terms all r-1":
                assert {bn.to_montgomery(at[name]) for name in on_h if name in aims.GATE_TERMS} == {R - 1}
            # every other position holds WORD_AIMS words
            other = (k0 + 2) % n
            assert all(bn.to_montgomery(ev[name][4 * other + c]) in dict((w, 1) for _, w in aims.WORD_AIMS) for name in on_h)
        # the model is defined on these inputs and, the witnesses being no satisfying ones, reports a non-zero high chunk
        b = [rng.randrange(R) for _ in range(9)]
        want, high_zero = aims.quotient_model(on_h, variant, n, SHIFT, K1, K2, alpha, beta, gamma, b)
        assert len(want) == (4 * n if variant == "blinded" else 3 * n) and not high_zero


@pytest.mark.parametrize("log_n", [1, 2, 6, 7])
def test_grand_product_model_equals_the_witness_generators(log_n):
    rng = random.Random(300 + log_n)
    beta, gamma = rng.randrange(R), rng.randrange(R)
    p = bn.plonk_witness(log_n, rng, K1, K2, beta, gamma)
    assert aims.grand_product_model(p, beta, gamma, K1, K2) == (p["z"], True)
    z, closes = aims.grand_product_model(dict(p, s1=p["s2"], s2=p["s1"]), beta, gamma, K1, K2)
    assert not closes and z[0] == 1 and z != p["z"]


@pytest.mark.parametrize("log_n", [7, 13])
def test_zero_cases_zero_the_named_rows_and_no_other(log_n):
    rng = random.Random(400 + log_n)
    n = 1 << log_n
    beta, gamma = rng.randrange(R), rng.randrange(R)
    p = bn.plonk_witness(log_n, rng, K1, K2, beta, gamma)
    w = bn.root_of_unity(log_n)
    xs, x = [], 1
    for _ in range(n):
        xs.append(x)
        x = x * w % R
    cases = aims.gp_zero_cases(p, beta, gamma, K1, K2)
    assert len(cases) == 9
    seen_den = set()
    base = [aims.gp_factors(p, i, xs[i], beta, gamma, K1, K2) for i in range(n)]
    assert all(num and den for num, den in base)
    for name, q, den_rows, num_rows in cases:
        factors = list(base)
        for i in range(n):
            if any(q[k][i] != p[k][i] for k in ("l", "r", "o", "s1", "s2", "s3")):
                factors[i] = aims.gp_factors(q, i, xs[i], beta, gamma, K1, K2)
        assert [i for i in range(n) if factors[i][1] == 0] == den_rows, name
        assert [i for i in range(n) if factors[i][0] == 0] == num_rows, name
        seen_den.update(i % 64 for i in den_rows)
        z, closes = aims.grand_product_model(q, beta, gamma, K1, K2)
        first = min(den_rows + num_rows)
        assert not closes and z[:first + 1] == p["z"][:first + 1] and all(z[:first + 1]) and not any(z[first + 1:]), name
    assert {0, 63} <= seen_den and n - 1 in [r for c in cases for r in c[2]]
    if log_n == 13:
        assert min(r for c in cases for r in c[2] if r) >= 4096      # the second block of the ratio kernel
