"""CPU: the pure-Python BN254 model (oracle/bn254_py.py) is an NTT - definition, inverse, Montgomery helpers."""
import random


def test_model_definition_and_inverse():
    import bn254_py as bn
    rng = random.Random(1)
    for log_n in (0, 1, 3, 6):
        n = 1 << log_n
        a = [rng.randrange(bn.R) for _ in range(n)]
        v = bn.ntt(a)
        w = bn.root_of_unity(log_n)
        for k in range(min(n, 5)):
            assert v[k] == sum(a[j] * pow(w, j * k, bn.R) for j in range(n)) % bn.R == bn.eval_poly(a, pow(w, k, bn.R))
        assert bn.ntt(v, inverse=True) == a
    assert bn.from_montgomery(bn.to_montgomery(12345)) == 12345 and bn.to_montgomery(1) == (1 << 256) % bn.R
    assert pow(bn.root_of_unity(28), 1 << 28, bn.R) == 1 and pow(bn.root_of_unity(28), 1 << 27, bn.R) != 1


def test_g1_model():
    """the G1 half of the model: group law, order, EIP-196's doubling of the generator, MSM = the sum of its terms"""
    import bn254_py as bn
    g = bn.G1
    assert (g[1] ** 2 - g[0] ** 3 - 3) % bn.Q == 0
    assert bn.g1_mul(bn.R, g) is None and bn.g1_mul(bn.R - 1, g) == bn.g1_neg(g) and bn.g1_add(g, bn.g1_neg(g)) is None
    assert bn.g1_mul(2, g) == bn.g1_add(g, g) and bn.g1_mul(7, g) == bn.g1_add(bn.g1_mul(3, g), bn.g1_mul(4, g))
    rng = random.Random(2)
    pts = [bn.g1_mul(rng.randrange(bn.R), g) for _ in range(5)]
    ks = [rng.randrange(bn.R) for _ in range(5)]
    for p in pts:
        assert (p[1] ** 2 - p[0] ** 3 - 3) % bn.Q == 0
    # linearity in the scalars, and against the discrete logs
    assert bn.msm_g1(ks, pts) == bn.g1_add(bn.msm_g1(ks[:2], pts[:2]), bn.msm_g1(ks[2:], pts[2:]))
    logs = [rng.randrange(bn.R) for _ in range(4)]
    assert bn.msm_g1(ks[:4], [bn.g1_mul(a, g) for a in logs]) == bn.g1_mul(sum(k * a for k, a in zip(ks, logs)) % bn.R, g)


def test_f29_field_code_built_for_the_host(tmp_path):
    """csrc/bn254_f29.hpp (the MSM kernels' arithmetic on nine 29-bit limbs), compiled with g++: every operation equals the
    big-integer computation and stays inside the bounds its header states - on random operands and on the extremes of the
    allowed ranges"""
    import os
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "f29check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bn254_f29_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    import bn254_aims as aims
    cases = aims.f29_cases(random.Random(29))         # the device runs the same list (tests/test_gpu_bn254_aims.py)
    assert {(c[0], c[1]) for c in cases} == {(m, op) for m in "qr" for op in ("mul", "add", "sub4", "sub8", "tighten", "canonical", "iszero",
                                                                                "frommont", "words", "tocanon")} | {("r", "x32")}
    text = "".join("%s %s %x %x\n" % c for c in cases)
    out = subprocess.run([exe], input=text, text=True, capture_output=True, check=True).stdout.split("\n")
    assert len(out) >= len(cases)
    for case, line in zip(cases, out):
        val, normalised = line.split()
        aims.f29_check(case, int(val, 16), int(normalised))     # value, bound and limb normalisation, as Python integers


def test_fp_field_code_built_for_the_host(tmp_path):
    """csrc/bn254_fp.hpp (the eight-limb Montgomery arithmetic behind the MSM's tail, the NTT's tables, the Groth16 rows and every
    range check of a caller's scalars), compiled with g++: for both moduli, every operation equals the big-integer computation
    on random operands and on 0, 1, p - 1 and R mod p, and below_mod draws the line exactly at p, word by word"""
    import os
    import subprocess
    import bn254_py as bn
    from conftest import ROOT
    exe = str(tmp_path / "fpcheck")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bn254_fp_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    big_r = 1 << 256
    rng = random.Random(8)
    cases = []
    for name, p in (("q", bn.Q), ("r", bn.R)):
        special = [0, 1, p - 1, big_r % p]
        ops = [rng.randrange(p) for _ in range(200)] + special
        for a in ops:
            for op in ("add", "sub", "mul"):
                cases.append((name, op, a, rng.choice(ops)))
            for op in ("neg", "tomont", "frommont", "inv"):
                cases.append((name, op, a, 0))
            cases.append((name, "pow", a, rng.choice([rng.getrandbits(64), rng.randrange(1 << 16), 0, 1, 2, (1 << 64) - 1])))
        for a in special:
            for b in special:
                for op in ("add", "sub", "mul"):
                    cases.append((name, op, a, b))
        # the comparison: around p, the top of the range, and p with exactly one of its four words one above or below
        for v in [p - 1, p, p + 1, big_r - 1, 0] + [p + s * (1 << (64 * k)) for k in range(4) for s in (1, -1)]:
            cases.append((name, "below", v, 0))
    text = "".join("%s %s %x %x\n" % c for c in cases)
    out = subprocess.run([exe], input=text, text=True, capture_output=True, check=True).stdout.split()
    assert len(out) == len(cases)
    for (name, op, a, b), line in zip(cases, out):
        p = bn.Q if name == "q" else bn.R
        r_inv = pow(big_r, -1, p)
        got = int(line, 16)
        want = {"add": lambda: (a + b) % p, "sub": lambda: (a - b) % p, "neg": lambda: -a % p, "mul": lambda: a * b * r_inv % p,
                "tomont": lambda: a * big_r % p, "frommont": lambda: a * r_inv % p,
                "inv": lambda: pow(a, -1, p) * big_r * big_r % p if a else 0,                  # (x R)^-1 in Montgomery form: R / x
                "pow": lambda: pow(a * r_inv, b, p) * big_r % p,                               # (x R)^b: x^b R
                "below": lambda: 1 if a < p else 0}[op]()
        assert got == want, (name, op, hex(a), hex(b))


def test_g1_sum_on_the_host(nlx):
    """nlx_bn254_g1_sum (host code of the MSM's tail, no GPU): sums of G1Affine words equal the model's, infinity included"""
    import bn254_py as bn
    rng = random.Random(3)
    pts = [bn.g1_mul(rng.randrange(1, bn.R), bn.G1) for _ in range(6)]
    for chosen in (pts, pts[:1], [], [pts[0], bn.g1_neg(pts[0])], [pts[1], pts[1], None, pts[2]]):
        want = None
        for p in chosen:
            want = bn.g1_add(want, p)
        assert nlx.bn254_g1_unpack(nlx.bn254_g1_sum(nlx.bn254_g1_pack(chosen))) == want


def test_g2_model_and_host_sum(nlx):
    """the G2 half of the model (EIP-197's generator: on the twist, of order r) and nlx_bn254_g2_sum (host code, no GPU)"""
    import bn254_py as bn
    g = bn.G2
    assert bn.g2_mul(bn.R, g) is None and bn.g2_mul(bn.R - 1, g) == bn.g2_neg(g) and bn.g2_add(g, bn.g2_neg(g)) is None
    assert bn.g2_mul(7, g) == bn.g2_add(bn.g2_mul(3, g), bn.g2_mul(4, g))
    rng = random.Random(4)
    pts = [bn.g2_mul(rng.randrange(1, bn.R), g) for _ in range(4)]
    for chosen in (pts, pts[:1], [], [pts[0], bn.g2_neg(pts[0])], [pts[1], pts[1], None, pts[2]]):
        want = None
        for p in chosen:
            want = bn.g2_add(want, p)
        assert nlx.bn254_g2_unpack(nlx.bn254_g2_sum(nlx.bn254_g2_pack(chosen))) == want


def test_plonk_quotient_model_and_kzg_division():
    """the big-integer model behind tests/test_gpu_bn254_plonk.py: a satisfying three-wire instance divides by Z_H (the quotient
    has degree < 3n), a broken gate or a broken copy does not; synthetic division satisfies p = q (X - zeta) + p(zeta)"""
    import random
    import bn254_py as bn
    rng = random.Random(21)
    k1, k2 = 5, 25
    alpha, beta, gamma = (rng.randrange(bn.R) for _ in range(3))
    for log_n in (2, 4):
        n = 1 << log_n
        p = bn.plonk_witness(log_n, rng, k1, k2, beta, gamma)
        t = bn.plonk_quotient(p, 5, k1, k2, alpha, beta, gamma)
        assert not any(t[3 * n:]) and any(t[:3 * n])
        bad = bn.plonk_witness(log_n, rng, k1, k2, beta, gamma, satisfied=False)
        assert any(bn.plonk_quotient(bad, 5, k1, k2, alpha, beta, gamma)[3 * n:])
        swapped = dict(p, s1=p["s2"], s2=p["s1"])             # a different permutation: z no longer matches it
        assert any(bn.plonk_quotient(swapped, 5, k1, k2, alpha, beta, gamma)[3 * n:])
    coeffs = [rng.randrange(bn.R) for _ in range(37)]
    zeta = rng.randrange(bn.R)
    y, q = bn.kzg_open(coeffs, zeta)
    assert y == bn.eval_poly(coeffs, zeta) and len(q) == 36
    back = [0] * 37
    for i, qi in enumerate(q):
        back[i + 1] = (back[i + 1] + qi) % bn.R
        back[i] = (back[i] - zeta * qi) % bn.R
    back[0] = (back[0] + y) % bn.R
    assert back == coeffs
