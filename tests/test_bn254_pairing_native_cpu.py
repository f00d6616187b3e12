"""CPU tests: csrc/bn254_pairing.hpp built with plain g++ (tests/native/bn254_pairing_check.cpp) against the big-integer model
tools/bn254_pairing_model.py - the tower on extreme and random operands, the Miller loop and the final exponentiation on random
pairs, points at infinity, the subgroup test.  The program is built twice: plainly, and with -fsanitize=address,undefined (that
stand-alone binary is run; skipped where a trivial sanitized program does not link)."""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_pairing_model as pm  # noqa: E402

bn = pm.bn
Q, R = pm.Q, pm.R
MONT = 1 << 256
SRC = os.path.join(ROOT, "tests", "native", "bn254_pairing_check.cpp")
INCLUDE = os.path.join(ROOT, "near-light-client_amd", "csrc")


def hx(x):
    return "%064x" % x


def mont(values):
    return " ".join(hx(v * MONT % Q) for v in values)


def canon(values):
    return " ".join(hx(v % Q) for v in values)


def f12_words(a):
    return mont(pm.f12_to_gnark(a))


def f12_expect(a):
    return canon(pm.f12_to_gnark(a))


def g1_words(p):
    return mont((0, 0) if p is None else p)


def g2_words(q2):
    return mont((0, 0, 0, 0) if q2 is None else (q2[0][0], q2[0][1], q2[1][0], q2[1][1]))


def frobenius(a, k):
    return pm.f12_pow(a, Q**k)


def conj(a):
    return pm.f12_pow(a, Q**6)


def cyclotomic(a):
    """a^((q^6 - 1)(q^2 + 1)): an element of the cyclotomic subgroup"""
    t = pm.f12_mul(conj(a), pm.f12_inv(a))
    return pm.f12_mul(frobenius(t, 2), t)


@pytest.fixture(scope="module")
def cases():
    rng = random.Random(254)
    rnd12 = lambda: pm.f12_from_gnark([rng.randrange(Q) for _ in range(12)])
    all0, all1, allm = pm.f12_from_gnark([0] * 12), pm.f12_from_gnark([1] * 12), pm.f12_from_gnark([Q - 1] * 12)
    operands = [all0, all1, allm, rnd12(), rnd12(), rnd12()]
    lines = []
    for a in operands:
        for b in operands:
            lines.append("mul %s %s = %s" % (f12_words(a), f12_words(b), f12_expect(pm.f12_mul(a, b))))
        lines.append("sqr %s = %s" % (f12_words(a), f12_expect(pm.f12_mul(a, a))))
        lines.append("conj %s = %s" % (f12_words(a), f12_expect(conj(a))))
        for k in (1, 2, 3):
            lines.append("frob%d %s = %s" % (k, f12_words(a), f12_expect(frobenius(a, k))))
        if a != all0:
            lines.append("inv %s = %s" % (f12_words(a), f12_expect(pm.f12_inv(a))))
        for l in ([0] * 6, [1] * 6, [Q - 1] * 6, [rng.randrange(Q) for _ in range(6)]):
            sparse = [0] * 12                     # l0 at C0.B0, l1 at C1.B0, l2 at C1.B1 (E12 order: pairs 0, 3, 4)
            sparse[0:2], sparse[6:8], sparse[8:10] = l[0:2], l[2:4], l[4:6]
            lines.append("line %s %s = %s" % (f12_words(a), mont(l), f12_expect(pm.f12_mul(a, pm.f12_from_gnark(sparse)))))
    for a in operands[1:]:
        c = cyclotomic(a)
        assert pm.f12_pow(c, Q**4 - Q**2 + 1) == pm.F12_ONE
        lines.append("cyc %s = %s" % (f12_words(c), f12_expect(pm.f12_mul(c, c))))
    c = cyclotomic(operands[3])
    lines.append("expx %s = %s" % (f12_words(c), f12_expect(pm.f12_pow(c, pm.X))))
    a = operands[4]
    lines.append("finalexp %s = %s" % (f12_words(a), f12_expect(pm.final_exponentiation(a))))
    for _ in range(4):
        p, q2 = bn.g1_mul(rng.randrange(1, R), bn.G1), bn.g2_mul(rng.randrange(1, R), bn.G2)
        f = pm.miller_loop(p, q2)
        lines.append("miller %s %s %s = " % (g1_words(p), g2_words(q2), f12_words(f)))
        lines.append("pairing %s %s = %s" % (g1_words(p), g2_words(q2), f12_expect(pm.final_exponentiation(f))))
    p, q2 = bn.g1_mul(5, bn.G1), bn.g2_mul(7, bn.G2)
    for pp, qq in ((None, q2), (p, None), (None, None)):
        lines.append("miller_is_one %s %s = " % (g1_words(pp), g2_words(qq)))
        lines.append("pairing %s %s = %s" % (g1_words(pp), g2_words(qq), f12_expect(pm.F12_ONE)))
    outside = pm.twist_point_outside_subgroup(rng)
    assert pm.g2_on_curve(outside) and not pm.g2_in_subgroup(outside)
    off_curve2 = (q2[0], bn.f2_add(q2[1], (1, 0)))
    checks = [((p, q2), 0), ((None, q2), 0), ((p, None), 0), ((bn.G1, bn.G2), 0), ((p, bn.g2_mul(R - 1, bn.G2)), 0),
              (((p[0], (p[1] + 1) % Q), q2), 2), ((p, off_curve2), 4), ((p, outside), 5)]
    for (pp, qq), status in checks:
        lines.append("check %s %s = %s" % (g1_words(pp), g2_words(qq), hx(status)))
    # a coordinate equal to q (words that are no residue): the range checks
    lines.append("check %s %s %s = %s" % (hx(Q), hx(p[1] * MONT % Q), g2_words(q2), hx(1)))
    g2w = g2_words(q2).split()
    lines.append("check %s %s = %s" % (g1_words(p), " ".join(g2w[:3] + [hx(Q)]), hx(3)))
    return "\n".join(lines) + "\n"


def _build(tmp, name, extra):
    exe = tmp / name
    r = subprocess.run(["g++", "-std=c++17", "-I", INCLUDE] + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(exe, cases, tmp):
    path = tmp / "cases.txt"
    path.write_text(cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("%d cases, 0 bad" % cases.count("\n"))


def test_header_against_the_model(cases, tmp_path):
    _run(_build(tmp_path, "bn254_pairing_check", ["-O2"]), cases, tmp_path)


def test_header_under_sanitizers(cases, tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    try:
        r = subprocess.run(["g++", "-std=c++17"] + san + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True)
        ok = r.returncode == 0 and subprocess.run([str(tmp_path / "trivial")], capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip("a trivial program does not link with -fsanitize=address,undefined here")
    _run(_build(tmp_path, "bn254_pairing_check_san", san), cases, tmp_path)
