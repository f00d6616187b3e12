"""CPU tests: csrc/bn254_codec.hpp built with plain g++ (tests/native/bn254_codec_check.cpp) against the big-integer model
tools/gnark_bytes_model.py - square roots in Fq and Fq2 of squares and of non-squares, the "largest" rule on aimed values (the
Fq2 branch with A1 = 0 can only be aimed at here: no curve point with it is at hand), byte parsing at the edges of the range,
and whole points both ways in both modes.  The program is built twice: plainly, and with -fsanitize=address,undefined (that
stand-alone binary is run; skipped where a trivial sanitized program does not link)."""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_py as bn  # noqa: E402
import gnark_bytes_model as gb  # noqa: E402

Q, R = gb.Q, gb.R
MONT = 1 << 256
SRC = os.path.join(ROOT, "tests", "native", "bn254_codec_check.cpp")
INCLUDE = os.path.join(ROOT, "near-light-client_amd", "csrc")
HALF_LO, HALF_HI = (Q - 1) // 2, (Q + 1) // 2


def hx(x):
    return "%064x" % x


def mont(*values):
    return " ".join(hx(v % Q * MONT % Q) for v in values)


def chunks(data):
    return " ".join(data[i:i + 32].hex() for i in range(0, len(data), 32))


def words_as_numbers(words):
    return " ".join(hx(sum(int(words[4 * i + k]) << (64 * k) for k in range(4))) for i in range(len(words) // 4))


def small(y):
    return Q - y if gb.fq_largest(y) else y


def small2(y):
    return ((-y[0]) % Q, (-y[1]) % Q) if gb.f2_largest(y) else y


def dec_line(g2, raw, data, subgroup=True):
    if g2:
        st, p = gb.g2_decode(data, raw, subgroup)
        return "g2dec %x %x %s = %s %s" % (raw, subgroup, chunks(data), hx(st), words_as_numbers(gb.g2_words(p)))
    st, p = gb.g1_decode(data, raw)
    return "g1dec %x %s = %s %s" % (raw, chunks(data), hx(st), words_as_numbers(gb.g1_words(p)))


def enc_line(g2, raw, p):
    data = gb.g2_encode(p, raw) if g2 else gb.g1_encode(p, raw)
    words = gb.g2_words(p) if g2 else gb.g1_words(p)
    return "%s %x %s = %s %s" % ("g2enc" if g2 else "g1enc", raw, words_as_numbers(words), hx(0), chunks(data))


def twist_point_outside_subgroup(rng):
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = gb.f2_sqrt(gb.f2_add(gb.f2_mul(gb.f2_mul(x, x), x), gb.B2))
        if y is not None and not gb.g2_in_subgroup((x, y)):
            return x, y


@pytest.fixture(scope="module")
def cases():
    rng = random.Random(2540)
    lines = []
    # square roots in Fq: squares (the edges among them) and non-squares
    for v in [0, 1, Q - 1, 2, HALF_LO, HALF_HI] + [rng.randrange(Q) for _ in range(8)]:
        lines.append("sqrt %s = %s %s" % (mont(v * v), hx(1), hx(small(gb.fq_sqrt(v * v)))))
    found = 0
    while found < 8:
        a = rng.randrange(Q)
        if gb.fq_sqrt(a) is None:
            lines.append("sqrt %s = %s %s" % (mont(a), hx(0), hx(0)))
            found += 1
    # ... and in Fq2: squares of random values, values in Fq that are and are not squares there (the root is then real or
    # purely imaginary), purely imaginary values, zero; non-squares
    f2_values = [(rng.randrange(Q), rng.randrange(Q)) for _ in range(8)] + [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1), (3, 0), (Q - 3, 0),
                                                                            (rng.randrange(Q), 0), (0, rng.randrange(Q)), (5, 5)]
    n_square = n_non = 0
    for v in f2_values:
        for a in (gb.f2_mul(v, v), v):
            y = gb.f2_sqrt(a)
            if y is None:
                n_non += 1
                lines.append("sqrt2 %s = %s %s" % (mont(*a), hx(0), mont(0, 0)))
            else:
                n_square += 1
                assert gb.f2_mul(y, y) == (a[0] % Q, a[1] % Q)
                lines.append("sqrt2 %s = %s %s %s" % (mont(*a), hx(1), hx(small2(y)[0]), hx(small2(y)[1])))
    assert n_square >= 18 and n_non >= 4
    # the largest rule
    for y, want in ((HALF_LO, 0), (HALF_HI, 1), (1, 0), (Q - 1, 1), (0, 0), (HALF_LO - 1, 0), (HALF_HI + 1, 1)):
        assert gb.fq_largest(y) == bool(want)
        lines.append("largest %s = %s" % (mont(y), hx(want)))
        lines.append("largest2 %s = %s" % (mont(y, 0), hx(want)))                 # A1 = 0: decided on A0
        lines.append("largest2 %s = %s" % (mont(Q - 1 - y, y), hx(want if y else gb.fq_largest(Q - 1))))   # decided on A1 against A0
    for a0 in (0, 1, HALF_HI, Q - 1):
        lines.append("largest2 %s = %s" % (mont(a0, HALF_LO), hx(0)))
        lines.append("largest2 %s = %s" % (mont(a0, HALF_HI), hx(1)))
    # byte parsing at the edges: x = 0, q - 1, q, q + 1, 2^254 - 1 under the mask, both flags; in raw mode on x and on y
    g1 = [bn.g1_mul(k, bn.G1) for k in (1, 2, R - 1, rng.randrange(R), rng.randrange(R))]
    g2 = [bn.g2_mul(k, bn.G2) for k in (1, 2, R - 1, rng.randrange(R))]
    for x in (0, Q - 1, Q, Q + 1, (1 << 254) - 1):
        for flag in (0x80, 0xC0):
            b = bytearray(x.to_bytes(32, "big"))
            b[0] |= flag
            lines.append(dec_line(False, False, bytes(b)))
            lines.append(dec_line(True, False, bytes(b) + gb._be(g2[0][0][0])))
            lines.append(dec_line(True, False, bytes([flag | gb._be(g2[0][0][1])[0]]) + gb._be(g2[0][0][1])[1:] + x.to_bytes(32, "big")))
        if x < 1 << 254:
            lines.append(dec_line(False, True, x.to_bytes(32, "big") + gb._be(g1[1][1])))
        lines.append(dec_line(False, True, gb._be(g1[1][0]) + x.to_bytes(32, "big")))
    # whole points, infinity, flags for the wrong mode, infinity with a stray bit
    for raw in (False, True):
        for p in g1 + [None]:
            data = gb.g1_encode(p, raw)
            lines += [dec_line(False, raw, data), enc_line(False, raw, p), dec_line(False, not raw, (data + data)[:gb.G1_SIZE[not raw]])]
        for p in g2 + [None]:
            data = gb.g2_encode(p, raw)
            lines += [dec_line(True, raw, data), enc_line(True, raw, p), dec_line(True, not raw, (data + data)[:gb.G2_SIZE[not raw]])]
        for size, is_g2 in ((gb.G1_SIZE[raw], False), (gb.G2_SIZE[raw], True)):
            for at, value in ((0, 0x41), (1, 1), (size - 1, 0x80)):
                b = bytearray(size)
                b[0] = 0x40
                b[at] = value if at else 0x41
                lines.append(dec_line(is_g2, raw, bytes(b)))
        p = g1[3]
        lines.append(dec_line(False, True, gb._be(p[0]) + gb._be((p[1] + 1) % Q)))
    outside = twist_point_outside_subgroup(rng)
    for raw in (False, True):
        for sub in (True, False):
            lines.append(dec_line(True, raw, gb.g2_encode(outside, raw), sub))
    q2 = g2[3]
    lines.append(dec_line(True, True, gb.g2_encode((q2[0], gb.f2_add(q2[1], (1, 0))), True)))
    # encode does not test the curve: the flag choice on synthetic y, the A1 = 0 branch among them
    for y in (HALF_LO, HALF_HI, 1, Q - 1):
        lines.append(enc_line(False, False, (7, y)))
        for yy in ((y, 0), (Q - 1 - y, y), (0, y)):
            lines.append(enc_line(True, False, ((7, 9), yy)))
            lines.append(enc_line(True, True, ((7, 9), yy)))
    # a coordinate that is no residue: refused, zero bytes
    lines.append("g1enc 0 %s %s = %s %s" % (hx(Q), hx(5), hx(gb.RANGE), hx(0)))
    lines.append("g2enc 1 %s %s %s %s = %s %s" % (hx(5), hx(5), hx(5), hx(Q), hx(gb.RANGE), " ".join([hx(0)] * 4)))
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


def test_statuses_present(cases):
    """the cases reach every status"""
    seen = {int(line.split("=")[1].split()[0], 16) for line in cases.splitlines() if line.startswith(("g1dec", "g2dec"))}
    assert seen == {gb.OK, gb.BAD_FLAG, gb.RANGE, gb.BAD_INFINITY, gb.OFF_CURVE, gb.NOT_IN_SUBGROUP}


def test_header_against_the_model(cases, tmp_path):
    _run(_build(tmp_path, "bn254_codec_check", ["-O2"]), cases, tmp_path)


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
    _run(_build(tmp_path, "bn254_codec_check_san", san), cases, tmp_path)
