"""CPU tests of PoseidonBN128 (the hash of plonky2x's wrapper config): the generator and reference model
(tools/gen_poseidon_bn128.py) against published known answers and hand-derived hash_no_pad expectations, the committed
constants table, and the device header csrc/poseidon_bn128.hpp built with g++ under UBSan against the model."""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_bn128 as m  # noqa: E402

R = m.R
GL_P = m.GL_P


def test_generator_reproduces_committed_table():
    with open(m.INC) as f:
        assert f.read() == m.render()


def test_known_answers():
    """circomlib poseidon([1, 2]) (t = 3, R_P = 57) and poseidon([1, 2, 3]) (t = 4, R_P = 56): recipe and round structure"""
    assert m.permute([0, 1, 2], t=3, rp=57)[0] == 7853200120776062878684798364095072458815029376092732009249414926327459813530
    assert hex(m.permute([0, 1, 2], t=3, rp=57)[0]).startswith("0x115cc0f5") and hex(m.permute([0, 1, 2], t=3, rp=57)[0]).endswith("4417189a")
    assert m.permute([0, 1, 2, 3])[0] == 6542985608222806190361240322586112750744169038454362455181422643027100751666
    rc3, mds3 = m.constants(3, 8, 57)
    assert len(rc3) == 65 * 3 and "%064x" % rc3[0] == "0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e"
    assert ("%064x" % mds3[0][0]).startswith("109b7f41") and ("%064x" % mds3[0][0]).endswith("2ba8118b")
    rc, mds = m.constants()
    assert len(rc) == 64 * 4 and all(0 <= c < R for c in rc)
    assert all(0 < mds[i][j] < R for i in range(4) for j in range(4)) and len({v for row in mds for v in row}) == 16


def _gl(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(GL_P) for _ in range(n)]


def test_hash_no_pad_slot_overwrite():
    """the chunking rule written out by hand: 9 elements per permutation, group j of <= 3 OVERWRITES slot j + 1, slots a short
    last chunk does not reach keep their value, digest = slot 0"""
    P = m.permute
    pk = m.pack3
    x = _gl(135, 7)
    assert m.hash_no_pad([]) == 0                                    # no chunk: no permutation
    assert m.hash_no_pad(x[:1]) == P([0, pk(x[:1]), 0, 0])[0]
    assert m.hash_no_pad(x[:4]) == P([0, pk(x[:3]), pk(x[3:4]), 0])[0]
    assert m.hash_no_pad(x[:5]) == P([0, pk(x[:3]), pk(x[3:5]), 0])[0]
    assert m.hash_no_pad(x[:8]) == P([0, pk(x[:3]), pk(x[3:6]), pk(x[6:8])])[0]
    s9 = P([0, pk(x[:3]), pk(x[3:6]), pk(x[6:9])])
    assert m.hash_no_pad(x[:9]) == s9[0]
    assert m.hash_no_pad(x[:10]) == P([s9[0], pk(x[9:10]), s9[2], s9[3]])[0]          # slots 2, 3 keep the permutation's output
    s18 = P([s9[0], pk(x[9:12]), pk(x[12:15]), pk(x[15:18])])
    assert m.hash_no_pad(x[:17]) == P([s9[0], pk(x[9:12]), pk(x[12:15]), pk(x[15:17])])[0]
    assert m.hash_no_pad(x[:18]) == s18[0]
    assert m.hash_no_pad(x[:19]) == P([s18[0], pk(x[18:19]), s18[2], s18[3]])[0]
    s = [0, 0, 0, 0]                                                 # 135 = 15 full chunks
    for c in range(0, 135, 9):
        s = P([s[0], pk(x[c:c + 3]), pk(x[c + 3:c + 6]), pk(x[c + 6:c + 9])])
    assert m.hash_no_pad(x) == s[0]
    # inputs are taken mod p, packing is little-endian by 64-bit words
    assert m.pack3([1, 2, 3]) == 1 + (2 << 64) + (3 << 128)
    assert m.hash_no_pad([GL_P + 5] * 5) == m.hash_no_pad([5] * 5)


def test_hash_or_noop_and_two_to_one():
    x = _gl(4, 3)
    assert m.hash_or_noop([]) == 0
    assert m.hash_or_noop(x[:3]) == x[0] + (x[1] << 64) + (x[2] << 128)
    assert m.hash_or_noop([1, 2]) == 1 + (2 << 64)
    w = m.to_words(R - 1)
    assert all(v < GL_P for v in w) and m.hash_or_noop(w) == R - 1   # r - 1 is a canonical Goldilocks quadruple and below r
    with pytest.raises(m.RangeError):
        m.hash_or_noop([0, 0, 0, (R >> 192) + 1])                     # a value >= r has no digest
    with pytest.raises(m.RangeError):
        m.hash_or_noop(m.to_words(R))
    y = _gl(5, 4)
    assert m.hash_or_noop(y) == m.hash_no_pad(y)
    assert m.two_to_one(3, 4) == m.permute([0, 0, 3, 4])[0]


def test_merkle_model_paths():
    leaves = [_gl(6, 100 + i) for i in range(8)]
    levels = m.merkle_digests(leaves, 1)
    assert [len(lv) for lv in levels] == [8, 4, 2]
    for idx in range(8):
        path, i = [], idx
        for lv in levels[:-1]:
            path.append(lv[i ^ 1])
            i >>= 1
        cap_i, h = m.merkle_root_from_path(m.hash_or_noop(leaves[idx]), idx, path)
        assert h == levels[-1][cap_i]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pbn") / "poseidon_bn128_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "poseidon_bn128_check.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.split("\n")[:len(lines)]
    return run


EDGES = [0, 1, R - 1, (1 << 192) - 1]


def test_header_permutation_equals_model(native):
    rng = random.Random(2024)
    states = [[rng.choice(EDGES) for _ in range(4)] for _ in range(24)] + [[e] * 4 for e in EDGES]
    states += [[rng.randrange(R) for _ in range(4)] for _ in range(200)]
    states += [[(1 << 256) - 1, R, R + 5, 1 << 255]]   # non-canonical integers < 2^256: the header takes them mod r
    out = native(["perm " + " ".join("%x" % v for v in st) for st in states])
    for st, line in zip(states, out):
        assert [int(w, 16) for w in line.split()] == m.permute(st), st


def test_header_dot_product_bounds(native):
    """dot4 on raw values up to 2^258 - 1 (the bound the header states): congruent to sum_j M_ij s_j, result < 2^255"""
    rng = random.Random(5)
    top = (1 << 258) - 1
    cases = [(i, [top] * 4) for i in range(4)] + [(i, [0, top, 0, top]) for i in range(4)]
    cases += [(rng.randrange(4), [rng.choice([top, rng.randrange(1 << 258), rng.randrange(R)]) for _ in range(4)]) for _ in range(300)]
    _, mds = m.constants()
    out = native(["dot4 %d " % i + " ".join("%x" % v for v in s) for i, s in cases])
    for (i, s), line in zip(cases, out):
        val, ok = line.split()
        assert ok == "1", (i, s)                                     # below 2^255, limbs 0..7 normalised
        assert int(val, 16) % R == sum(mds[i][j] * s[j] for j in range(4)) % R
    # the S-box at its input bound (< 2^257.5) and the conversions
    rinv = pow(1 << 261, -1, R)
    xs = [int(2 ** 257.5) - 1, top >> 1, R - 1, 0, 1] + [rng.randrange(1 << 257) for _ in range(50)]
    out = native(["sbox %x" % x for x in xs])
    for x, line in zip(xs, out):
        val, ok = line.split()
        assert ok == "1" and int(val, 16) % R == pow(x, 5, R) * pow(rinv, 4, R) % R
    ys = [0, 1, R - 1, R, (1 << 256) - 1, (1 << 192) - 1] + [rng.randrange(1 << 256) for _ in range(50)]
    out = native(["conv %x" % y for y in ys])
    for y, line in zip(ys, out):
        val, ok = line.split()
        assert ok == "1" and int(val, 16) == y % R
