"""CPU tests of tools/gnark_bytes_model.py, the place of record for gnark's point and container bytes: point round trips in
both modes, its compressed bytes against the package's host g1_compress / g2_compress (written independently, for the proofs),
its classification of malformed points, container round trips at the smallest sizes, and the refusal of a file cut anywhere or
carrying trailing bytes, naming the section."""
import os
import random
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_py as bn  # noqa: E402
import gnark_bytes_model as gb  # noqa: E402

Q, R = gb.Q, gb.R


@pytest.fixture(scope="module")
def points():
    rng = random.Random(91)
    ks = [1, 2, R - 1] + [rng.randrange(1, R) for _ in range(5)]
    return [bn.g1_mul(k, bn.G1) for k in ks] + [None], [bn.g2_mul(k, bn.G2) for k in ks] + [None]


def test_model_constants_agree_with_the_oracle():
    assert (gb.Q, gb.R, gb.B2) == (bn.Q, bn.R, bn.B2) and gb.root_of_unity(5) == bn.root_of_unity(5)
    assert pow(gb.root_of_unity(7), 1 << 7, R) == 1 and pow(gb.root_of_unity(7), 1 << 6, R) != 1


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
def test_point_round_trips(points, raw):
    g1, g2 = points
    for p in g1:
        data = gb.g1_encode(p, raw)
        assert len(data) == gb.G1_SIZE[raw] and gb.g1_decode(data, raw) == (gb.OK, p)
    for p in g2:
        data = gb.g2_encode(p, raw)
        assert len(data) == gb.G2_SIZE[raw] and gb.g2_decode(data, raw) == (gb.OK, p)
    assert gb.g1_encode(None, raw) == b"\x40" + bytes(gb.G1_SIZE[raw] - 1) and gb.g2_encode(None, raw) == b"\x40" + bytes(gb.G2_SIZE[raw] - 1)
    # y and -y differ in the flag alone
    p, n = g1[3], (g1[3][0], Q - g1[3][1])
    a, b = gb.g1_encode(p), gb.g1_encode(n)
    assert a[1:] == b[1:] and {a[0] >> 6, b[0] >> 6} == {2, 3}


def test_compressed_bytes_equal_the_packages_host_encoders(nlx, points):
    g16 = nlx.bn254_groth16
    g1, g2 = points
    for p in g1:
        words = nlx.bn254_g1_pack([p])[0]
        assert list(words) == gb.g1_words(p)
        assert gb.g1_encode(p) == g16.g1_compress(words) == bn.g1_compress(p)
    for p in g2:
        words = nlx.bn254_g2_pack([p])[0]
        assert list(words) == gb.g2_words(p)
        assert gb.g2_encode(p) == g16.g2_compress(words)


def test_square_roots():
    rng = random.Random(17)
    roots = none = 0
    for i in range(48):
        a = (rng.randrange(Q), rng.randrange(Q) if i % 3 else 0)
        y = gb.f2_sqrt(a)
        norm_is_square = gb.fq_sqrt(a[0] * a[0] + a[1] * a[1]) is not None      # a is a square in Fq2 iff its norm is one in Fq
        assert (y is not None) == norm_is_square
        if y is None:
            none += 1
        else:
            roots += 1
            assert gb.f2_mul(y, y) == a
    assert roots >= 12 and none >= 12
    assert gb.f2_sqrt((0, 0)) == (0, 0) and gb.f2_sqrt((Q - 1, 0)) in ((0, 1), (0, Q - 1))


def test_classification_of_malformed_points(points):
    g1, g2 = points
    p, q2 = g1[4], g2[4]
    c, r = gb.g1_encode(p), gb.g1_encode(p, True)
    flag = lambda data, f: bytes([(data[0] & 0x3F) | (f << 6)]) + data[1:]
    assert gb.g1_decode(flag(c, 0))[0] == gb.BAD_FLAG and gb.g1_decode(flag(r, 2), True)[0] == gb.BAD_FLAG and gb.g1_decode(flag(r, 3), True)[0] == gb.BAD_FLAG
    assert gb.g1_decode(b"\x40" + bytes(30) + b"\x01")[0] == gb.BAD_INFINITY and gb.g1_decode(b"\x41" + bytes(63), True)[0] == gb.BAD_INFINITY
    for x in (Q, Q + 1, (1 << 254) - 1):
        assert gb.g1_decode(flag(x.to_bytes(32, "big"), 2))[0] == gb.RANGE
        assert gb.g2_decode(flag(gb._be(q2[0][1]), 3) + x.to_bytes(32, "big"))[0] == gb.RANGE
    assert gb.g1_decode(r[:32] + gb._be((p[1] + 1) % Q), True)[0] == gb.OFF_CURVE
    assert gb.g1_decode(flag(bytes(32), 2))[0] == gb.OFF_CURVE                                   # x = 0: 3 is no square
    rng = random.Random(5)
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = gb.f2_sqrt(gb.f2_add(gb.f2_mul(gb.f2_mul(x, x), x), gb.B2))
        if y is not None:
            break
    outside = gb.g2_encode((x, y))                       # the twist's cofactor is about q: a random twist point is outside
    assert gb.g2_decode(outside)[0] == gb.NOT_IN_SUBGROUP and gb.g2_decode(outside, subgroup=False) in ((gb.OK, (x, y)),)
    assert gb.g2_decode(gb.g2_encode((x, y), True), True)[0] == gb.NOT_IN_SUBGROUP


def _small_key(points, k):
    g1, g2 = points
    key = {"log_n": 1, "n_wires": 3, "g1_alpha": g1[0], "g1_beta": g1[1], "g1_delta": g1[2], "g2_beta": g2[1], "g2_delta": g2[2],
           "g1_a": [g1[3], None], "g1_b": [g1[4]], "g2_b": [g2[4]], "g1_z": [g1[5]], "g1_k": [g1[6]] if k == 0 else [],
           "infinity_a": [False, True, False], "infinity_b": [True, False, True],
           "commitments": [([g1[5]], [g1[6]])][:k]}
    return key


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
def test_container_round_trips(points, raw):
    g1, g2 = points
    for n in (1, 2, 3):
        data = gb.srs_bytes(g1[:n], g2[0], g2[1], raw)
        assert len(data) == 4 + (n + 1) * gb.G1_SIZE[raw] + 2 * gb.G2_SIZE[raw]
        assert gb.srs_parse(data) == (g1[:n], g2[0], g2[1])
    for k in (0, 1):
        key = _small_key(points, k)
        data = gb.key_bytes(key, raw)
        assert gb.key_parse(data) == key
        assert data[:8] == (2).to_bytes(8, "big") and data[8 + 3 * 32:8 + 4 * 32] == (5).to_bytes(32, "big")


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
def test_truncated_and_trailing_data_are_refused_naming_the_section(points, raw):
    g1, g2 = points
    srs = gb.srs_bytes(g1[:2], g2[0], g2[1], raw)
    s1, s2 = gb.G1_SIZE[raw], gb.G2_SIZE[raw]
    cuts = {"Pk.G1 count": 2, "Pk.G1:": 4 + s1 + 1, "Vk.G2[0]": 4 + 2 * s1 + 5, "Vk.G2[1]": 4 + 2 * s1 + s2 + 5, "Vk.G1:": len(srs) - 1}
    for section, cut in cuts.items():
        with pytest.raises(ValueError, match="truncated in " + re.escape(section)):
            gb.srs_parse(srs[:cut])
    with pytest.raises(ValueError, match="truncated in Pk.G1:"):
        gb.srs_parse(srs[:4])
    with pytest.raises(ValueError, match="Pk.G1 is empty"):
        gb.srs_parse(bytes(4) + srs[4:])
    with pytest.raises(ValueError, match="SRS: 1 trailing"):
        gb.srs_parse(srs + b"\x00")
    key = _small_key(points, 1)
    data = gb.key_bytes(key, raw)
    # walk the sections by their sizes: a cut in the middle of each names it
    sections = [("domain", gb.DOMAIN_BYTES), ("G1.Alpha", s1), ("G1.Beta", s1), ("G1.Delta", s1), ("G1.A", 4 + 2 * s1), ("G1.B", 4 + s1),
                ("G1.Z", 4 + s1), ("G1.K", 4), ("G2.Beta", s2), ("G2.Delta", s2), ("G2.B", 4 + s2), ("nbWires", 8), ("NbInfinityA", 8),
                ("NbInfinityB", 8), ("InfinityA", 4 + 3), ("InfinityB", 4 + 3), ("commitment keys count", 4), ("commitment key 0 Basis", 4 + s1),
                ("commitment key 0 BasisExpSigma", 4 + s1)]
    assert sum(size for _, size in sections) == len(data)
    at = 0
    for section, size in sections:
        with pytest.raises(ValueError, match="truncated in %s" % section):
            gb.key_parse(data[:at + size - 1])
        if section == "G1.Alpha":
            with pytest.raises(ValueError, match="truncated in G1.Alpha"):
                gb.key_parse(data[:at])
        at += size
    with pytest.raises(ValueError, match="proving key: 2 trailing"):
        gb.key_parse(data + b"\x00\x00")
    # counts that disagree with the sizes
    bad = dict(key, infinity_a=[False, False, False])
    with pytest.raises(ValueError, match="InfinityA"):
        gb.key_parse(gb.key_bytes(bad, raw))
    with pytest.raises(ValueError, match="G1.Z"):
        gb.key_parse(gb.key_bytes(dict(key, g1_z=[]), raw))
    with pytest.raises(ValueError, match="G2.B"):
        gb.key_parse(gb.key_bytes(dict(key, g2_b=[]), raw))
    with pytest.raises(ValueError, match="domain"):
        gb.key_parse(b"\x00" * 7 + b"\x03" + data[8:])
