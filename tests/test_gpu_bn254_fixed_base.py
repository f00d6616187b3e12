"""GPU: the fixed-base batch scalar multiplications nlx_bn254_g1_scalar_muls / nlx_bn254_g2_scalar_muls against the big-integer
model (tools/groth16_model.py g1_gen_mul / g2_gen_mul for the generators, oracle bn.g1_mul and gm.g2_mul for another base), point
by point and exactly: scalars aimed at the 8-bit windows' boundaries, the batch sizes at which the lane assignment changes, both
scalar forms, host and device pointers, the refusals, and 2^16 scalars checked in the exponent through the library's MSM."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu
bn, R, Q = gm.bn, gm.R, gm.Q
E_INVAL, E_RANGE = -1, -4
WINDOW = 8          # csrc/bn254_fixed_base.hpp WINDOW_BITS: the boundaries the scalars below aim at


def _aimed_scalars():
    s = [0, 1, 2, R - 1, R - 2]
    for k in list(range(WINDOW, 254, WINDOW)) + [253]:
        s += [1 << k, (1 << k) - 1]
    top = R >> (WINDOW * 31)                                          # the top window's largest digit that can occur
    for j in range(32):                                                # every digit zero but one: the smallest and the largest
        s += [1 << (WINDOW * j), (255 if j < 31 else top) << (WINDOW * j)]
    s.append(((top - 1) << (WINDOW * 31)) | ((1 << (WINDOW * 31)) - 1))   # every digit maximal, below r
    s.append(int("01" * 32, 16) % R)                                   # every digit 1
    assert all(0 <= x < R for x in s)
    return s


@pytest.fixture(scope="module")
def scalars():
    rng = random.Random(8254)
    s = _aimed_scalars()
    return s + [rng.randrange(R) for _ in range(1000 - len(s))]


@pytest.fixture(scope="module")
def want_g1(scalars):
    return [gm.g1_gen_mul(k) for k in scalars]


@pytest.fixture(scope="module")
def want_g2(scalars):
    return [gm.g2_gen_mul(k) for k in scalars[:321]]


def _canonical(nlx, values):
    return nlx.bn254_pack([values])[0]


def _g1(nlx, words):
    return [nlx.bn254_g1_unpack(w) for w in np.asarray(words)]


def _g2(nlx, words):
    return [nlx.bn254_g2_unpack(w) for w in np.asarray(words)]


def test_aimed_scalars_cover_the_windows(scalars):
    aimed = _aimed_scalars()
    assert len(aimed) < 257 and scalars[:len(aimed)] == aimed
    digits = lambda x: [(x >> (WINDOW * j)) & 255 for j in range(32)]
    for j in range(32):
        assert any(digits(x)[j] != 0 and sum(1 for d in digits(x) if d) == 1 for x in aimed)
    assert max(digits(aimed[-2])[:31]) == 255 == min(digits(aimed[-2])[:31])


# 1000 = 15 x 64 + 40 and 257 = 4 x 64 + 1: lanes take scalars t, t + L, ..; neither size gives every lane the same count
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_g1_generator_multiples(nlx, ctx, g16, scalars, want_g1, n):
    off = 3 if n == 1 else 0                                            # n = 1: r - 1
    got = nlx.bn254_g1_scalar_muls(ctx, bn.G1, _canonical(nlx, scalars[off:off + n]))
    assert got.shape == (n, 8) and _g1(nlx, got) == want_g1[off:off + n]
    mont = nlx.bn254_g1_scalar_muls(ctx, bn.G1, g16.fr_pack(scalars[off:off + n]), montgomery=True)
    assert np.array_equal(mont, got)
    if n > 1:
        assert not got[0].any() and got[1].any()                       # 0 * G = the point at infinity as all-zero words


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 321])
def test_g2_generator_multiples(nlx, ctx, g16, scalars, want_g2, n):
    off = 3 if n == 1 else 0
    got = nlx.bn254_g2_scalar_muls(ctx, bn.G2, _canonical(nlx, scalars[off:off + n]))
    assert got.shape == (n, 16) and _g2(nlx, got) == want_g2[off:off + n]
    mont = nlx.bn254_g2_scalar_muls(ctx, bn.G2, g16.fr_pack(scalars[off:off + n]), montgomery=True)
    assert np.array_equal(mont, got)
    if n > 1:
        assert not got[0].any() and got[1].any()


@pytest.fixture(scope="module")
def g16(nlx):
    return nlx.bn254_groth16


def test_other_bases(nlx, ctx, scalars):
    rng = random.Random(77)
    ks = scalars[:5] + [scalars[61], scalars[-1]] + [rng.randrange(R) for _ in range(5)]
    p1 = bn.g1_mul(rng.randrange(1, R), bn.G1)
    got = nlx.bn254_g1_scalar_muls(ctx, p1, _canonical(nlx, ks))
    assert _g1(nlx, got) == [bn.g1_mul(k, p1) if k else None for k in ks]
    p2 = gm.g2_mul(rng.randrange(1, R), bn.G2)
    got = nlx.bn254_g2_scalar_muls(ctx, p2, _canonical(nlx, ks))
    assert _g2(nlx, got) == [gm.g2_mul(k, p2) for k in ks]
    # the base as words
    assert np.array_equal(nlx.bn254_g1_scalar_muls(ctx, nlx.bn254_g1_pack([p1])[0], _canonical(nlx, ks[:3])), nlx.bn254_g1_scalar_muls(ctx, p1, _canonical(nlx, ks[:3])))


def test_device_pointers(nlx, ctx, g16, scalars, want_g1, want_g2):
    import torch
    dev = "cuda:%d" % ctx.device
    n = 257
    d_s = torch.from_numpy(g16.fr_pack(scalars[:n]).view(np.int64)).to(dev)
    out = nlx.bn254_g1_scalar_muls(ctx, bn.G1, d_s, montgomery=True, device=dev)
    assert out.device.type == "cuda" and _g1(nlx, out.cpu().numpy().view(np.uint64)) == want_g1[:n]
    out = nlx.bn254_g2_scalar_muls(ctx, bn.G2, d_s, montgomery=True, device=dev)
    assert _g2(nlx, out.cpu().numpy().view(np.uint64)) == want_g2[:n]
    # device scalars, host result; host scalars, device result
    assert _g1(nlx, nlx.bn254_g1_scalar_muls(ctx, bn.G1, d_s[:65].contiguous(), montgomery=True)) == want_g1[:65]
    out = nlx.bn254_g2_scalar_muls(ctx, bn.G2, _canonical(nlx, scalars[:65]), device=dev)
    assert _g2(nlx, out.cpu().numpy().view(np.uint64)) == want_g2[:65]
    assert nlx.bn254_g1_scalar_muls(ctx, bn.G1, np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)


def _raises(nlx, code, *needles):
    class Check:
        def __enter__(self):
            self.cm = pytest.raises(nlx.NlxError)
            self.e = self.cm.__enter__()
            return self

        def __exit__(self, *exc):
            done = self.cm.__exit__(*exc)
            assert self.e.value.code == code, str(self.e.value)
            for needle in needles:
                assert needle in str(self.e.value), str(self.e.value)
            return done
    return Check()


def test_refusals(nlx, ctx, g16, scalars):
    before = ctx.memory()[1]
    good = _canonical(nlx, scalars[:70])
    for entry, base in ((nlx.bn254_g1_scalar_muls, bn.G1), (nlx.bn254_g2_scalar_muls, bn.G2)):
        for value, montgomery in ((R, False), (R, True), ((1 << 256) - 1, False)):
            bad = good.copy()
            bad[67] = [(value >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]
            bad[69] = bad[67]
            with _raises(nlx, E_RANGE, "scalar 67 ", "below r"):
                entry(ctx, base, bad, montgomery=montgomery)
    # the base: a coordinate not below q, off the curve, (G2) on the curve outside the subgroup, the point at infinity
    with _raises(nlx, E_RANGE, "below q"):
        nlx.bn254_g1_scalar_muls(ctx, np.array([0xFFFFFFFFFFFFFFFF] * 8, dtype=np.uint64), good)
    with _raises(nlx, E_RANGE, "curve"):
        nlx.bn254_g1_scalar_muls(ctx, (1, 3), good)
    with _raises(nlx, E_RANGE, "curve"):
        nlx.bn254_g2_scalar_muls(ctx, ((1, 0), (2, 0)), good)
    x = 0
    while True:                                                        # a twist point: almost surely outside the subgroup (the cofactor is ~2^254)
        x += 1
        y = gm.f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul((x, 1), (x, 1)), (x, 1)), bn.B2))
        if y is not None and gm.g2_mul(R - 1, ((x, 1), y)) != ((x, 1), ((-y[0]) % Q, (-y[1]) % Q)):
            break
    with _raises(nlx, E_RANGE, "subgroup"):
        nlx.bn254_g2_scalar_muls(ctx, ((x, 1), y), good)
    with _raises(nlx, E_INVAL, "infinity"):
        nlx.bn254_g1_scalar_muls(ctx, np.zeros(8, dtype=np.uint64), good)
    with _raises(nlx, E_INVAL, "infinity"):
        nlx.bn254_g2_scalar_muls(ctx, np.zeros(16, dtype=np.uint64), good)
    assert ctx.memory()[1] == before


def test_2_16_scalars_in_the_exponent(nlx, ctx, g16):
    """sum_i rho_i out_i = (sum_i rho_i k_i) * base through the library's MSM, over both groups; a wrong point anywhere changes
    the left side but for a 2^-128 chance over rho"""
    import torch
    rng = np.random.default_rng(16)
    n = 1 << 16
    dev = "cuda:%d" % ctx.device
    limbs = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    ks = [sum(int(v) << (64 * j) for j, v in enumerate(row)) % R for row in limbs]
    ks[0], ks[n - 1], ks[777] = 0, R - 1, 0
    rhos = [int(a) | (int(b) << 64) for a, b in rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64)]
    d_k = torch.from_numpy(_canonical(nlx, ks).view(np.int64)).to(dev)
    rho_words = _canonical(nlx, rhos)
    total = sum(r_ * k for r_, k in zip(rhos, ks)) % R
    out1 = nlx.bn254_g1_scalar_muls(ctx, bn.G1, d_k, device=dev)
    assert not out1[0].any() and not out1[777].any() and bool(out1[1].any())
    assert nlx.bn254_g1_unpack(nlx.bn254_msm_g1(ctx, out1, rho_words)) == gm.g1_gen_mul(total)
    out2 = nlx.bn254_g2_scalar_muls(ctx, bn.G2, d_k, device=dev)
    assert not out2[0].any() and not out2[777].any()
    assert nlx.bn254_g2_unpack(nlx.bn254_msm_g2(ctx, out2, rho_words)) == gm.g2_gen_mul(total)
    assert nlx.bn254_g1_unpack(out1[n - 1].cpu().numpy().view(np.uint64)) == bn.g1_neg(bn.G1)
