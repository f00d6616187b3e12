"""GPU: segmented G1 linear combinations (nlx_bn254_g1_lincomb, csrc/bn254_g1_lincomb.hip) against the big-integer group law of
oracle/bn254_py.py.  Exact.  Every point is a known multiple of G, so a segment's expected sum is one scalar multiplication of
the model; the kernel knows nothing of the logarithms."""
import random

import numpy as np
import pytest

from bn254_plonk_verify_cases import bn

pytestmark = pytest.mark.gpu
R = bn.R
E_RANGE = -4
LENGTHS = (0, 1, 2, 63, 64, 65, 130)        # one wave per segment: none, one lane, two, a wave less one, a wave, a second pass, a third


def _scalar_words(nlx, scalars):
    return nlx.bn254_pack([[int(s) for s in scalars]])[0]


@pytest.fixture(scope="module")
def problem():
    """(logs or None per term, scalars, first, expected points): the lengths above with random scalars, then the special segments"""
    rng = random.Random(3232)
    logs, scalars, first = [], [], [0]

    def segment(terms):
        for a, s in terms:
            logs.append(a)
            scalars.append(s)
        first.append(len(logs))

    for n in LENGTHS:
        segment([(rng.randrange(1, R), rng.randrange(R)) for _ in range(n)])
    a, s = rng.randrange(1, R), rng.randrange(1, R)
    segment([(rng.randrange(1, R), x) for x in (0, 1, R - 1, 0, rng.randrange(R))])          # the scalars 0, 1, r - 1
    segment([(a, s), (a, s)])                                                               # P + P in the tree's first round
    segment([(a, s)] * 64)                                                                  # P + P in every round
    segment([(a, s), (R - a, s)])                                                           # P + (-P)
    segment([(a, s), (R - a, s)] * 32 + [(a, 1)])                                           # cancellations in the tree, then one more pass
    segment([(None, rng.randrange(R)) for _ in range(5)])                                   # all infinities
    segment([(None, 5), (a, s), (None, 1), (a, 1), (None, 0)])                              # infinity among points
    segment([(a, 0)] * 3)                                                                   # all scalars 0
    segment([(a, R - 1), (a, 1)])                                                           # -P + P through the ladder's last steps
    expected = []
    for lo, hi in zip(first, first[1:]):
        total = sum(logs[t] * scalars[t] for t in range(lo, hi) if logs[t] is not None) % R
        expected.append(bn.g1_mul(total, bn.G1) if total else None)
    points = [None if a is None else bn.g1_mul(a, bn.G1) for a in logs]
    return points, scalars, first, expected


def test_segments_against_the_model(nlx, ctx, problem):
    points, scalars, first, expected = problem
    assert [b - a for a, b in zip(first, first[1:])][:len(LENGTHS)] == list(LENGTHS)
    got = nlx.bn254_g1_lincomb(ctx, nlx.bn254_g1_pack(points), _scalar_words(nlx, scalars), first)
    assert got.shape == (len(first) - 1, 8)
    assert [nlx.bn254_g1_unpack(w) for w in got] == expected
    assert not got[0].any() and expected[0] is None                      # the empty segment: all-zero words
    # a cross-check of the logarithm bookkeeping itself on one segment: the model's own multi-scalar sum
    lo, hi = first[2], first[3]
    assert bn.msm_g1(scalars[lo:hi], points[lo:hi]) == expected[2]


def test_inputs_on_the_device(nlx, ctx, problem):
    import torch
    points, scalars, first, expected = problem
    p = torch.from_numpy(nlx.bn254_g1_pack(points).view(np.int64)).cuda()
    s = torch.from_numpy(_scalar_words(nlx, scalars).view(np.int64)).cuda()
    got = nlx.bn254_g1_lincomb(ctx, p, s, first)
    assert [nlx.bn254_g1_unpack(w) for w in got] == expected


def test_one_segment_and_none(nlx, ctx, problem):
    points, scalars, first, expected = problem
    lo, hi = first[4], first[5]                                          # the segment of 64 alone
    got = nlx.bn254_g1_lincomb(ctx, nlx.bn254_g1_pack(points[lo:hi]), _scalar_words(nlx, scalars[lo:hi]), [0, hi - lo])
    assert nlx.bn254_g1_unpack(got[0]) == expected[4]
    assert nlx.bn254_g1_lincomb(ctx, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), [0]).shape == (0, 8)
    got = nlx.bn254_g1_lincomb(ctx, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), [0, 0, 0])
    assert got.shape == (2, 8) and not got.any()


def test_refusals(nlx, ctx, problem):
    points, scalars, first, _ = problem
    lo, hi = first[5], first[6]                                          # 65 terms
    pw, sw = nlx.bn254_g1_pack(points[lo:hi]), _scalar_words(nlx, scalars[lo:hi])
    off = pw.copy()
    off[64, 4] ^= np.uint64(1)
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_g1_lincomb(ctx, off, sw, [0, 3, 65])
    assert e.value.code == E_RANGE and "term 64:" in str(e.value) and "curve" in str(e.value)
    big = pw.copy()
    big[7, :4] = nlx.bn254_pack([[bn.Q]])[0][0]
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_g1_lincomb(ctx, big, sw, [0, 65])
    assert e.value.code == E_RANGE and "term 7:" in str(e.value) and "below q" in str(e.value)
    bad = sw.copy()
    bad[33] = nlx.bn254_pack([[R]])[0][0]
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_g1_lincomb(ctx, pw, bad, [0, 65])
    assert e.value.code == E_RANGE and "term 33:" in str(e.value) and "below r" in str(e.value)
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_g1_lincomb(ctx, pw, sw, [0, 40, 30, 65])
    assert e.value.code == E_RANGE
    with pytest.raises(ValueError):
        nlx.bn254_g1_lincomb(ctx, pw, sw, [0, 64])
