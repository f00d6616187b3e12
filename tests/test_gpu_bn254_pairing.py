"""GPU: the optimal ate pairing on the device (nlx_bn254_pairing, nlx_bn254_pairing_check) against the big-integer model
tools/bn254_pairing_model.py.  Values: e(a G1, b G2) = E^(a b) with E the model's single e(G1, G2) - one model pairing and one
GT power per pair - on a partial wave, a full one, one lane over and more than one block, and two pairs of points that are no
known multiples of the generators against the model's full pairing.  Checks, and the refusals of the entry.  Exact."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_pairing_model as pm  # noqa: E402
import groth16_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu
bn, R, Q = pm.bn, pm.R, pm.Q
E_RANGE = -4
N_POOL = 130


@pytest.fixture(scope="module")
def pool():
    """130 pairs (a, b, a G1 or None, b G2 or None) and E^(a b): the first ones full-size and extreme, the rest with small
    scalars so that the model's GT power stays short"""
    rng = random.Random(2540)
    e11 = pm.pairing(bn.G1, bn.G2)
    scalars = [(1, 1), (R - 1, 1), (R - 1, R - 1), (rng.randrange(R), rng.randrange(R))]
    inv = rng.randrange(2, R)
    scalars.append((inv, pow(inv, R - 2, R)))                       # a b = 1 mod r
    scalars += [(rng.randrange(R), rng.randrange(R)) for _ in range(3)]
    scalars += [(rng.randrange(1, 1 << 12), rng.randrange(1, 1 << 12)) for _ in range(N_POOL - len(scalars))]
    out = []
    for i, (a, b) in enumerate(scalars):
        p, q2 = gm.g1_gen_mul(a), gm.g2_gen_mul(b)
        if i in (9, 70):
            p = None                                                # a point at infinity on either side: the pairing is 1
        if i in (10, 129):
            q2 = None
        want = pm.F12_ONE if p is None or q2 is None else pm.f12_pow(e11, a * b % R)
        out.append((p, q2, want))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_values(nlx, ctx, pool, n):
    start = 0 if n != 1 else 3                                      # the single pair: a random full-size one
    rows = pool[start:start + n]
    g1, g2 = nlx.bn254_g1_pack([r[0] for r in rows]), nlx.bn254_g2_pack([r[1] for r in rows])
    got = nlx.bn254_gt_unpack(nlx.bn254_pairing(ctx, g1, g2))
    for i, (g, row) in enumerate(zip(got, rows)):
        assert g == row[2], (n, i)


def test_canonical_words_and_device_tensors(nlx, ctx, pool):
    import torch
    rows = pool[:5]
    g1, g2 = nlx.bn254_g1_pack([r[0] for r in rows]), nlx.bn254_g2_pack([r[1] for r in rows])
    t1 = torch.from_numpy(g1.view(np.int64)).to("cuda:0")
    t2 = torch.from_numpy(g2.view(np.int64)).to("cuda:0")
    got = nlx.bn254_gt_unpack(nlx.bn254_pairing(ctx, t1, t2, montgomery=False), montgomery=False)
    assert got == [r[2] for r in rows]


def _random_g1(rng):
    while True:
        x = rng.randrange(Q)
        y = gm.fq_sqrt(x * x * x + 3)
        if y is not None:
            return x, y


def test_points_that_are_no_known_multiples(nlx, ctx):
    """G1 has cofactor 1: any curve point; G2: a twist point cleared of the cofactor 2 q - r"""
    rng = random.Random(77)
    pairs = []
    for _ in range(2):
        q2 = pm._g2_mul_any(2 * Q - R, pm.twist_point_outside_subgroup(rng))
        assert q2 is not None and pm.g2_in_subgroup(q2)
        pairs.append((_random_g1(rng), q2))
    got = nlx.bn254_gt_unpack(nlx.bn254_pairing(ctx, nlx.bn254_g1_pack([p for p, _ in pairs]), nlx.bn254_g2_pack([q for _, q in pairs])))
    assert got == [pm.pairing(p, q2) for p, q2 in pairs]


def _check_pairs(rng, m, good):
    """m pairs whose pairings multiply to 1 (good) or miss it by one factor e(G1, G2)"""
    if m == 1:
        return [(None, gm.g2_gen_mul(rng.randrange(1, R)))] if good else [(bn.G1, bn.G2)]
    ab = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(m - 1)]
    total = sum(a * b for a, b in ab) % R
    last = (-total + (0 if good else 1)) % R
    return [(gm.g1_gen_mul(a), gm.g2_gen_mul(b)) for a, b in ab] + [(gm.g1_gen_mul(last), bn.G2)]


@pytest.mark.parametrize("n_checks", [1, 64, 65])
def test_checks(nlx, ctx, n_checks):
    rng = random.Random(100 + n_checks)
    pairs, counts, want = [], [], []
    for c in range(n_checks):
        if n_checks == 65 and c == 40:
            pairs += [(None, None), (None, bn.G2), (bn.G1, None)]   # a check whose pairs are all at infinity
            counts.append(3)
            want.append(True)
            continue
        if n_checks == 65 and c == 41:
            counts.append(0)                                        # and one of no pairs
            want.append(True)
            continue
        m = 2 if n_checks == 1 else 1 + (c % 5)
        good = n_checks == 1 or rng.random() < 0.5
        pairs += _check_pairs(rng, m, good)
        counts.append(m)
        want.append(good)
    assert len(counts) == n_checks and (n_checks == 1 or (True in want and False in want))
    got = nlx.bn254_pairing_check(ctx, nlx.bn254_g1_pack([p for p, _ in pairs]), nlx.bn254_g2_pack([q for _, q in pairs]), counts)
    assert got == want


def test_inverse_pair_and_off_by_one(nlx, ctx):
    rng = random.Random(9)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    p, q2 = gm.g1_gen_mul(a), gm.g2_gen_mul(b)
    g2 = nlx.bn254_g2_pack([q2, bn.G2])
    assert nlx.bn254_pairing_check(ctx, nlx.bn254_g1_pack([p, gm.g1_gen_mul(-a * b % R)]), g2, [2]) == [True]
    assert nlx.bn254_pairing_check(ctx, nlx.bn254_g1_pack([p, gm.g1_gen_mul((1 - a * b) % R)]), g2, [2]) == [False]


def test_refusals_leave_the_context_usable(nlx, ctx, pool):
    rng = random.Random(31)
    p, q2 = gm.g1_gen_mul(5), gm.g2_gen_mul(7)
    good1, good2 = nlx.bn254_g1_pack([p, p]), nlx.bn254_g2_pack([q2, q2])
    # a coordinate = q: the words of the integer q (no residue), on either side
    qw = np.array([(Q >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)], dtype=np.uint64)
    bad = good1.copy()
    bad[1, 0:4] = qw
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_pairing(ctx, bad, good2)
    assert e.value.code == E_RANGE and "pair 1" in str(e.value) and "below q" in str(e.value)
    bad2 = good2.copy()
    bad2[0, 12:16] = qw
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_pairing_check(ctx, good1, bad2, [2])
    assert e.value.code == E_RANGE and "pair 0" in str(e.value)
    # a G1 point off the curve
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_pairing(ctx, nlx.bn254_g1_pack([p, (p[0], (p[1] + 1) % Q)]), good2)
    assert e.value.code == E_RANGE and "pair 1" in str(e.value) and "not on the curve" in str(e.value)
    # a twist point outside the subgroup: x drawn until x^3 + b' is a square
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = gm.f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.B2))
        if y is not None:
            break
    assert pm._g2_mul_any(R, (x, y)) is not None                    # [r] Q != O
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_pairing(ctx, good1, nlx.bn254_g2_pack([q2, (x, y)]))
    assert e.value.code == E_RANGE and "pair 1" in str(e.value) and "subgroup" in str(e.value)
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_pairing_check(ctx, good1, nlx.bn254_g2_pack([(x, y), q2]), [1, 1])
    assert e.value.code == E_RANGE
    with pytest.raises(nlx.NlxError) as e:
        ctx.check(nlx.lib.dll.nlx_bn254_pairing(ctx.handle, good1.ctypes.data, good2.ctypes.data, 2, 8, None))
    assert e.value.code == -1
    # and the context still answers
    row = pool[3]
    assert nlx.bn254_gt_unpack(nlx.bn254_pairing(ctx, nlx.bn254_g1_pack([row[0]]), nlx.bn254_g2_pack([row[1]])))[0] == row[2]
