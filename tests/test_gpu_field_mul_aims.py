"""GPU: the device field multiply (gl::mul_chain + gl::reduce128_core, csrc/gl.hpp) on the aimed operand set of
tests/field_mul_model.py - every class (carry k of the product chain, borrow, the rare w2 = 0 case, final carry) in lanes 0, 31,
32 and 63 of a wave and as the last element of a batch - against Python integers: gl::mul and gl::mul_loose through
nlx_field_ops, gl::mul_wide (k folded or handed to the reduction) through nlx_ext_ops, gl32::mul through the permutation's
first-round S-boxes.  Per-lane functions with no dependence on a domain size: one batch each is the whole of it."""
import numpy as np
import pytest

import field_mul_model as fm
import poseidon_aims as pa

pytestmark = pytest.mark.gpu

P = fm.P
LANES = (0, 31, 32, 63)


def _laid_out(n_random, seed):
    """the aimed pairs as one batch: wave c holds class c's hit in lanes 0, 31, 32, 63; the other lanes and the waves after take
    the aimed pairs in order, then n_random random loose pairs; the last element is a hit again (the rare case)"""
    rng = np.random.default_rng(seed)
    aimed = fm.aimed_pairs()
    n = 64 * len(fm.KNOWN_HITS) + len(aimed) + n_random + 1
    a = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    free = [i for i in range(n - 1) if not (i < 64 * len(fm.KNOWN_HITS) and i % 64 in LANES)]
    for i, (x, y) in zip(free, aimed):
        a[i], b[i] = x, y
    for c, (x, y) in enumerate(fm.KNOWN_HITS):
        for lane in LANES:
            a[64 * c + lane], b[64 * c + lane] = x, y
    a[n - 1], b[n - 1] = fm.KNOWN_HITS[0]
    return a, b


def _check_field_ops(nlx, ctx, a, b):
    out = nlx.field_ops(ctx, a, b)
    mul, loose = out[0].tolist(), out[4].tolist()
    for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        assert mul[i] == (x % P) * (y % P) % P, ("gl::mul", i, hex(x), hex(y), fm.classify(x % P, y % P))
        assert loose[i] == x * y % P, ("canon(gl::mul_loose)", i, hex(x), hex(y), fm.classify(x, y))


def test_field_ops_aimed(nlx, ctx):
    a, b = _laid_out(1 << 14, 14)
    seen = {fm.classify(x, y) for x, y in zip(a[:64 * 9].tolist(), b[:64 * 9].tolist())}
    assert set(fm.KNOWN_CLASSES) <= seen
    _check_field_ops(nlx, ctx, a, b)
    # every class as the last element of a short batch, in a lane of its own
    for c, (x, y) in enumerate(fm.KNOWN_HITS):
        k = 1 + 7 * c
        aa = np.array([fm.KNOWN_HITS[(c + j) % 9][0] for j in range(k - 1, -1, -1)], dtype=np.uint64)
        bb = np.array([fm.KNOWN_HITS[(c + j) % 9][1] for j in range(k - 1, -1, -1)], dtype=np.uint64)
        assert (int(aa[-1]), int(bb[-1])) == (x, y)
        _check_field_ops(nlx, ctx, aa, bb)


def test_ext_ops_on_aimed_pairs(nlx, ctx):
    """gl::mul(Ext, Ext): the four products of (a, b) x (c, d) are a d, b c (component 1) and a c, b d (component 0); with
    x = (a, b) and y = (b', a') built from hits (a, a'), (b, b') both products of component 1 are hits, and with y = (a', b')
    both of component 0 - each class so reaches the product whose k the reduction takes and the one whose k is folded"""
    a, b = _laid_out(1 << 12, 12)
    n = len(a) - 1                              # pairs (i, i + 1) of the batch, every element first and second once
    x = np.stack([a[:n], a[1:]], axis=1)
    for y in (np.stack([b[1:], b[:n]], axis=1), np.stack([b[:n], b[1:]], axis=1)):
        out = nlx.ext_ops(ctx, x, y).tolist()
        for i, ((x0, x1), (y0, y1)) in enumerate(zip(x.tolist(), y.tolist())):
            want = fm.ext_mul_exact((x0, x1), (y0, y1))
            assert (out[0][i], out[1][i]) == want, ("extension product", i, hex(x0), hex(x1), hex(y0), hex(y1))
            assert (out[5][i], out[6][i]) == want, ("loose extension product", i, hex(x0), hex(x1), hex(y0), hex(y1))
            assert (out[2][i], out[3][i]) == (x0 * y0 % P, x1 * y0 % P), ("product by a base element", i)


def test_permute_first_round_sboxes_on_aimed_operands(nlx, ctx, orc):
    """2^10 states whose first-round S-box inputs (state + round constants) are aimed operands: the first multiply of each of
    the twelve S-boxes is the square of one, the later ones take what it gives; against the host permutation"""
    vals = sorted({v % P for pair in fm.aimed_pairs() for v in pair})
    rc = pa.RC[:12]
    n = 1 << 10
    st = np.zeros((n, 12), dtype=np.uint64)
    for i in range(n):
        for j in range(12):
            st[i, j] = (vals[(i + 5 * j + (i // 64)) % len(vals)] - rc[j]) % P
    # lanes 0, 31, 32, 63 of wave c and the last state: one aimed operand in all twelve places
    for c in range(n // 64):
        for lane in LANES:
            st[64 * c + lane] = [(vals[(4 * c + LANES.index(lane)) % len(vals)] - rc[j]) % P for j in range(12)]
    st[n - 1] = [((1 << 63) - rc[j]) % P for j in range(12)]
    got = nlx.poseidon_permute(ctx, st)
    assert np.array_equal(got, orc.poseidon_permute(st))
    assert got[n - 1].tolist() == pa.gpb.naive(st[n - 1].tolist())
