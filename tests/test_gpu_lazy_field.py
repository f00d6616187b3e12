"""GPU test of nlx_ext_ops: the device extension product (one reduction per component), the product by a base element and
reduce160 on UNREDUCED operands, canonical and loose forms, against Python integers.  The code under test is per lane with no dependence on a domain
size, so one batch of the 4 096 aimed combinations and 2^14 random loose operands is the whole of it."""
import numpy as np
import pytest

import lazy_field_model as m

pytestmark = pytest.mark.gpu

P = m.P


def _check(nlx, ctx, cases):
    a = np.array([(c[0], c[1]) for c in cases], dtype=np.uint64)
    b = np.array([(c[2], c[3]) for c in cases], dtype=np.uint64)
    out = nlx.ext_ops(ctx, a, b)
    assert out.shape == (8, len(cases))
    got = out.tolist()
    for i, (a0, a1, b0, b1) in enumerate(cases):
        c0, c1 = m.ext_mul_exact((a0, a1), (b0, b1))
        assert (got[0][i], got[1][i]) == (c0, c1), ("extension product", i, cases[i])
        assert (got[2][i], got[3][i]) == (a0 * b0 % P, a1 * b0 % P), ("product by a base element", i, cases[i])
        assert got[4][i] == m.reduce160_exact(m.limbs_of(a0, a1, b1)), ("reduce160", i, cases[i])
        assert (got[5][i], got[6][i]) == (c0, c1), ("loose extension product", i, cases[i])
        assert got[7][i] == got[4][i], ("reduce160_loose", i, cases[i])


def test_aimed_combinations(nlx, ctx):
    cases = m.aimed_operands()
    top = (1 << 64) - 1
    for lane in (0, 31, 32, 63, len(cases) - 1):   # an extreme case in the wave's end lanes and in the batch's last element
        assert all(v in (top, P, P - 1) for v in cases[lane])
    _check(nlx, ctx, cases)


def test_random_loose_operands(nlx, ctx):
    rng = np.random.default_rng(160)
    v = rng.integers(0, 1 << 64, size=(1 << 14, 4), dtype=np.uint64, endpoint=False)
    v[: 1 << 10] |= np.uint64(0xFFFFFFFF00000000)  # a share of them at and above p
    _check(nlx, ctx, [tuple(int(x) for x in row) for row in v])
