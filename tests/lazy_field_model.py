"""Python-integer model of the lazily reduced device forms of csrc/gl.hpp - the extension product with one reduction per
component and reduce160 - limb by limb, with the device code's limb widths and order of additions.  Every intermediate is
checked against the width of the register (pair) that holds it on the device.  Shared by tests/test_lazy_field_cpu.py (the
model against exact arithmetic) and tests/test_gpu_lazy_field.py (the device against exact arithmetic, on the same operands)."""
import itertools

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
W = 7

# the aimed operand values: both ends of each 32-bit half, the carry edges of the reduction (EPS = 2^32 - 1 and EPS + 1 = 2^32,
# which the list names twice on purpose: the batch keeps its 8^4 places), the ends of the canonical range and of the register
AIMS = (0, 1, (1 << 32) - 1, 1 << 32, EPS + 1, P - 1, P, (1 << 64) - 1)


def fits(v, bits):
    assert 0 <= v < (1 << bits), "an intermediate of %d bits in a register of %d" % (v.bit_length(), bits)
    return v


def mul_wide(a, b):
    """gl::mul_wide: the 128-bit product as four 32-bit limbs, by five multiply-adds into 64-bit register pairs"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p0 = fits(a0 * b0, 64)
    p1 = fits(a0 * b1 + (p0 >> 32), 64)
    p2 = fits(a1 * b0 + (p1 & M32), 64)
    p3 = fits(a1 * b1 + (p1 >> 32), 64)
    p3 = fits((p2 >> 32) * 1 + p3, 64)
    w = [p0 & M32, p2 & M32, p3 & M32, p3 >> 32]
    assert sum(x << (32 * i) for i, x in enumerate(w)) == a * b
    return w


def canon(x):
    """gl::canon: x + EPS carries out of 2^64 exactly when x >= p, and the wrapped sum is then x - p"""
    t = x + EPS
    return t & M64 if t >> 64 else x


def sub(a, b):
    """gl::sub, any u64 minus canonical: a borrow is worth -EPS and the correction cannot borrow again"""
    assert b < P
    d = a - b
    if d < 0:
        d += 1 << 64
        d = fits(d - EPS, 64)
    return d


def reduce160(w, canonical=True):
    """gl::reduce160 / reduce160_loose of five 32-bit limbs, lowest first"""
    w0, w1, w2, w3, w4 = (fits(x, 32) for x in w)
    r = ((w1 << 32) | w0) - w3                      # (w1:w0) - w3, a borrow is worth -EPS
    if r < 0:
        r += 1 << 64
        r = fits(r - EPS, 64)
    r = w2 * EPS + r                                # one multiply-add, a carry out of 2^64 is worth +EPS
    if r >> 64:
        r = fits((r & M64) + EPS, 64)
    if canonical:
        r = canon(r)
        assert r < P
    return sub(r, fits(w4 << 32, 64))               # w4 2^32 <= p - 1: canonical for every w4


def ext_mul(x, y, canonical=True):
    """gl::mul(Ext, Ext), device form: any u64 operands, c1 = a0 b1 + a1 b0 and c0 = a0 b0 + 7 a1 b1 as 160-bit integers"""
    ab, ba = mul_wide(x[0], y[1]), mul_wide(x[1], y[0])
    s, carry = [], 0
    for i in range(4):                              # four additions with carry, the last carry is the fifth limb
        t = fits(ab[i] + ba[i] + carry, 33)
        s.append(t & M32)
        carry = t >> 32
    s.append(carry)
    c1 = reduce160(s, canonical)
    aa, bb = mul_wide(x[0], y[0]), mul_wide(x[1], y[1])
    t, carry = [], 0
    for i in range(4):                              # limb * 7 + limb + carry: a multiply-add into a 64-bit pair
        v = fits(bb[i] * W + fits(aa[i] + carry, 64), 64)
        t.append(v & M32)
        carry = v >> 32
    t.append(fits(carry, 32))
    c0 = reduce160(t, canonical)
    return c0, c1


def ext_mul_exact(x, y):
    return (x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P


def reduce160_exact(w):
    return sum(x << (32 * i) for i, x in enumerate(w)) % P


def limbs_of(a0, a1, b1):
    """the five limbs nlx_ext_ops hands to reduce160: both halves of a0 and of a1, then the low half of b1"""
    return [a0 & M32, a0 >> 32, a1 & M32, a1 >> 32, b1 & M32]


def aimed_operands():
    """every combination of AIMS in the four slots (a0, a1, b0, b1): 4 096 cases.  The order is moved so that lanes 0, 31, 32
    and 63 of the first wave and the last element of the batch each see an extreme case (all four operands at an end of the
    range)."""
    cases = list(itertools.product(AIMS, repeat=4))
    top, pm1 = (1 << 64) - 1, P - 1
    extremes = {0: (top, top, top, top), 31: (pm1, pm1, pm1, pm1), 32: (P, P, P, P), 63: (top, pm1, pm1, top),
                len(cases) - 1: (top, top, pm1, pm1)}
    for at, case in extremes.items():
        j = cases.index(case)
        cases[at], cases[j] = cases[j], cases[at]
    for at, case in extremes.items():
        assert cases[at] == case
    assert len(cases) == 4096
    return cases


class GateAccModel:
    """one challenge's half of GateAcc (csrc/prover_kernels.hip): sum_k c_k b_k as four 64-bit columns of 32 x 32 partial
    products, a 32-bit carry counter each, folded into five limbs and reduced once (fold_columns -> gl::reduce160)"""

    def __init__(self):
        self.a, self.k, self.exact = [0] * 4, [0] * 4, 0

    def mac(self, c, b):
        c0, c1, b0, b1 = c & M32, c >> 32, b & M32, b >> 32
        for i, prod in enumerate((c0 * b0, c0 * b1, c1 * b0, c1 * b1)):
            t = self.a[i] + fits(prod, 64)
            self.a[i] = t & M64
            self.k[i] = fits(self.k[i] + (t >> 64), 32)
        self.exact += c * b

    def fold(self):
        A, K = self.a, self.k
        lo, hi = (lambda v: v & M32), (lambda v: v >> 32)

        def addc(x, y, c):
            t = fits(x, 32) + fits(y, 32) + c
            return t & M32, t >> 32
        m0, c = addc(lo(A[1]), lo(A[2]), 0)
        m1, c = addc(hi(A[1]), hi(A[2]), c)
        cm = c
        t1, c = addc(hi(A[0]), m0, 0)
        t2, c = addc(m1, lo(A[3]), c)
        t3, c = addc(cm, hi(A[3]), c)
        t4, c = addc(0, K[3], c)
        assert c == 0
        t2, c = addc(t2, K[0], 0)
        t3, c = addc(t3, K[1], c)
        t4, c = addc(0, t4, c)
        assert c == 0
        t3, c = addc(t3, K[2], 0)
        t4, c = addc(0, t4, c)
        assert c == 0
        w = [lo(A[0]), t1, t2, t3, t4]
        assert sum(x << (32 * i) for i, x in enumerate(w)) == self.exact
        return reduce160(w)


class GateAcc3Model:
    """one challenge's half of GateAcc3 (csrc/prover_kernels.hip, NLX_GATEACC_LIMBS3): the multiplier as three 22-bit limbs, six
    64-bit columns (constraint half h, limb j) of weight 2^(32 h + 22 j) and NO carry counters; the fold adds all but the top
    column as one 128-bit integer, splits the top column at bit 20 and subtracts its upper part after the reduction"""
    MAX_TERMS = 1024

    def __init__(self):
        self.a, self.exact, self.terms = [0] * 6, 0, 0

    @staticmethod
    def limbs(b):
        return [b & 0x3FFFFF, (b >> 22) & 0x3FFFFF, b >> 44]

    def mac(self, c, limbs):
        c0, c1 = c & M32, c >> 32
        for j, l in enumerate(limbs):
            fits(l, 22)
            self.a[j] = fits(self.a[j] + fits(c0 * l, 54), 64)          # no carry counter: the column itself must hold the sum
            self.a[3 + j] = fits(self.a[3 + j] + fits(c1 * l, 54), 64)
        self.exact += c * sum(l << (22 * j) for j, l in enumerate(limbs))
        self.terms += 1

    def fold(self):
        A = self.a
        t = fits(A[0] + (A[1] << 22) + (A[2] << 44) + (A[3] << 32) + (A[4] << 54) + ((A[5] & 0xFFFFF) << 76), 128)
        r = reduce160([(t >> (32 * i)) & M32 for i in range(4)] + [0])
        top = A[5] >> 20
        assert top < P and t + (top << 96) == self.exact
        return sub(r, top)
