"""Python-integer model of the device field multiply of csrc/gl.hpp (gl::mul_chain, gl::reduce128_core; gl32::mul and
gl::mul_loose_asm are these two, gl::mul_wide is the chain), limb by limb, with the device code's limb widths and order of
operations.  Every intermediate is checked against the width of the register (pair) that holds it on the device.  Shared by
tests/test_field_mul_model.py (the model against exact arithmetic) and tests/test_gpu_field_mul_aims.py (the device against
exact arithmetic, on the same operands).

The chain lets its third multiply-add overflow: the carry k has weight 2^96 = -1 (mod p) and enters the reduction as the
borrow-in of its first subtraction.  Both reductions are modelled: the eight-instruction one (borrow repair, then w2 EPS) and the
seven-instruction one of -DNLX_FIELD_REDUCE7 ((w2 - borrow) EPS, with the wrap of w2 = 0 repaired by the last carry-in)."""
import random

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
W = 7


def fits(v, bits):
    assert 0 <= v < (1 << bits), "an intermediate of %d bits in a register of %d" % (v.bit_length(), bits)
    return v


def mul_chain(a, b):
    """gl::mul_chain: (w0, w1, w2, w3, k) with a b = w0 + 2^32 w1 + 2^64 w2 + 2^96 (w3 + k)"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p0 = fits(a0 * b0, 64)
    p1 = fits(a0 * b1 + (p0 >> 32), 64)
    p2 = a1 * b0 + p1                      # the whole of p1 is the addend: this one may carry out of the pair
    k = fits(p2 >> 64, 1)
    p2 &= M64
    p3 = fits(a1 * b1 + (p2 >> 32), 64)
    w = (p0 & M32, p2 & M32, p3 & M32, p3 >> 32)
    assert sum(x << (32 * i) for i, x in enumerate(w)) + (k << 96) == a * b
    fits(w[3] + k, 32)
    return w + (k,)


def mul_chain_parent(a, b):
    """-DNLX_FIELD_MUL_PARENT: five multiply-adds none of which can overflow, k = 0"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p0 = fits(a0 * b0, 64)
    p1 = fits(a0 * b1 + (p0 >> 32), 64)
    p2 = fits(a1 * b0 + (p1 & M32), 64)
    p3 = fits(a1 * b1 + (p1 >> 32), 64)
    p3 = fits((p2 >> 32) * 1 + p3, 64)
    w = (p0 & M32, p2 & M32, p3 & M32, p3 >> 32)
    assert sum(x << (32 * i) for i, x in enumerate(w)) == a * b
    return w + (0,)


def _sub_w3_k(w0, w1, w3, k):
    """(w1:w0) - w3 - k as v_subb (borrow-in k) and v_subbrev: the wrapped 64-bit difference and its borrow"""
    t = fits(w0, 32) - fits(w3, 32) - fits(k, 1)
    r0, b0 = t & M32, int(t < 0)
    t = fits(w1, 32) - b0
    r1, b = t & M32, int(t < 0)
    assert ((r1 << 32) | r0) == (((w1 << 32) | w0) - w3 - k) % (1 << 64)
    return r0, r1, b


def reduce8(w0, w1, w2, w3, k=0):
    """gl::reduce128_core, eight instructions -> (loose result, (borrow, rare, final carry)); rare is never taken here"""
    r0, r1, b = _sub_w3_k(w0, w1, w3, k)
    t0 = M32 if b else 0                                   # v_cndmask
    t = r0 - t0                                            # v_sub_co: a borrow is worth -EPS
    r0, c = t & M32, int(t < 0)
    t = r1 - c                                             # v_subbrev
    assert t >= 0, "the borrow repair borrowed again"
    r1 = t
    base = (r1 << 32) | r0
    u = fits(w2, 32) * EPS + base                          # v_mad_u64_u32, carry-out in VCC
    c = fits(u >> 64, 1)
    u &= M64
    r = fits((M32 if c else 0) * 1 + u, 64)                # v_cndmask, v_mad_u64_u32: + EPS cannot carry again
    return r, (b, int(w2 == 0 and b == 1), c)


def reduce7(w0, w1, w2, w3, k=0):
    """gl::reduce128_core under NLX_FIELD_REDUCE7 -> (loose result, (borrow, rare, final carry))"""
    r0, r1, b = _sub_w3_k(w0, w1, w3, k)
    t = fits(w2, 32) - b                                   # v_subbrev m, bad, 0, w2, vcc
    m, bad = t & M32, int(t < 0)
    assert bad == int(w2 == 0 and b == 1)
    base = (r1 << 32) | r0
    u = m * EPS + base                                     # v_mad_u64_u32, carry-out in VCC
    c = fits(u >> 64, 1)
    u &= M64
    t = (u & M32) + (M32 if c else 0) + bad                # v_cndmask, v_addc (carry-in bad)
    lo, c2 = t & M32, t >> 32
    hi = fits((u >> 32) + c2, 32)                          # v_addc: cannot carry out
    return (hi << 32) | lo, (b, bad, c)


def mul8(a, b):
    w = mul_chain(a, b)
    r, cls = reduce8(*w)
    return r, (w[4],) + cls


def mul7(a, b):
    w = mul_chain(a, b)
    r, cls = reduce7(*w)
    return r, (w[4],) + cls


def mul_parent(a, b):
    w = mul_chain_parent(a, b)
    return reduce8(*w)[0]


def classify(a, b):
    """(k, borrow, rare, final carry) of a product; the final carry is the seven-instruction form's (its multiplier differs
    from the eight-instruction form's only when there was a borrow)"""
    return mul7(a, b)[1]


def classify8(a, b):
    return mul8(a, b)[1]


# ---- the extension product on this chain (gl::mul_impl): one k of each component is the reduction's borrow-in, the other
# product's k goes into its limb 3 (fold_k) ----
def canon(x):
    t = x + EPS
    return t & M64 if t >> 64 else x


def sub(a, b):
    assert b < P
    d = a - b
    if d < 0:
        d = fits(d + (1 << 64) - EPS, 64)
    return d


def fold_k(w):
    return w[:3] + (fits(w[3] + w[4], 32), 0)


def reduce160(w, k, reduce=reduce8):
    r = canon(reduce(w[0], w[1], w[2], w[3], k)[0])
    return sub(r, fits(w[4] << 32, 64))


def ext_mul(x, y, reduce=reduce8):
    ab, ba = mul_chain(x[0], y[1]), fold_k(mul_chain(x[1], y[0]))
    s, carry = [], 0
    for i in range(4):
        t = fits(ab[i] + ba[i] + carry, 33)
        s.append(t & M32)
        carry = t >> 32
    s.append(carry)
    c1 = reduce160(s, ab[4], reduce)
    aa, bb = mul_chain(x[0], y[0]), fold_k(mul_chain(x[1], y[1]))
    t, carry = [], 0
    for i in range(4):
        v = fits(bb[i] * W + fits(aa[i] + carry, 64), 64)
        t.append(v & M32)
        carry = v >> 32
    t.append(fits(carry, 32))
    c0 = reduce160(t, aa[4], reduce)
    return c0, c1


def ext_mul_exact(x, y):
    return (x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P


# ---- operands ----
# one hit (at least) per class (k, borrow, rare, final carry); the first five are the ones the derivation names
KNOWN_HITS = (
    (1 << 63, 1 << 33),                               # the rare case: w2 = 0 with a borrow
    (0x7FFFFFFF00000000, 0x7FFFFFFF00000000),         # k = 0, borrow, no final carry
    (0xD17F6494FFFFFFFE, 0xFFFFFFFF0A248CFF),         # k = 1, no borrow, no final carry
    (0xFFFFFFFF00000002, M64),                        # k = 1, borrow (w0 == w3, w1 == 0: caused by k alone), no final carry
    (M64, M64),                                       # k = 1, borrow, final carry
    (0, 0),                                           # k = 0, no borrow, no final carry
    (0xFFFFFFFE07D4BEDC, 0xAFBD67F9F06C144A),         # k = 0, no borrow, final carry
    (0xDDF688CFC57FEC86, 1 << 63),                    # k = 0, borrow, final carry
    (0xB610A9F7E5446DD4, 0xFFFFFFFFF79B17AE),         # k = 1, no borrow, final carry
)
# the classes (k, borrow, rare, final carry) the hits above are there for, in their order
KNOWN_CLASSES = ((0, 1, 1, 1), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 1), (0, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 1),
                 (1, 0, 0, 1))
EDGES = (0, 1, 2, EPS - 1, EPS, EPS + 1, EPS + 2, 1 << 33, 1 << 63, 0x7FFFFFFF00000000, 0x8000000000000000 - 1,
         P - 2, P - 1, P, P + 1, 0xFFFFFFFF00000002, M64 - 1, M64)
_WORDS = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)


def structured(rng):
    """a 64-bit operand whose halves are, one time in two each, an edge word"""
    lo = rng.choice(_WORDS) if rng.random() < 0.5 else rng.getrandbits(32)
    hi = rng.choice(_WORDS) if rng.random() < 0.5 else rng.getrandbits(32)
    return (hi << 32) | lo


def search_classes(n, seed):
    """{class: first pair that reaches it} over n structured random pairs"""
    rng, seen = random.Random(seed), {}
    for _ in range(n):
        a, b = structured(rng), structured(rng)
        seen.setdefault(classify(a, b), (a, b))
    return seen


def aimed_pairs():
    """the aimed operand pairs: the known hits, every pair of EDGES, and both orders of each"""
    out = list(KNOWN_HITS) + [(b, a) for a, b in KNOWN_HITS]
    out += [(a, b) for a in EDGES for b in EDGES]
    return out
