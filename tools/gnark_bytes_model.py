#!/usr/bin/env python3
"""gnark's bytes for BN254 points and for the two containers built from them, on big integers: the place of record for every
byte rule of the device codec (csrc/bn254_codec.hpp) and of the readers / writers in bn254_plonk.py and bn254_groth16.py, and
what the tests compare them with.  Pure Python: Fq and Fq2 on integers, square roots by `pow`, no other file of the project.

Status of every rule: RECALLED from gnark v0.9 (backend/groth16/bn254/marshal.go) and gnark-crypto (ecc/bn254/marshal.go,
ecc/bn254/kzg/marshal.go, fft/domain.go), UNPINNED - there is no Go source and no gnark-produced file to compare with, like the
rest of row f.4.  Each rule is written once, here.

  rule 1  flags      the top two bits of the first byte: 00 raw point, 01 the point at infinity, 10 / 11 compressed with the
                     smaller / larger y.  00 is valid only in raw mode, 10 and 11 only in compressed mode
  rule 2  infinity   0x40 and zeros, 32 / 64 (G1 / G2) bytes compressed and 64 / 128 raw; words: all zero.  Any other bit set
                     next to flag 01 is malformed
  rule 3  G1         X big-endian (, Y big-endian), canonical integers below q; y^2 = x^3 + 3
  rule 4  G2         X.A1 || X.A0 (|| Y.A1 || Y.A0) over Fq[u] / (u^2 + 1); y^2 = x^3 + 3 / (9 + u); the point is in the
                     subgroup of order r (both modes test it, unless switched off)
  rule 5  largest    y > (q - 1) / 2 as a canonical integer; over Fq2 decided on A1, on A0 when A1 is zero
  rule 6  status     the first failing check in this order: infinity's zeros, the flag for the mode, every coordinate below
                     q, the curve (compressed: a root exists), the subgroup                                   (g1_decode, g2_decode)
  rule 7  words      a coordinate in memory is its Montgomery form x 2^256 mod q as four little-endian 64-bit words;
                     G1Affine = X Y, G2Affine = X.A0 X.A1 Y.A0 Y.A1
  rule 8  scalars    uint32 and uint64 big-endian; a slice of points is a uint32 count and its points; a []bool is a uint32
                     count and one byte each
  rule 9  SRS        kzg.SRS.WriteTo: slice Pk.G1, Vk.G2[0], Vk.G2[1], Vk.G1                                 (srs_bytes, srs_parse)
  rule 10 key        groth16.ProvingKey.WriteTo / WriteRawTo: the domain (uint64 cardinality; CardinalityInv, Generator,
                     GeneratorInv, FrMultiplicativeGen, FrMultiplicativeGenInv as 32-byte big-endian canonical Fr); G1 Alpha,
                     Beta, Delta, slices A, B, Z, K; G2 Beta, Delta, slice B; uint64 nbWires, NbInfinityA, NbInfinityB; []bool
                     InfinityA, InfinityB; uint32 k and per commitment key the slices Basis, BasisExpSigma     (key_bytes, key_parse)
"""
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256
FR_GENERATOR = 5                                      # FrMultiplicativeGen
ROOT_2_28 = pow(FR_GENERATOR, (R - 1) >> 28, R)
OK, BAD_FLAG, RANGE, BAD_INFINITY, OFF_CURVE, NOT_IN_SUBGROUP = range(6)
STATUS_NAMES = ("ok", "bad flag", "range", "bad infinity", "off curve", "not in subgroup")
G1_SIZE = {False: 32, True: 64}                       # bytes of a point, by raw
G2_SIZE = {False: 64, True: 128}


# ---- Fq2 = Fq[u] / (u^2 + 1): pairs (a0, a1) ----
def f2_add(a, b):
    return (a[0] + b[0]) % Q, (a[1] + b[1]) % Q


def f2_sub(a, b):
    return (a[0] - b[0]) % Q, (a[1] - b[1]) % Q


def f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], Q - 2, Q)
    return a[0] * d % Q, -a[1] * d % Q


B2 = f2_mul((3, 0), f2_inv((9, 1)))                   # the twist's constant 3 / (9 + u)


def fq_sqrt(a):
    """a square root in Fq (q = 3 mod 4), or None"""
    a %= Q
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a else None


def f2_sqrt(a):
    """a square root in Fq2, or None, for q = 3 mod 4: b = a^((q - 3) / 4) in Fq2, alpha = a b^2; no root if alpha^(q + 1) = -1;
    x0 = a b; the root is u x0 if alpha = -1, else (1 + alpha)^((q - 1) / 2) x0 (Adj and Rodriguez-Henriquez, "Square root
    computation over even extension fields", algorithm 9).  Shares nothing with the device's norm method."""
    a = (a[0] % Q, a[1] % Q)
    if a == (0, 0):
        return (0, 0)

    def f2_pow(x, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = f2_mul(r, r)
            if bit == "1":
                r = f2_mul(r, x)
        return r
    b = f2_pow(a, (Q - 3) // 4)
    x0 = f2_mul(a, b)
    alpha = f2_mul(x0, b)
    if f2_mul(alpha, (alpha[0], -alpha[1] % Q)) == (Q - 1, 0):
        return None
    y = f2_mul((0, 1), x0) if alpha == (Q - 1, 0) else f2_mul(f2_pow(f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    return y if f2_mul(y, y) == a else None


# ---- rule 5 ----
def fq_largest(y):
    return int(y) % Q > (Q - 1) // 2


def f2_largest(y):
    return fq_largest(y[0]) if y[1] % Q == 0 else fq_largest(y[1])


# ---- the twist's group law, only for the subgroup test ----
def _g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if f2_add(p[1], q[1]) == (0, 0):
            return None
        lam = f2_mul(f2_mul((3, 0), f2_mul(p[0], p[0])), f2_inv(f2_add(p[1], p[1])))
    else:
        lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x = f2_sub(f2_sub(f2_mul(lam, lam), p[0]), q[0])
    return x, f2_sub(f2_mul(lam, f2_sub(p[0], x)), p[1])


def g2_mul_any(k, p):
    """k p for a twist point of any order"""
    acc = None
    for bit in bin(k)[2:]:
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return acc


def g1_on_curve(p):
    return p is None or (p[1] * p[1] - p[0] ** 3 - 3) % Q == 0


def g2_on_curve(p):
    return p is None or f2_mul(p[1], p[1]) == f2_add(f2_mul(f2_mul(p[0], p[0]), p[0]), B2)


def g2_in_subgroup(p):
    return p is None or g2_mul_any(R, p) is None


# ---- rule 7: words ----
def _words4(x):
    m = int(x) % Q * MONT % Q
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def g1_words(p):
    return [0] * 8 if p is None else _words4(p[0]) + _words4(p[1])


def g2_words(p):
    return [0] * 16 if p is None else _words4(p[0][0]) + _words4(p[0][1]) + _words4(p[1][0]) + _words4(p[1][1])


def _be(x):
    return int(x).to_bytes(32, "big")


# ---- rules 1 - 4: encode.  A point is None (infinity) or its affine coordinates; the curve is not tested (gnark does not) ----
def g1_encode(p, raw=False):
    if p is None:
        return bytes([0x40]) + bytes(G1_SIZE[raw] - 1)
    assert 0 <= p[0] < Q and 0 <= p[1] < Q
    if raw:
        return _be(p[0]) + _be(p[1])
    b = bytearray(_be(p[0]))
    b[0] |= 0xC0 if fq_largest(p[1]) else 0x80
    return bytes(b)


def g2_encode(p, raw=False):
    if p is None:
        return bytes([0x40]) + bytes(G2_SIZE[raw] - 1)
    (x0, x1), (y0, y1) = p
    assert all(0 <= c < Q for c in (x0, x1, y0, y1))
    if raw:
        return _be(x1) + _be(x0) + _be(y1) + _be(y0)
    b = bytearray(_be(x1) + _be(x0))
    b[0] |= 0xC0 if f2_largest((y0, y1)) else 0x80
    return bytes(b)


# ---- rules 1 - 6: decode -> (status, point); a bad point comes back as None (zero words) ----
def _coords(data, count):
    """the flag, and `count` coordinates with the flag bits dropped from the first"""
    c = [int.from_bytes(data[32 * i:32 * i + 32], "big") for i in range(count)]
    c[0] &= (1 << 254) - 1
    return data[0] >> 6, c


def _head(data, raw, flag):
    """rules 1 and 2 on one point's bytes: a status, or None to go on"""
    if flag == 1:
        return BAD_INFINITY if data[0] != 0x40 or any(data[1:]) else OK
    if (flag != 0) if raw else (flag == 0):
        return BAD_FLAG
    return None


def g1_decode(data, raw=False):
    assert len(data) == G1_SIZE[raw]
    flag, c = _coords(data, 2 if raw else 1)
    st = _head(data, raw, flag)
    if st is not None:
        return st, None
    if any(v >= Q for v in c):
        return RANGE, None
    x = c[0]
    if raw:
        y = c[1]
        if (y * y - x ** 3 - 3) % Q:
            return OFF_CURVE, None
    else:
        y = fq_sqrt(x ** 3 + 3)
        if y is None:
            return OFF_CURVE, None
        if fq_largest(y) != (flag == 3):
            y = -y % Q
    return OK, (x, y)


def g2_decode(data, raw=False, subgroup=True):
    assert len(data) == G2_SIZE[raw]
    flag, c = _coords(data, 4 if raw else 2)
    st = _head(data, raw, flag)
    if st is not None:
        return st, None
    if any(v >= Q for v in c):
        return RANGE, None
    x = (c[1], c[0])
    rhs = f2_add(f2_mul(f2_mul(x, x), x), B2)
    if raw:
        y = (c[3], c[2])
        if f2_mul(y, y) != rhs:
            return OFF_CURVE, None
    else:
        y = f2_sqrt(rhs)
        if y is None:
            return OFF_CURVE, None
        if f2_largest(y) != (flag == 3):
            y = (-y[0] % Q, -y[1] % Q)
    if subgroup and not g2_in_subgroup((x, y)):
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


# ---- rule 8 ----
def u32(x):
    return int(x).to_bytes(4, "big")


def u64(x):
    return int(x).to_bytes(8, "big")


def g1_slice(points, raw):
    return u32(len(points)) + b"".join(g1_encode(p, raw) for p in points)


def g2_slice(points, raw):
    return u32(len(points)) + b"".join(g2_encode(p, raw) for p in points)


def bool_slice(flags):
    return u32(len(flags)) + bytes(1 if f else 0 for f in flags)


class Reader:
    """walks a container: every read names its section, short data raises ValueError with that name"""

    def __init__(self, data):
        self.data, self.at = bytes(data), 0

    def take(self, n, section):
        if self.at + n > len(self.data):
            raise ValueError("truncated in %s: %d bytes wanted at offset %d, %d left" % (section, n, self.at, len(self.data) - self.at))
        out = self.data[self.at:self.at + n]
        self.at += n
        return out

    def u32(self, section):
        return int.from_bytes(self.take(4, section), "big")

    def u64(self, section):
        return int.from_bytes(self.take(8, section), "big")

    def point(self, g2, raw, section, subgroup=True):
        data = self.take((G2_SIZE if g2 else G1_SIZE)[raw], section)
        st, p = g2_decode(data, raw, subgroup) if g2 else g1_decode(data, raw)
        if st != OK:
            raise ValueError("%s: %s" % (section, STATUS_NAMES[st]))
        return p

    def points(self, g2, raw, section, subgroup=True):
        n = self.u32(section + " count")
        size = (G2_SIZE if g2 else G1_SIZE)[raw]
        if self.at + n * size > len(self.data):
            raise ValueError("truncated in %s: %d points of %d bytes wanted, %d bytes left" % (section, n, size, len(self.data) - self.at))
        out = []
        for i in range(n):
            data = self.take(size, section)
            st, p = g2_decode(data, raw, subgroup) if g2 else g1_decode(data, raw)
            if st != OK:
                raise ValueError("%s point %d: %s" % (section, i, STATUS_NAMES[st]))
            out.append(p)
        return out

    def bools(self, section):
        n = self.u32(section + " count")
        data = self.take(n, section)
        if any(b > 1 for b in data):
            raise ValueError("%s: a byte that is neither 0 nor 1" % section)
        return [b == 1 for b in data]

    def end(self, what):
        if self.at != len(self.data):
            raise ValueError("%s: %d trailing bytes" % (what, len(self.data) - self.at))


def container_is_raw(data, before, what):
    """the mode of a container, from the flag of its first point `what` (never the point at infinity).  before: the (section,
    size) pairs that precede it - a file that ends inside one of them is refused naming that one"""
    at = 0
    for section, size in before:
        if len(data) < at + size:
            raise ValueError("truncated in %s: %d bytes wanted at offset %d, %d left" % (section, size, at, len(data) - at))
        at += size
    if len(data) <= at:
        raise ValueError("truncated in %s: a point wanted at offset %d, 0 bytes left" % (what, at))
    flag = data[at] >> 6
    if flag == 1:
        raise ValueError("%s is the point at infinity" % what)
    return flag == 0


# ---- rule 9: kzg.SRS ----
def srs_bytes(g1, g2_0, g2_1, raw=False):
    """g1: the points [tau^i]_1; g2_0, g2_1: [1]_2 and [tau]_2; Vk.G1 is g1[0]"""
    return g1_slice(g1, raw) + g2_encode(g2_0, raw) + g2_encode(g2_1, raw) + g1_encode(g1[0], raw)


def srs_parse(data):
    if len(data) >= 4 and not any(data[:4]):
        raise ValueError("Pk.G1 is empty")
    raw = container_is_raw(data, [("Pk.G1 count", 4)], "Pk.G1")
    rd = Reader(data)
    g1 = rd.points(False, raw, "Pk.G1")
    if not g1:
        raise ValueError("Pk.G1 is empty")
    g2_0, g2_1 = rd.point(True, raw, "Vk.G2[0]"), rd.point(True, raw, "Vk.G2[1]")
    vk_g1 = rd.point(False, raw, "Vk.G1")
    rd.end("SRS")
    if vk_g1 != g1[0]:
        raise ValueError("Vk.G1 is not Pk.G1[0]")
    return g1, g2_0, g2_1


# ---- rule 10: groth16.ProvingKey ----
def root_of_unity(log_n):
    return pow(ROOT_2_28, 1 << (28 - log_n), R)


def domain_bytes(log_n):
    n, w = 1 << log_n, root_of_unity(log_n)
    return u64(n) + b"".join(_be(v) for v in (pow(n, R - 2, R), w, pow(w, R - 2, R), FR_GENERATOR, pow(FR_GENERATOR, R - 2, R)))


DOMAIN_BYTES = 8 + 5 * 32


def key_bytes(key, raw=False):
    """key: a dict - log_n, n_wires; g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta (points); g1_a, g1_b, g1_z, g1_k, g2_b (lists
    of points); infinity_a, infinity_b (lists of bools over the wires); commitments: a list of (basis, basis_exp_sigma)"""
    out = domain_bytes(key["log_n"])
    out += b"".join(g1_encode(key[k], raw) for k in ("g1_alpha", "g1_beta", "g1_delta"))
    out += b"".join(g1_slice(key[k], raw) for k in ("g1_a", "g1_b", "g1_z", "g1_k"))
    out += g2_encode(key["g2_beta"], raw) + g2_encode(key["g2_delta"], raw) + g2_slice(key["g2_b"], raw)
    out += u64(key["n_wires"]) + u64(sum(map(bool, key["infinity_a"]))) + u64(sum(map(bool, key["infinity_b"])))
    out += bool_slice(key["infinity_a"]) + bool_slice(key["infinity_b"])
    out += u32(len(key["commitments"]))
    for basis, sigma in key["commitments"]:
        out += g1_slice(basis, raw) + g1_slice(sigma, raw)
    return out


def key_parse(data):
    raw = container_is_raw(data, [("domain", DOMAIN_BYTES)], "G1.Alpha")
    rd = Reader(data)
    n = rd.u64("domain")
    if n == 0 or n & (n - 1) or n > 1 << 28:
        raise ValueError("domain: the cardinality %d is no power of two up to 2^28" % n)
    log_n = n.bit_length() - 1
    if rd.take(5 * 32, "domain") != domain_bytes(log_n)[8:]:
        raise ValueError("domain: not the domain of cardinality %d" % n)
    key = {"log_n": log_n}
    for k in ("g1_alpha", "g1_beta", "g1_delta"):
        key[k] = rd.point(False, raw, "G1." + k[3:].capitalize())
    for k in ("g1_a", "g1_b", "g1_z", "g1_k"):
        key[k] = rd.points(False, raw, "G1." + k[3:].upper())
    key["g2_beta"], key["g2_delta"] = rd.point(True, raw, "G2.Beta"), rd.point(True, raw, "G2.Delta")
    key["g2_b"] = rd.points(True, raw, "G2.B")
    key["n_wires"], nb_a, nb_b = rd.u64("nbWires"), rd.u64("NbInfinityA"), rd.u64("NbInfinityB")
    key["infinity_a"], key["infinity_b"] = rd.bools("InfinityA"), rd.bools("InfinityB")
    for name, mask, nb, pts in (("A", key["infinity_a"], nb_a, key["g1_a"]), ("B", key["infinity_b"], nb_b, key["g1_b"])):
        if len(mask) != key["n_wires"] or sum(mask) != nb or len(pts) != key["n_wires"] - nb:
            raise ValueError("Infinity%s: %d flags, %d set, NbInfinity%s %d, %d wires, %d points in G1.%s"
                             % (name, len(mask), sum(mask), name, nb, key["n_wires"], len(pts), name))
    if len(key["g2_b"]) != len(key["g1_b"]):
        raise ValueError("G2.B: %d points, G1.B has %d" % (len(key["g2_b"]), len(key["g1_b"])))
    if len(key["g1_z"]) != n - 1:
        raise ValueError("G1.Z: %d points, the domain wants %d" % (len(key["g1_z"]), n - 1))
    key["commitments"] = []
    for j in range(rd.u32("commitment keys count")):
        basis, sigma = rd.points(False, raw, "commitment key %d Basis" % j), rd.points(False, raw, "commitment key %d BasisExpSigma" % j)
        if len(basis) != len(sigma):
            raise ValueError("commitment key %d BasisExpSigma: %d points, Basis has %d" % (j, len(sigma), len(basis)))
        key["commitments"].append((basis, sigma))
    rd.end("proving key")
    return key
