"""Aimed Poseidon states: inputs whose state at a chosen layer is a chosen worst case.

Both permutations are invertible (the S-boxes x^7 mod p and x^5 mod r are permutations of their fields, the MDS matrices are
invertible), so any layer's input can be chosen and the permutation run backwards to the input state that produces it.  An edge
INPUT is gone after the first round; an aimed state puts the edge into the layer itself - the byte planes of a Goldilocks linear
layer, a fused block's S-box inputs, a BN128 MDS row - where the device's bounds are tight.

Goldilocks (tools/gen_poseidon_blocks.py, naive schedule): round r adds rc[r], applies the S-box (all twelve elements in a full
round, element 0 in a partial one) and multiplies by M.  Layer r's input is the state after round r's S-boxes (the MDS input);
an S-box input is the state after round r's constants.  The device holds the fused blocks' states in its own basis: inside
blocks 0 .. 6 (rounds 4 .. 24) and at round 25 it holds true state - delta, delta the offset of the generator's `constants()`;
`device_offset(layer)` gives it, so that aiming at `z_held + device_offset(layer)` puts z_held into the device's byte planes.

PoseidonBN128 (tools/gen_poseidon_bn128.py `permute`): the same construction with the 4 x 4 Cauchy MDS matrix, x^5, 64 rounds.
The device holds every element in Montgomery form (x 2^261 mod r, csrc/poseidon_bn128.hpp); `mont_aim(v)` is the residue whose
Montgomery form is v, so that v itself reaches the device's limbs.

A plain module (not a conftest): the CPU tests check the construction against the models, the GPU tests use it."""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_blocks as gpb  # noqa: E402
import gen_poseidon_bn128 as pbn  # noqa: E402
from gen_poseidon_constants import round_constants  # noqa: E402


def inverse_matrix(a, mod):
    """a^-1 mod a prime, by Gauss-Jordan elimination"""
    n = len(a)
    w = [[x % mod for x in row] + [1 if i == j else 0 for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        piv = next(r for r in range(c, n) if w[r][c])
        w[c], w[piv] = w[piv], w[c]
        inv = pow(w[c][c], -1, mod)
        w[c] = [x * inv % mod for x in w[c]]
        for r in range(n):
            if r != c and w[r][c]:
                f = w[r][c]
                w[r] = [(x - f * y) % mod for x, y in zip(w[r], w[c])]
    return [row[n:] for row in w]


def _matvec(a, v, mod):
    return [sum(x * y for x, y in zip(row, v)) % mod for row in a]


# ---- Goldilocks Poseidon ------------------------------------------------------------------------------------------------------
P = gpb.P
T = gpb.T
NR = gpb.NR
EPS = (1 << 32) - 1
RC = round_constants()
M = gpb.mds()
MINV = inverse_matrix(M, P)
SBOX_INV = pow(7, -1, P - 1)
PARTIAL = range(gpb.RF_HALF, gpb.RF_HALF + gpb.RP)          # rounds 4 .. 25


def is_full(r):
    return r not in PARTIAL


def sbox_inv(x):
    return pow(x, SBOX_INV, P)


def trace(state):
    """the naive permutation, keeping every round's S-box input and MDS input: (sbox_in[30], mds_in[30], output)"""
    s = [x % P for x in state]
    sbox_in, mds_in = [], []
    for r in range(NR):
        s = [(x + RC[r * T + i]) % P for i, x in enumerate(s)]
        sbox_in.append(list(s))
        s = [gpb.sbox(x) for x in s] if is_full(r) else [gpb.sbox(s[0])] + s[1:]
        mds_in.append(list(s))
        s = _matvec(M, s, P)
    return sbox_in, mds_in, s


def inverse_permute_to(layer, z):
    """the input state whose MDS input (after the S-boxes) at round `layer` is z (twelve residues)"""
    s = [x % P for x in z]
    for r in range(layer, -1, -1):
        if r < layer:
            s = _matvec(MINV, s, P)
        s = [sbox_inv(x) for x in s] if is_full(r) else [sbox_inv(s[0])] + s[1:]
        s = [(x - RC[r * T + i]) % P for i, x in enumerate(s)]
    return s


def inverse_to_sbox_input(r, w0, rest):
    """partial round r: the input state whose element-0 S-box input at round r is w0, the other eleven elements of that round's
    MDS input being `rest`.  Inside a fused block the device computes these S-box inputs (u1 / u2's arguments) as dot products
    on the vector pipe."""
    assert r in PARTIAL and len(rest) == T - 1
    return inverse_permute_to(r, [gpb.sbox(w0 % P)] + list(rest))


_OFFSETS = None


def device_offset(layer):
    """true MDS input - the device's held one at `layer`: delta_b at the first round of block b (layers 4, 7, .., 22), the
    offset layer 26 settles at layer 25, zero elsewhere (the full rounds hold the true state; inside a block only element 0 is
    held in byte planes again, and delta[0] = 0)"""
    global _OFFSETS
    if _OFFSETS is None:
        deltas = []
        gpb.constants(gpb.tables(), deltas)
        _OFFSETS = deltas
    first = gpb.FIRST
    if first <= layer < first + gpb.K * gpb.N_BLOCKS and (layer - first) % gpb.K == 0:
        return list(_OFFSETS[(layer - first) // gpb.K])
    if layer == first + gpb.K * gpb.N_BLOCKS:
        return list(_OFFSETS[-1])
    return [0] * T


def block_start_layers():
    """the layers held in the device's own basis: the first round of every fused block, and round 25"""
    return [gpb.FIRST + gpb.K * b for b in range(gpb.N_BLOCKS)] + [gpb.FIRST + gpb.K * gpb.N_BLOCKS]


def inverse_permute_to_held(layer, z_held):
    """the input state whose MDS input at `layer`, as the device holds it, is z_held"""
    d = device_offset(layer)
    return inverse_permute_to(layer, [(x + y) % P for x, y in zip(z_held, d)])


# one 64-bit value per element: each one a worst case of the byte planes or of a fold
GL_VALUES = {
    "zero": 0,                          # may be held as p = FFFFFFFF00000001
    "p-1": P - 1,                       # FFFFFFFF00000000
    "p-2": P - 2,                       # FFFFFFFEFFFFFFFF: the largest bytes a canonical value has
    "eps-1": EPS - 1,                   # FFFFFFFE: its loose form p + x is 2^64 - 1, every byte 0xFF
    "eps": EPS,                         # 2^32 - 1
    "bias0": 0x8080808080808080,        # every biased byte 0
    "bias-1": 0x7F7F7F7F7F7F7F7F,       # every biased byte -1
    "alt": 0xFF00FF00FF00FF00,          # alternating 0x00 / 0xFF bytes
    "alt'": 0x00FF00FF00FF00FF,
}
_HALVES = [("p-2", "zero"), ("p-1", "eps"), ("bias0", "bias-1"), ("alt", "alt'"), ("eps-1", "zero")]


def gl_patterns():
    """(name, twelve residues): every value across the state, half / half splits (so that the circulant's row sums reach both
    ends), and the row-maximising mix for output 0 (its largest coefficients, the +8 diagonal among them, at p - 2) with its
    complement"""
    out = [("fill " + k, [v] * T) for k, v in GL_VALUES.items()]
    for a, b in _HALVES:
        out.append(("half %s/%s" % (a, b), [GL_VALUES[a]] * 6 + [GL_VALUES[b]] * 6))
        out.append(("half %s/%s" % (b, a), [GL_VALUES[b]] * 6 + [GL_VALUES[a]] * 6))
    big = [M[0][j] >= 17 for j in range(T)]
    out.append(("row0 max", [P - 2 if b else 0 for b in big]))
    out.append(("row0 min", [0 if b else P - 2 for b in big]))
    return out


@functools.lru_cache(None)
def gl_aims():
    """(name, input state, (kind, layer, target)) for every pattern at every layer's MDS input in the naive basis, at the
    block-start layers in the device's basis, and every value at element 0's S-box input of every partial round.
    kind: "mds" (naive), "held" (device basis) or "sbox0".  Cached: treat as read-only."""
    pats = gl_patterns()
    out = []
    for layer in range(NR):
        for name, z in pats:
            out.append(("%s @ mds %d" % (name, layer), inverse_permute_to(layer, z), ("mds", layer, z)))
    for layer in block_start_layers():
        for name, z in pats:
            out.append(("%s @ held %d" % (name, layer), inverse_permute_to_held(layer, z), ("held", layer, z)))
    for r in PARTIAL:
        for name, v in GL_VALUES.items():
            out.append(("%s @ sbox0 %d" % (name, r), inverse_to_sbox_input(r, v, [v] * (T - 1)), ("sbox0", r, v)))
    return out


def gl_rate_row(z8, row_len):
    """a sponge row whose every absorb puts z8[j] at slot j of the first layer's MDS input: with the overwrite sponge, slot j of
    each absorb's state is the row element itself, so element c of the row is sbox^-1(z8[c % 8]) - rc[0][c % 8]"""
    return [(sbox_inv(z8[c % 8] % P) - RC[c % 8]) % P for c in range(row_len)]


# ---- PoseidonBN128 -------------------------------------------------------------------------------------------------------------
R = pbn.R
BT = pbn.T
BROUNDS = pbn.RF + pbn.RP
BRC, BMDS = pbn.constants()
BMINV = inverse_matrix(BMDS, R)
SBOX5_INV = pow(5, -1, R - 1)
MONT = 1 << 261                      # the device's Montgomery radix R' (csrc/bn254_f29.hpp)
MONT_INV = pow(MONT, -1, R)
LIMB_MASK = (1 << pbn.LB) - 1
LIMBS_AT_MASK = (((R >> 232) - 1) << 232) | ((1 << 232) - 1)   # limbs 0 .. 7 at MASK, limb 8 the largest that keeps it below r


def bn_is_full(rnd):
    return rnd < pbn.RF // 2 or rnd >= pbn.RF // 2 + pbn.RP


def bn_trace(state):
    """the model's permutation, keeping every round's S-box input and MDS input: (sbox_in[64], mds_in[64], output)"""
    s = [int(v) % R for v in state]
    sbox_in, mds_in = [], []
    for rnd in range(BROUNDS):
        s = [(s[i] + BRC[rnd * BT + i]) % R for i in range(BT)]
        sbox_in.append(list(s))
        s = [pow(v, 5, R) for v in s] if bn_is_full(rnd) else [pow(s[0], 5, R)] + s[1:]
        mds_in.append(list(s))
        s = _matvec(BMDS, s, R)
    return sbox_in, mds_in, s


def bn_inverse_to(rnd, target, where="mds"):
    """the input state whose S-box input (where="sbox") or MDS input (where="mds") at round `rnd` is `target`"""
    s = [int(v) % R for v in target]
    if where == "sbox":
        s = [pow(v, 5, R) for v in s] if bn_is_full(rnd) else [pow(s[0], 5, R)] + s[1:]
    for r in range(rnd, -1, -1):
        if r < rnd:
            s = _matvec(BMINV, s, R)
        s = [pow(v, SBOX5_INV, R) for v in s] if bn_is_full(r) else [pow(s[0], SBOX5_INV, R)] + s[1:]
        s = [(v - BRC[r * BT + i]) % R for i, v in enumerate(s)]
    return s


def mont_aim(v):
    """the residue whose Montgomery form is v: aiming at it puts v into the device's limbs"""
    return v * MONT_INV % R


def bn_patterns():
    """(name, four residues): the canonical extremes, and the same extremes as the device's Montgomery limbs"""
    r1 = R - 1
    plain = [("r-1", [r1] * 4), ("0", [0] * 4), ("1", [1] * 4), ("r-2", [R - 2] * 4), ("limbs at MASK", [LIMBS_AT_MASK] * 4),
             ("r-1,0,r-1,0", [r1, 0, r1, 0]), ("0,r-1,0,r-1", [0, r1, 0, r1])]
    mont = [("mont " + k, [mont_aim(x) for x in v]) for k, v in plain if k in ("r-1", "r-2", "limbs at MASK", "r-1,0,r-1,0")]
    return plain + mont


@functools.lru_cache(None)
def bn_aims():
    """(name, input state, (where, round, target)) for every pattern at every round's S-box input and MDS input.  Cached: treat
    as read-only."""
    out = []
    for rnd in range(BROUNDS):
        for where in ("sbox", "mds"):
            for name, v in bn_patterns():
                out.append(("%s @ %s %d" % (name, where, rnd), bn_inverse_to(rnd, v, where), (where, rnd, v)))
    return out


# ---- placing aimed items in a batch --------------------------------------------------------------------------------------------
LANE_CLASSES = (0, 1, 31, 32, 33, 63)   # lanes n and n + 32 take different K halves and result rows of the matrix cores


def placement(n_items, n=None, tail=37):
    """(batch size, {position: item}): wave w's lanes LANE_CLASSES[c] hold item (w - c) mod n_items, so that with at least
    n_items full waves every item sits at every lane class; by default the batch is 64 n_items + `tail` (a ragged last wave)
    long.  The last position holds item 0: the last item's lane is copied into the spare lanes of the last wave."""
    n = 64 * n_items + tail if n is None else n
    where = {}
    for w in range(n // 64):
        for c, lane in enumerate(LANE_CLASSES):
            where[64 * w + lane] = (w - c) % n_items
    where[n - 1] = 0
    return n, where
