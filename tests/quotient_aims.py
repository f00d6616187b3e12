"""Aimed witnesses for the plonky2 quotient and Z / partial-product stages: wire, Z and partial-product polynomials whose values
at chosen LDE points are chosen worst cases.

The quotient is evaluated on the rate-8 LDE, at the point x = coset_base[r] * w_n^k of position r * n + k (class r, index k:
csrc/prover_kernels.hip point_of; csrc/prover.hip sets coset_base[r] = g * w_L^r with g the multiplicative generator and w_L the
2^(log_n + rate_bits)-th root of unity).  A polynomial of degree < n is fixed by its n values on any one class, so those values
can be chosen: their coset inverse NTT gives the coefficients (for a from_coeffs commitment), and the NTT of the coefficients the
witness on H (for a whole proof).  The prover then reads exactly the chosen values at those points; the other classes stay
random.  Z(w_n x) is index k + 1 of the same class.  k_quotient and k_quotient_poseidon put index k on lane k mod 64.

Every gate is evaluated at every point whatever its selector, so a "row" of 135 wire values at one point reaches every gate's
arithmetic at once: a PoseidonGate row that is an honest permutation trace through a poseidon_aims target, or a pattern of edge
values that gives the u32 / BaseSum / Comparison limb recombinations (Sum128, limb4) their extreme inputs.

A plain module (not a conftest): the CPU tests check the construction, the GPU tests use it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import poseidon_aims as pa  # noqa: E402
from conftest import GEN, POW2_GEN, P, rand_field  # noqa: E402

NUM_WIRES = 135
EPS = (1 << 32) - 1


# ---- the LDE points and the interpolation ---------------------------------------------------------------------------------------
def root(log_n):
    """the primitive 2^log_n-th root of unity (of the POWER_OF_TWO_GENERATOR in use)"""
    return pow(POW2_GEN, 1 << (32 - log_n), P)


def coset_base(r, log_n, rate_bits=3):
    """class r's shift: the prover's coset_base[r] = g * w_L^r"""
    return GEN * pow(root(log_n + rate_bits), r, P) % P


def point(r, k, log_n, rate_bits=3):
    """the LDE point of class r, index k"""
    return coset_base(r, log_n, rate_bits) * pow(root(log_n), k, P) % P


def lde_row(r, k, log_n, rate_bits=3):
    """the row of a commitment's (bit-reversed) leaves that holds point (r, k): natural LDE index (k << rate_bits) + r"""
    log_L = log_n + rate_bits
    i = (k << rate_bits) + r
    return int(format(i, "0%db" % log_L)[::-1], 2)


def interpolate(orc, targets, n_cols, log_n, rng, rate_bits=3):
    """targets {(column, class r, k): value} -> (coefficients, values on H), each (n_cols, n).  A column's targets must share one
    class; its other n - (targets) values on that class, and every column without targets, are random."""
    n = 1 << log_n
    cls = {}
    for (c, r, _k) in targets:
        assert cls.setdefault(c, r) == r, "column %d is aimed at two classes" % c
    vals = rand_field(rng, (n_cols, n))
    coeffs = np.zeros((n_cols, n), dtype=np.uint64)
    for (c, _r, k), v in targets.items():
        vals[c, k] = int(v) % P
    for c in range(n_cols):
        if c in cls:
            coeffs[c] = orc.fft(vals[c], inverse=True, shift=coset_base(cls[c], log_n, rate_bits))
        else:
            coeffs[c] = orc.fft(vals[c], inverse=True)
    on_h = np.stack([orc.fft(coeffs[c]) for c in range(n_cols)])
    return coeffs, on_h


def rows_to_targets(rows, r):
    """{k: row of 135 values (None = free)} at class r -> interpolate()'s targets"""
    return {(c, r, k): v for k, row in rows.items() for c, v in enumerate(row) if v is not None}


# ---- gate rows ---------------------------------------------------------------------------------------------------------------
def poseidon_gate_row(inputs, swap=0):
    """PoseidonGate's 135 wires for an honest permutation of `inputs` (swap: the first two 4-element words exchanged):
    inputs 0..11, outputs 12..23, swap 24, deltas 25..28, full rounds 1..3's S-box inputs 29..64, the 22 partial rounds' element-0
    S-box inputs 65..86, full rounds 26..29's S-box inputs 87..134"""
    inp = [int(x) % P for x in inputs]
    st = list(inp)
    if swap:
        st[0:4], st[4:8] = inp[4:8], inp[0:4]
    sbox_in, _mds_in, out = pa.trace(st)
    row = [0] * NUM_WIRES
    row[0:12] = inp
    row[12:24] = out
    row[24] = swap
    row[25:29] = [swap * (inp[i + 4] - inp[i]) % P for i in range(4)]
    for r in range(1, 4):
        row[29 + 12 * (r - 1): 41 + 12 * (r - 1)] = sbox_in[r]
    row[65:87] = [sbox_in[4 + j][0] for j in range(22)]
    for r in range(4):
        row[87 + 12 * r: 99 + 12 * r] = sbox_in[26 + r]
    return row


def poseidon_gate_aims():
    """(name, permutation input, target) of poseidon_aims.gl_aims() at every fused-block start in the device's basis, every full
    round's MDS input and element 0's S-box input of every partial round"""
    return [a for a in pa.gl_aims() if a[2][0] in ("held", "sbox0") or (a[2][0] == "mds" and pa.is_full(a[2][1]))]


# the edges of test_field_core_edge_values a canonical wire value can take
EDGES = [0, 1, 2, 3, EPS - 1, EPS, EPS + 1, EPS + 2, 2 * EPS, (1 << 33) - 1, 1 << 33, 1 << 48, (1 << 63) - 1, 1 << 63, (1 << 63) + 1,
         P - 2, P - 1, 0xFFFFFFFE00000001, 0x00000001FFFFFFFF, 0xFFFFFFFEFFFFFFFF, 0x8000000080000000, 0x7FFFFFFF7FFFFFFF,
         0xAAAAAAAA55555555]
PAIR_EDGES = [0, 1, EPS, EPS + 1, 1 << 63, P - 2, P - 1, 0xFFFFFFFEFFFFFFFF]


def gate_rows():
    """(name, 135 wire values): every edge in every wire; every ordered pair of PAIR_EDGES alternating wire by wire (x op y for
    the arithmetic gates' operand pairs, both halves of an extension element); the u32 limb patterns 0 / 2^32 - 1 / 2^32 and
    p - 1 / 2^32 - 1 cycling through the wires, so that every limb of the U32 gates, BaseSumGate and ComparisonGate sits at its
    extremes and every recombination (Sum128, limb4) meets its largest totals"""
    out = [("fill %#x" % v, [v] * NUM_WIRES) for v in EDGES]
    for a in PAIR_EDGES:
        for b in PAIR_EDGES:
            if a != b:
                out.append(("pair %#x/%#x" % (a, b), [a if c % 2 == 0 else b for c in range(NUM_WIRES)]))
    cycles = [(0, EPS, EPS + 1), (EPS, EPS + 1, 0), (EPS + 1, 0, EPS), (P - 1, EPS), (EPS, P - 1), (P - 1, P - 1, 0),
              (P - 1, 0, 0, 0), (EPS, EPS, EPS, 0)]
    for cyc in cycles:
        out.append(("cycle " + "/".join("%#x" % v for v in cyc), [cyc[c % len(cyc)] for c in range(NUM_WIRES)]))
    return out


def gate_aim_rows(shift=0):
    """every gate_rows() row and every PoseidonGate aim as (name, 135 wire values); the Poseidon rows rotated by `shift` so that
    the gate rows can go to the lane classes and the permutation traces to the other positions"""
    pos = poseidon_gate_aims()
    prow = [("poseidon %s%s" % (name, " swapped" if i % 2 else ""), poseidon_gate_row(inp if i % 2 == 0 else _unswap(inp), i % 2))
            for i, (name, inp, _t) in enumerate(pos)]
    s = shift % len(prow)
    return gate_rows(), prow[s:] + prow[:s]


def _unswap(inp):
    """the gate input that, swapped, gives the permutation input `inp`"""
    return list(inp[4:8]) + list(inp[0:4]) + list(inp[8:12])


def permutation_positions(log_n):
    """the indices a stage test keeps for permutation_rows: lanes 2 - 5 and 34 - 37 of every wave (none of them a lane class)"""
    return [k for k in range(1 << log_n) if k % 32 in (2, 3, 4, 5)]


def place_rows(gate_rows_, poseidon_rows, log_n, skip=()):
    """{k: (name, row)} over the n indices of a class but `skip`: the gate rows round-robin over the indices at a lane class
    (poseidon_aims.LANE_CLASSES), those that find none there at the first other indices, the Poseidon rows at the rest, as many
    times as they fit"""
    n = 1 << log_n
    skip = set(skip)
    lane_pos = [k for k in range(n) if k % 64 in pa.LANE_CLASSES and k not in skip]
    other = [k for k in range(n) if k % 64 not in pa.LANE_CLASSES and k not in skip]
    out = {k: gate_rows_[j % len(gate_rows_)] for j, k in enumerate(lane_pos)}
    for k, row in zip(other, gate_rows_[len(lane_pos):]):
        out[k] = row
    rest = [k for k in other if k not in out]
    for j, k in enumerate(rest):
        out[k] = poseidon_rows[j % len(poseidon_rows)]
    return out


# ---- the permutation argument ------------------------------------------------------------------------------------------------
# numerator / denominator factors w + beta k_i x + gamma, w + beta sigma_i(x) + gamma aimed at these (a denominator never at 0:
# plonky2 leaves a zero denominator undefined)
FACTOR_TARGETS = [0, 1, P - 1, P - 2, EPS, EPS + 1, 1 << 63, 0xFFFFFFFEFFFFFFFF, 2]


def permutation_rows(k_is, sigma_at, beta, gamma, xs, routed=80, zero_numerators=True):
    """{k: row} for the points xs {k: x}: routed wires aimed so that, for this (beta, gamma), every numerator factor (even
    positions m of xs) or every denominator factor (odd m) takes a FACTOR_TARGETS value, wire j at the m-th point taking target
    (m + j) mod 9.  The denominator is the numerator + beta (sigma_j(x) - k_j x): where that would make it 0 - a wire the
    permutation leaves in place has sigma_j(x) = k_j x, so its numerator 0 is a denominator 0 - the next target is taken, and
    a denominator aimed at 0 takes 3.  sigma_at(j, k): sigma_j at xs[k].  zero_numerators=False skips the numerator 0 too (on H
    it zeroes Z from the next row on).  The non-routed wires stay free."""
    rows = {}
    nt = len(FACTOR_TARGETS)
    for m, (k, x) in enumerate(xs.items()):
        row = [None] * NUM_WIRES
        for j in range(routed):
            kx, s = int(k_is[j]) * x % P, sigma_at(j, k) % P
            if m % 2 == 0:
                t = next(t for t in (FACTOR_TARGETS[(m + j + i) % nt] for i in range(nt))
                         if (t + beta * (s - kx)) % P and (t or zero_numerators))
                row[j] = (t - beta * kx - gamma) % P
            else:
                t = FACTOR_TARGETS[(m + j) % nt] or 3
                row[j] = (t - beta * s - gamma) % P
        rows[k] = row
    return rows


ZS_EDGES = [0, 1, P - 1, P - 2, EPS, EPS + 1, 1 << 63, 0xFFFFFFFEFFFFFFFF, 2, 0x8000000080000000]


def zs_targets(n_zs, r, ks):
    """Z and partial-product polynomials at edge values on class r: column c at ks[m] takes ZS_EDGES[(m + c) mod 10]"""
    return {(c, r, k): ZS_EDGES[(m + c) % len(ZS_EDGES)] for m, k in enumerate(ks) for c in range(n_zs)}
