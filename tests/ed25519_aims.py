"""Aimed Ed25519 slots: sixteen named slots (ax, ay, rx, ry, s, d, active) that drive the trace generator's scan (k_ed_scan4 on
fe25519_fast.hpp), its sixteen witness units per row and its reduction mod L to their extremes, in lists whose lengths make the
scan run a partially filled block (1, 2, 4, 8 slots), a full one and exactly two.

An inactive slot (active = 0) takes any coordinates below p, on the curve or not, any S < L and any 512-bit D: the reference
(ed25519_air.reference_slot) and the device generate its rows with the three checks off.  That is what reaches 0, p - 1 and
all-ones limbs; real signatures are random-looking field values.  The active slots are true statements built from chosen
scalars: [S]B = R + [D mod L]A with A = aB, R = rB, S = r + D a mod L.

ORDER alternates active and inactive slots, so the prefixes end on an active slot (1 and 16 slots) and on an inactive one (2, 4
and 8): row 0 of slot 0 holds the Y comparison of the LAST slot and so sees both values of its flag.  SIZES gives the lists the tests run.

A plain module (not a conftest): the CPU tests check the construction and the host build of the row code, the GPU tests the device.
The package is passed in (the `nlx` fixture) - the library must be built before it can be imported."""
import random

import numpy as np

P = (1 << 255) - 19
ORDER = ("random0", "off_extremes", "s_zero", "idle", "h_zero", "off_zero_pt_hzero", "a_order2", "off_26bit_half", "d_max",
         "off_order2", "s_lm1", "off_16bit_ones", "r_identity", "a_identity", "d_zero", "random1")
# (label, log_slots, names): the prefixes, the list followed by its reverse (two scan blocks, and every slot behind a
# predecessor it did not have before), and off_extremes alone (its own predecessor)
SIZES = tuple(("2^%d" % ls, ls, ORDER[:1 << ls]) for ls in range(5)) + (("2^5", 5, ORDER + ORDER[::-1]), ("extremes alone", 0, ("off_extremes",)))

_cache = {}


def slots(nlx):
    """{name: slot} of the sixteen aimed slots"""
    if "slots" in _cache:
        return _cache["slots"]
    E, NP = nlx.ed25519_air, nlx.near_protocol
    L = E.L_ORDER  # noqa: N806
    assert E.P == P
    rnd = random.Random(25519)

    def point(k):
        x, y, z = NP._mul(k % L, NP._G)[:3]
        zi = pow(z, P - 2, P)
        return x * zi % P, y * zi % P

    def draw():
        return rnd.randrange(1, L), rnd.randrange(1, L), rnd.randrange(1 << 512)

    def true_slot(a, r, d):
        return point(a) + point(r) + ((r + d * a) % L, d, 1)

    def limbs26(v):
        return sum(v << (26 * i) for i in range(10)) % (1 << 255) % P

    out = {"idle": E.inactive_slot(),
           # A.x = p - 2, not p - 1 (which is even): the largest ODD coordinate, so that the encoding of A carries the sign bit on top
           # of limb 15 = 0x7FFF; off_16bit_ones and off_order2 hold A.x = p - 1 and R.x = p - 1 is here
           "off_extremes": (P - 2, P - 1, P - 1, P - 1, L - 1, (1 << 512) - 1, 0),
           "off_zero_pt_hzero": (0, 0, 0, 0, L - 1, L * ((1 << 259) + 12345), 0),
           "off_26bit_half": (limbs26(1 << 25), limbs26((1 << 25) - 1), limbs26((1 << 26) - 1), P - 1, (1 << 252) - 1,
                              (1 << 512) - 1 - (1 << 256), 0),
           "off_16bit_ones": (P - 1, (1 << 254) - 1, 1 << 254, 2, int("55" * 32, 16) % L, int("aa" * 64, 16), 0),
           "off_order2": (0, P - 1, 0, P - 1, L - 1, (1 << 512) - 1, 0)}
    a, r, d = draw()
    out["s_zero"] = true_slot(a, -(d % L) * a, d)
    a, r, d = draw()
    out["h_zero"] = true_slot(a, r, L * rnd.randrange(1 << 250))
    a, r, d = draw()
    out["d_zero"] = true_slot(a, r, 0)
    a, r, d = draw()
    out["d_max"] = true_slot(a, r, (1 << 512) - 1)
    a, r, d = draw()
    out["s_lm1"] = true_slot(a, L - 1 - (d % L) * a, d)
    a, r, d = draw()
    out["r_identity"] = true_slot(a, 0, d)
    a, r, d = draw()
    out["a_identity"] = (0, 1) + point(r) + (r, d, 1)
    a, r, d = draw()
    out["a_order2"] = (0, P - 1) + point(r) + (r, d + (d % L) % 2, 1)    # [h](0, -1) is neutral for an even h = D mod L
    out["random0"], out["random1"] = E.synthetic_slots(2, seed=9)
    assert sorted(out) == sorted(ORDER)
    _cache["slots"] = out
    return out


def slot_list(nlx, names):
    s = slots(nlx)
    return [s[n] for n in names]


def reference(nlx, names):
    """The expected round-0 trace of the named slots, (N_COLS0, 256 len(names)) - ed25519_air.reference_trace over a per-slot
    cache of reference_slot (a slot is 256 rows of sixteen big-integer units: seconds for the sixteen, so once per session).
    The cache hands out COPIES: reference_trace writes row 0 (the previous slot's Y comparison) into the arrays it is given, and a
    slot that occurs twice in a list would otherwise share one array."""
    E = nlx.ed25519_air
    per_slot = _cache.setdefault("reference_slot", {})

    def cached(*sl):
        if sl not in per_slot:
            per_slot[sl] = E.reference_slot(*sl)
        t, q = per_slot[sl]
        return t.copy(), q
    key = ("reference", tuple(names))
    if key not in _cache:
        t = E.reference_trace(slot_list(nlx, names), slot_rows=cached)
        t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def reference_rows(nlx, name):
    """the 256 rows of one slot on its own (row 0's auxiliary unit is the neighbour's to fill: zero here); read-only"""
    reference(nlx, (name,))
    t = _cache["reference_slot"][slots(nlx)[name]][0]
    t.setflags(write=False)
    return t


def first_difference(nlx, got, want, names):
    """None, or where two traces first differ: column, row, the slot's name and the row within the slot"""
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    col, row = (int(v) for v in np.argwhere(got != want)[0])
    rows = nlx.ed25519_air.ROWS
    return "column %d row %d (slot %d = %s, row %d of the slot): %#x, expected %#x" % (
        col, row, row // rows, names[row // rows], row % rows, int(got[col, row]), int(want[col, row]))


def false_statements(nlx):
    """[(what, names, {index: slot}, reported)]: the sixteen-slot list with one or two slots replaced by a false statement made of
    random0's values; `reported` is the slot the generator must name (the smallest)."""
    E = nlx.ed25519_air
    ax, ay, rx, ry, s, d, _ = slots(nlx)["random0"]
    return [("a forged S in two active slots", {5: (ax, ay, rx, ry, s ^ 2, d, 1), 11: (ax, ay, rx, ry, s ^ 2, d, 1)}, 5),
            ("a wrong R.y alone in the last active slot: slot 0's row 0 reports it as its predecessor", {15: (ax, ay, rx, (ry + 1) % P, s, d, 1)}, 15),
            ("A.x = p in an inactive slot", {2: (P, ay, rx, ry, s, d, 0)}, 2),
            ("S = L in an inactive slot", {7: (ax, ay, rx, ry, E.L_ORDER, d, 0)}, 7)]


def with_replaced(nlx, replaced):
    out = slot_list(nlx, ORDER)
    for k, sl in replaced.items():
        out[k] = sl
    return out


# ---- operands for the direct check of fe25519_fast.hpp (host: tests/native/fe25519_fast_check.cpp; device: nlx_fe25519_ops) -----
B28 = (1 << 28) - 1                      # fe::mul's and freeze's input bound: |l_i| < 2^28
MUL_L0_MAX = (1 << 25) + 608             # carry10's result (fe25519_fast.hpp): |l_0| <= 2^25 + 608 ...
MUL_LI_MIN, MUL_LI_MAX = -(1 << 25), (1 << 25) - 1    # ... and -2^25 <= l_i <= 2^25 - 1 for i >= 1


def assert_mul_limbs_in_bound(limbs, what):
    """what quad::F10 and fe::mul's input contract rely on (fe25519_fast.hpp, carry10)"""
    assert abs(limbs[0]) <= MUL_L0_MAX and all(MUL_LI_MIN <= v <= MUL_LI_MAX for v in limbs[1:]), (what, limbs)


def value(limbs):
    """the integer ten signed 26-bit limbs stand for"""
    return sum(int(v) << (26 * i) for i, v in enumerate(limbs))


def freeze_operands():
    """values at the edges of p: k p + r for k in -3 .. 3, r in -20 .. 20, written (a) as a canonical-looking 26-bit split of
    |k p + r| with the sign on every limb and the excess in the top limb and (b) as k times p's own limbs (2^26 - 19, all ones,
    2^21 - 1) plus r in limb 0; 2^255 - 1; limbs all +-(2^28 - 1); the fixed points of the balanced carry at its rounding
    boundary (limbs of -2^25, with a small limb 0) and the values whose floor carries borrow through every limb; random signed limbs."""
    out = []
    p_limbs = [(1 << 26) - 19] + [(1 << 26) - 1] * 8 + [(1 << 21) - 1]
    for k in range(-3, 4):
        for r in range(-20, 21):
            v = k * P + r
            sign, mag = (-1 if v < 0 else 1), abs(v)
            out.append([sign * ((mag >> (26 * i)) & ((1 << 26) - 1)) for i in range(9)] + [sign * (mag >> 234)])
            out.append([k * p_limbs[0] + r] + [k * x for x in p_limbs[1:]])
    out.append([(1 << 26) - 1] * 9 + [(1 << 21) - 1])
    for sign in ((1,) * 10, (-1,) * 10, (1, -1) * 5, (-1, 1) * 5):
        out.append([sg * B28 for sg in sign])
    for l0 in (0, 1, 5, 303, 304, 305, 607, 608, 609, -1, -608, -609):
        out.append([l0] + [0] * 8 + [-(1 << 25)])
        out.append([l0] + [-(1 << 25)] * 9)
        out.append([l0] + [(1 << 25) - 1] * 9)
        out.append([l0] + [0] * 8 + [(1 << 25) - 1])
        out.append([l0 - (1 << 25)] + [0] * 8 + [-(1 << 25)])
    for k in (1, 12, 16):     # -k 2^255 + d, d around 19 k: where a floor carry's borrow runs through every limb into the top one
        for d in (0, 19 * k - 1, 19 * k):
            out.append([d] + [0] * 8 + [-k << 21])
    rnd = random.Random(255)
    for _ in range(599):     # with the pairs of mul_operands the device's list then ends in a partial quad
        out.append([rnd.randrange(-B28, B28 + 1) for _ in range(10)])
    for v in out:
        assert len(v) == 10 and max(abs(x) for x in v) <= B28
    return out


def mul_operands():
    """pairs at the input bound (all +, all -, each sign pattern against each, random signs) and random pairs"""
    rnd = random.Random(608)
    pats = [[sg * B28 for sg in s] for s in ((1,) * 10, (-1,) * 10, (1, -1) * 5, (-1, 1) * 5)]
    out = [(a, b) for a in pats for b in pats]
    for _ in range(200):
        out.append(([rnd.choice((-B28, B28)) for _ in range(10)], [rnd.choice((-B28, B28)) for _ in range(10)]))
    for _ in range(100):   # sums of four carried values at carry10's own bound, as the scan feeds them
        out.append(([rnd.choice((-4, 4)) * (1 << 25) for _ in range(10)], [rnd.choice((-4, 4)) * ((1 << 25) - 1) for _ in range(10)]))
    for _ in range(600):
        out.append(([rnd.randrange(-B28, B28 + 1) for _ in range(10)], [rnd.randrange(-B28, B28 + 1) for _ in range(10)]))
    return out


def device_operands():
    """the (a, b) pairs nlx_fe25519_ops is run on: every freeze operand as a (against a cycling b) and every mul pair"""
    fz, ml = freeze_operands(), mul_operands()
    return [(a, ml[i % len(ml)][1]) for i, a in enumerate(fz)] + ml


def from_limbs16_operands():
    rnd = random.Random(16)
    return [(1 << 256) - 1, 0, 1, (1 << 255) - 19, int("5a" * 32, 16)] + [rnd.randrange(1 << 256) for _ in range(200)]


def sum_operands():
    """quadruples of carried values at carry10's bound for add / sub / dbl / neg: the four-term sums the scan forms"""
    rnd = random.Random(4)
    edge = [[MUL_L0_MAX] + [MUL_LI_MAX] * 9, [-MUL_L0_MAX] + [MUL_LI_MIN] * 9]
    out = [[edge[(m >> k) & 1] for k in range(4)] for m in range(16)]
    for _ in range(100):
        out.append([[rnd.randrange(-MUL_L0_MAX, MUL_L0_MAX + 1)] + [rnd.randrange(MUL_LI_MIN, MUL_LI_MAX + 1) for _ in range(9)] for _ in range(4)])
    return out
