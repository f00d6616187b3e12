"""The SOLVABLE constraint systems of the PLONK witness-solver tests (nlx_bn254_plonk_solver_*): one
definition, shared by the CPU file (the model tools/gnark_plonk_solve_model.py against the frozen models) and the GPU file (the
device against the model).  A plain module, not a conftest.  The tables are bn254_plonk_setup_cases.Circuit's; the builder here
adds constraints that ASSIGN: it picks the form, draws the coefficients and leaves the value to the solver - no value is ever
computed here, a check-only constraint is an earlier constraint scaled by a random factor.

The shapes are the smallest at which each part can go wrong:
  forms8     2^3: one constraint of each form - O with qo = -1, O with a random qo, L with qm = 0, L with qm != 0 (a
             value-dependent divisor), R likewise, one check-only
  chain300   2^9: depth 300, width 1: one fused run
  ragged     2^14: level widths 1, 63, 64, 65, FUSE - 1, FUSE, FUSE + 1, 5000, 1, 1, 70: fused run, two wide launches, fused run;
             the widths cross the wave, the block and several blocks.  Its failing inputs: FAILING
  hints      2^13: N_BITS with nb = 1, 64, 254, 256 on 0, 1, 2^64 - 1, r - 1; QUO_REM64 with m = 1, 2^64 - 1 and the Goldilocks
             prime on 0, m - 1, m, 2^128 + 5, r - 1; INV_ZERO on 0, 1, r - 1; constraints recombine the outputs, so that a
             wrong bit breaks a check
  k2chain    2^5: two commitments, the second committing c_0, the second's own constraint last (n32_k2's shape, solvable)
  k1_1000    2^10, k = 1; plain4096: 2^12, k = 0: the end-to-end sizes
The refusals of the schedule: REFUSALS."""
import functools
import os
import random
import sys

import bn254_plonk_setup_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gnark_plonk_solve_model as pm  # noqa: E402

R, bn = sc.R, sc.bn
ZERO, ONE, MINUS_ONE = sc.ZERO, sc.ONE, sc.MINUS_ONE
FUSE = 1024                      # NLX_BN254_PLONK_SOLVER_FUSE (the GPU file holds the two together)
GOLDILOCKS = (1 << 64) - (1 << 32) + 1
RAGGED_WIDTHS = (1, 63, 64, 65, FUSE - 1, FUSE, FUSE + 1, 5000, 1, 1, 70)


class Solvable(sc.Circuit):
    """a Circuit whose .variables hold the INPUTS (n_public + n_secret of them) and a 0 for every variable the solver is to
    find; .hints in the Python API's shape; .level_of[v] as the builder means it (checked against the model's levels)"""

    def __init__(self, name, log_n, n_public, n_secret, seed):
        super().__init__(name, log_n, n_public, 39000 + seed)
        while len(self.variables) < n_public + n_secret:
            self.var()
        self.n_secret = len(self.variables) - n_public
        self.hints = []

    @property
    def inputs(self):
        return list(self.variables[:self.n_public + self.n_secret])

    def coeff(self, value=None):
        self.coeffs.append(self.rng.randrange(1, R) if value is None else value % R)
        return len(self.coeffs) - 1

    def unknown(self):
        return self.var(0)

    def add(self, a, b, c, ql, qr, qm, qo, qk):
        self.constraints.append((a, b, c, ql, qr, qm, qo, qk))
        return len(self.constraints) - 1

    def pick(self):
        return self.rng.choice(self.pool)

    # -- constraints that assign --
    def solve_o(self, a, b, qo=None):
        """o from l = a, r = b; qo = -1 unless given"""
        v = self.unknown()
        self.add(a, b, v, self.pick(), self.pick(), self.pick(), MINUS_ONE if qo is None else qo, self.pick())
        return v

    def solve_l(self, b, c, qm=ZERO):
        """l from r = b, o = c; qm = 0: a constant divisor, else ql + qm r"""
        v = self.unknown()
        self.add(v, b, c, self.pick(), self.pick(), qm, self.pick(), self.pick())
        return v

    def solve_r(self, a, c, qm=ZERO):
        v = self.unknown()
        self.add(a, v, c, self.pick(), self.pick(), qm, self.pick(), self.pick())
        return v

    def any_solve(self, a, b):
        """a random form on the operands a, b"""
        t = self.rng.random()
        if t < 0.5:
            return self.solve_o(a, b)
        if t < 0.65:
            return self.solve_o(a, b, self.pick())
        if t < 0.8:
            return self.solve_l(a, b)
        if t < 0.9:
            return self.solve_l(a, b, self.pick())
        return self.solve_r(a, b, self.pick())

    def scaled_check(self, c):
        """constraint c again, every coefficient times one random factor: satisfied exactly when c is"""
        con, f = self.constraints[c], self.rng.randrange(2, R)
        return self.add(con[0], con[1], con[2], *[self.coeff(self.coeffs[i] * f) if self.coeffs[i] else ZERO for i in con[3:8]])

    def solver_model(self):
        return pm.Solver(self.n_variables, self.n_public, self.n_secret, self.constraints, self.coeffs, self.sets, self.hints)

    def solver_args(self):
        return dict(n_secret=self.n_secret, hints=self.hints)


def _forms8():
    c = Solvable("forms8", 3, 1, 2, 8)
    a, b, p = 1, 2, 0
    v0 = c.solve_o(a, b)
    v1 = c.solve_o(v0, p, c.pick())
    v2 = c.solve_l(a, v1)
    v3 = c.solve_l(v2, v0, c.pick())
    c.solve_r(v3, b, c.pick())
    c.scaled_check(3)
    assert c.n_public + len(c.constraints) == 7
    return c


def _chain300():
    c = Solvable("chain300", 9, 2, 2, 300)
    v = 2
    for i in range(300):
        v = c.any_solve(v, c.rng.randrange(4))
    return c


def _ragged():
    """Inputs: 0, 1 public; a = 2 seeds the spine s_lv = a + lv (the first constraint of every level); b = 3 is the R operand of
    the level-2 divisor appended at the END of the circuit; chk = 4 must equal s_1; 5 .. 9 random.  c.special names the aimed
    constraints."""
    c = Solvable("ragged", 14, 2, 8, 14)
    a, b, chk = 2, 3, 4
    c.variables[chk] = (c.variables[a] + 1) % R
    previous, older = [], list(range(10))
    c.special = {}
    qm7, qm2 = c.coeff(), c.coeff()
    for lv, width in enumerate(RAGGED_WIDTHS, start=1):
        spine = c.unknown()
        c.add(previous[0] if previous else a, 0, spine, ONE, ZERO, ZERO, MINUS_ONE, ONE)      # s_lv = s_(lv-1) + 1
        now, count = [spine], 1
        count += {2: 2, 3: 1}.get(lv, 0)     # level 2: the check here and the divisor at the end; level 3: the check at the end
        if lv == 7:
            # l = -(qr r + qo o + qk) / (ql + qm7 s_6): FAILING picks a' so that a' + 6 makes the divisor 0; nothing reads l
            c.special["div7"] = c.add(c.unknown(), previous[0], c.rng.choice(older), c.coeff(), c.pick(), qm7, c.pick(), c.pick())
            count += 1
        while count < width:
            now.append(c.any_solve(c.rng.choice(previous), c.rng.choice(older)))
            count += 1
        if lv == 2:
            c.special["check"] = c.add(chk, 0, previous[0], ONE, ZERO, ZERO, MINUS_ONE, ZERO)       # chk - s_1 == 0
        older += previous
        previous = now
    c.spine1 = c.constraints[0][2]
    # level 2, the highest indices: l = .. / (ql + qm2 b), o = s_1 makes it level 2; then its scaled copy: a check at level 3
    v = c.unknown()
    c.special["div2"] = c.add(v, b, c.spine1, c.coeff(), c.pick(), qm2, c.pick(), c.pick())
    c.special["downstream"] = c.scaled_check(c.special["div2"])
    return c


def failing(c):
    """ragged's failing inputs: name -> (inputs, the failure the model must stop at as (kind, constraint), failures, poisoned)"""
    a, b, chk = 2, 3, 4
    q7, q2 = c.constraints[c.special["div7"]], c.constraints[c.special["div2"]]
    inv = lambda x: pow(x, R - 2, R)
    a_bad = (-c.coeffs[q7[3]] * inv(c.coeffs[q7[5]]) - 6) % R          # ql + qm (a + 6) == 0
    b_bad = (-c.coeffs[q2[3]] * inv(c.coeffs[q2[5]])) % R              # ql + qm b == 0
    out = {}
    x = c.inputs
    x[a], x[chk], x[b] = a_bad, (a_bad + 1) % R, b_bad
    out["two_divisors"] = (x, (pm.DIV_ZERO, c.special["div7"]), 2, 2)      # the lower index, although its level is the higher
    x = c.inputs
    x[chk] = (x[chk] + 1) % R
    out["unsatisfied"] = (x, (pm.UNSATISFIED, c.special["check"]), 1, 0)
    x = c.inputs
    x[b] = b_bad
    out["poisoned_check"] = (x, (pm.DIV_ZERO, c.special["div2"]), 1, 1)    # its scaled copy downstream: not reported, not counted
    return out


def _hints():
    r"""Inputs: variable 0 pads (public), then one secret per hint input."""
    nbits_on = [0, 1, (1 << 64) - 1, R - 1]
    quo = [(m, x) for m in (1, (1 << 64) - 1, GOLDILOCKS) for x in (0, m - 1, m, (1 << 128) + 5, R - 1)]
    inv_on = [0, 1, R - 1]
    values = [x for x in nbits_on for _ in (1, 64, 254, 256)] + [x for _, x in quo] + inv_on
    c = Solvable("hints", 13, 1, len(values), 13)
    for i, x in enumerate(values):
        c.variables[1 + i] = x % R
    two = [c.coeff(1 << i) for i in range(256)]
    at = 1
    for x in nbits_on:
        for nb in (1, 64, 254, 256):
            bits = [c.unknown() for _ in range(nb)]
            c.hints.append(("n_bits", len(c.constraints), at, bits))
            acc = None
            for i, bit in enumerate(bits):
                c.add(bit, bit, 0, MINUS_ONE, ZERO, ONE, ZERO, ZERO)                    # b b - b == 0
                nxt = c.unknown()
                if acc is None:
                    c.add(bit, 0, nxt, two[0], ZERO, ZERO, MINUS_ONE, ZERO)             # acc = b_0
                else:
                    c.add(acc, bit, nxt, ONE, two[i], ZERO, MINUS_ONE, ZERO)            # acc' = acc + 2^i b_i
                acc = nxt
            if x < 1 << nb:
                c.add(acc, at, 0, ONE, MINUS_ONE, ZERO, ZERO, ZERO)                     # the bits are x
            else:
                c.add(acc, 0, 0, ONE, ZERO, ZERO, ZERO, c.coeff(-(x % (1 << nb))))      # .. are its low nb bits
            at += 1
    for m, x in quo:
        q, rem = c.unknown(), c.unknown()
        c.hints.append(("quo_rem64", len(c.constraints), at, m, q, rem))
        c.add(q, rem, at, c.coeff(m), ONE, ZERO, MINUS_ONE, ZERO)                       # q m + rem - x == 0
        c.solve_o(q, rem)                                                                # and both feed a solve
        at += 1
    for x in inv_on:
        y = c.unknown()
        c.hints.append(("inv_zero", len(c.constraints), at, y))
        if x:
            c.add(at, y, 0, ZERO, ZERO, ONE, ZERO, MINUS_ONE)                            # x y == 1
        else:
            c.add(y, 0, 0, ONE, ZERO, ZERO, ZERO, ZERO)                                  # y == 0
        at += 1
    assert at == c.n_public + c.n_secret and c.n_public + len(c.constraints) <= c.n
    return c


def _k2chain():
    c = Solvable("k2chain", 5, 2, 3, 32)
    free = [c.any_solve(c.rng.randrange(5), c.rng.randrange(5)) for _ in range(6)]
    j0 = c.commitment([free[2], free[4]])
    c.close_commitment(j0)
    w = c.solve_o(c.c_var[0], free[0])                  # depends on c_0
    j1 = c.commitment([c.c_var[0], w, free[3]])         # depth: commitment 1 covers c_0
    c.any_solve(w, free[1])
    c.scaled_check(len(c.constraints) - 1)
    c.close_commitment(j1)                              # the last constraint: commit row = last_row
    assert c.n_public + len(c.constraints) <= 32
    return c


def _random_dag(c, count, known):
    for _ in range(count):
        known.append(c.any_solve(c.rng.choice(known), c.rng.choice(known)))
        if c.rng.random() < 0.1:
            c.scaled_check(len(c.constraints) - 1)


def _k1_1000():
    c = Solvable("k1_1000", 10, 3, 5, 1000)
    known = list(range(8))
    _random_dag(c, 400, known)
    j = c.commitment([known[20], known[50], known[20], known[300]])
    c.close_commitment(j)
    known.append(c.c_var[0])
    while c.n_public + len(c.constraints) < 998:
        _random_dag(c, 1, known)
    assert c.n_public + len(c.constraints) <= 1000
    return c


def _plain4096():
    c = Solvable("plain4096", 12, 3, 13, 4096)
    known = list(range(16))
    while c.n_public + len(c.constraints) < 4090:
        _random_dag(c, 1, known)
    return c


_BUILDERS = {"forms8": _forms8, "chain300": _chain300, "ragged": _ragged, "hints": _hints, "k2chain": _k2chain, "k1_1000": _k1_1000,
             "plain4096": _plain4096}
ALL = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    return case(name).solver_model()


def commit_blinding(name):
    rng = random.Random("blind" + name)
    return [rng.randrange(R) for _ in range(2 * case(name).k)]


def trapdoor(name):
    return random.Random("tau" + name).randrange(1, R)


@functools.lru_cache(maxsize=None)
def solved(name):
    """the model's vector on the case's own inputs (the commitments through the trapdoor): (values, [PI2_j], [c_j]); solved
    once, shared, never changed"""
    c, m = case(name), model(name)
    commit, points = pm.bsb22_committer(c.model(), None, commit_blinding(name), trapdoor(name))
    values, failure = m.solve(c.inputs, commit)
    assert failure is None, failure
    return tuple(values), tuple(points), tuple(values[v] for v in c.c_var)


def launches(m, fuse=True):
    """(launches, fused runs) of one solve as the level widths predict: a commitment's hint breaks a run in front of its level;
    a run of one level is a plain launch; a level of commitments alone launches nothing"""
    width, commits = {}, {}
    for c, lv in enumerate(m.level):
        if m.form[c] != pm.SKIPPED:
            width[lv] = width.get(lv, 0) + 1
    for h, lv in enumerate(m.hint_level):
        width[lv] = width.get(lv, 0) + 1
        if m.hints[h][0] == pm.COMMIT:
            commits[lv] = commits.get(lv, 0) + 1
    levels = max(width) if width else 0
    n_launch = runs = 0
    lv = 1
    while lv <= levels:
        n = 1
        if fuse and width[lv] <= FUSE:
            while lv + n <= levels and width[lv + n] <= FUSE and not commits.get(lv + n):
                n += 1
        if n > 1:
            n_launch, runs = n_launch + 1, runs + 1
        elif width[lv] > commits.get(lv, 0):
            n_launch += 1
        lv += n
    return n_launch, runs


def refusals():
    """(what, constraints, hints, ("constraint" | "hint", index)) over REFUSAL_VARIABLES variables, n_public = n_secret = 1:
    variables 0 and 1 are given"""
    P = [3, 4, 5, 6, 7]      # coefficient ids of five nonzero values
    ok = (0, 1, 2) + (P[0], P[1], ZERO, MINUS_ONE, P[4])                 # solves variable 2
    return [
        ("two unassigned variables", [ok, (2, 3, 4, P[0], P[1], ZERO, P[3], ZERO)], [], ("constraint", 1)),
        ("quadratic", [ok, (3, 3, 1, P[0], ZERO, P[2], P[3], ZERO)], [], ("constraint", 1)),
        ("quadratic through qm alone", [ok, (3, 3, 1, ZERO, ZERO, P[2], P[3], ZERO)], [], ("constraint", 1)),
        ("hint input not assigned", [ok, (2, 3, 4, P[0], P[1], ZERO, MINUS_ONE, ZERO)], [("inv_zero", 1, 3, 5)], ("hint", 0)),
        ("hint output given", [ok], [("inv_zero", 0, 0, 1)], ("hint", 0)),
        ("hint output assigned twice", [ok], [("inv_zero", 0, 0, 3), ("n_bits", 1, 1, [4, 3])], ("hint", 1)),
        ("hint output assigned by a constraint", [ok], [("inv_zero", 1, 0, 2)], ("hint", 0)),
        ("before descends", [ok, ok[:2] + (3,) + ok[3:]], [("inv_zero", 1, 0, 4), ("inv_zero", 0, 1, 5)], ("hint", 1)),
        ("before beyond the constraints", [ok], [("inv_zero", 2, 0, 4)], ("hint", 0)),
    ]


REFUSAL_COEFFS = [0, 1, R - 1, 11, 12, 13, 14, 15]
REFUSAL_VARIABLES = 6
