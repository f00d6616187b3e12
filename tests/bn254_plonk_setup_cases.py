"""The constraint systems of the PLONK setup tests (nlx_bn254_plonk_setup): one definition, shared by the
CPU file (the model against its own invariants and the frozen provers) and the GPU file (the device against the model).  A plain
module, not a conftest.  Every circuit is a gnark-shaped SparseR1CS: per constraint three variable ids and five coefficient ids.

The shapes are the smallest at which each kernel can go wrong:
  n8, n8_nopub  2^3, N = 8 exactly: no padding, class 0 is short (with and without public rows)
  n5            2^3, N = 5: padding
  n32_k2        2^5: a variable in all three cells of one row, a variable used once, k = 2 with the last constraint as a
                commitment row (commit row = last_row)
  n256          2^8: one variable in 300 cells and variable 0 in about 500: classes cross 256-lane blocks and waves
  n1000_k1      2^10: N = 1000, n_public = 3, k = 1, random reuse
  n1024, n4096  2^10, 2^12, k = 0: the end-to-end sizes
  s14           2^14 structured (constraint c uses variables c, c + 1, 7 c mod V): rows above the root tables' split (2^7)
  s16           2^16 structured with more than 2^16 variables: the sort takes more than one digit pass
The small ones are satisfied by .variables (c_j through .complete); s14 and s16 test structure only and carry no witness."""
import functools
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_plonk_setup_model as sm  # noqa: E402

bn, R = sm.bn, sm.R
ZERO, ONE, MINUS_ONE = 0, 1, 2      # ids of 0, 1, -1 in every coefficient table


class Circuit:
    """n_variables, n_public, constraints [(xa, xb, xc, ql, qr, qm, qo, qk)], coeffs (integers), sets (the commitments),
    variables (a satisfying vector with the c_j at 0, or None), c_var"""

    def __init__(self, name, log_n, n_public, seed):
        self.name, self.log_n, self.n_public = name, log_n, n_public
        self.n, self.k1, self.k2 = 1 << log_n, 5, 25
        self.rng = random.Random(37000 + seed)
        self.variables = [self.rng.randrange(R) for _ in range(max(1, n_public))]
        self.constraints, self.coeffs, self.sets, self.c_var = [], [0, 1, R - 1], [], []
        self.pool = []
        for _ in range(12):
            self.coeffs.append(self.rng.randrange(R))
            self.pool.append(len(self.coeffs) - 1)

    # -- building --
    def var(self, value=None):
        self.variables.append(self.rng.randrange(R) if value is None else value)
        return len(self.variables) - 1

    def gate(self, a, b, c):
        """a satisfied constraint on the three variables: four selectors from the pool, qk fitted"""
        ids = [self.rng.choice(self.pool) for _ in range(4)]
        ql, qr, qm, qo = (self.coeffs[i] for i in ids)
        va, vb, vc = self.variables[a], self.variables[b], self.variables[c]
        self.coeffs.append(-(ql * va + qr * vb + qm * va * vb + qo * vc) % R)
        self.constraints.append((a, b, c, ids[0], ids[1], ids[2], ids[3], len(self.coeffs) - 1))
        return len(self.constraints) - 1

    def minus_l(self, x):
        """ql = -1, the rest 0: a committed constraint or a commitment's own"""
        self.constraints.append((x, 0, 0, MINUS_ONE, ZERO, ZERO, ZERO, ZERO))
        return len(self.constraints) - 1

    def commitment(self, committed_vars):
        """one Bsb22 commitment: committed constraints on these variables (ascending as they are added); the commitment's own
        constraint is added by close_commitment, so that it can come last"""
        self.sets.append({"committed": [self.minus_l(x) for x in committed_vars], "constraint": None})
        return len(self.sets) - 1

    def close_commitment(self, j):
        self.c_var.append(self.var(0))
        self.sets[j]["constraint"] = self.minus_l(self.c_var[-1])

    # -- reading --
    @property
    def n_variables(self):
        return len(self.variables) if self.variables is not None else self.n_declared

    @property
    def k(self):
        return len(self.sets)

    @property
    def public_inputs(self):
        return list(self.variables[:self.n_public])

    def complete(self, cs=()):
        """the variable vector once c_0 .. c_{len(cs) - 1} are known"""
        v = list(self.variables)
        for j, c in enumerate(cs):
            v[self.c_var[j]] = int(c) % R
        return v

    @functools.lru_cache(maxsize=None)
    def model(self):
        return sm.Setup(self.n_variables, self.n_public, self.constraints, self.coeffs, self.k1, self.k2, self.sets, self.log_n)

    def args(self):
        """what nlx.bn254_plonk.Setup takes after the context"""
        return dict(n_variables=self.n_variables, n_public=self.n_public, constraints=self.constraints, coeffs=self.coeffs, k1=self.k1,
                    k2=self.k2, commitments=self.sets, log_n=self.log_n)


def _random_gates(c, count, n_free, zero_share=0.0):
    free = [c.var() for _ in range(n_free)]
    pick = lambda: 0 if c.rng.random() < zero_share else c.rng.choice(free)
    for _ in range(count):
        c.gate(pick(), pick(), pick())
    return free


def _n8(n_public):
    c = Circuit("n8" if n_public else "n8_nopub", 3, n_public, 1 + n_public)
    _random_gates(c, 8 - n_public, 4)
    return c


def _n5():
    c = Circuit("n5", 3, 1, 5)
    _random_gates(c, 4, 3)
    return c


def _n32_k2():
    c = Circuit("n32_k2", 5, 2, 32)
    free = _random_gates(c, 14, 6)
    triple, once = c.var(), c.var()
    c.gate(triple, triple, triple)
    c.gate(free[0], once, free[1])
    j0 = c.commitment([free[2], free[4]])
    c.close_commitment(j0)
    j1 = c.commitment([c.c_var[0], free[3], triple])      # depth: commitment 1 covers c_0
    _random_gates(c, 3, 2)
    c.close_commitment(j1)                                # the last constraint: commit row = last_row
    assert c.n_public + len(c.constraints) == 28
    return c


def _n256():
    c = Circuit("n256", 8, 1, 256)
    hot = c.var()
    free = [c.var() for _ in range(5)]
    slots = [hot] * 300 + [0] * 440 + [c.rng.choice(free) for _ in range(10)]      # variable 0: these, 15 padding cells, the public row
    c.rng.shuffle(slots)
    for i in range(250):
        c.gate(*slots[3 * i:3 * i + 3])
    return c


def _n1000_k1():
    c = Circuit("n1000_k1", 10, 3, 1000)
    free = _random_gates(c, 600, 200, zero_share=0.1)
    j = c.commitment([free[5], free[17], free[5], free[100]])
    c.close_commitment(j)
    for _ in range(997 - len(c.constraints)):
        c.gate(c.rng.choice(free), c.rng.choice(free), c.rng.choice(free))
    assert c.n_public + len(c.constraints) == 1000
    return c


def _plain(log_n, n_public, seed):
    c = Circuit("n%d" % (1 << log_n), log_n, n_public, seed)
    n = 1 << log_n
    _random_gates(c, n - n_public - 5, n // 3, zero_share=0.05)
    return c


def structured(log_n, n_constraints, n_variables, n_public=2, name=None):
    """constraint c uses variables c, c + 1, (7 c) mod V and coefficients from a pool of eight: structure only, no witness"""
    c = Circuit(name or "s%d" % log_n, log_n, n_public, log_n)
    c.variables, c.n_declared = None, n_variables
    c.constraints = [(i, i + 1, 7 * i % n_variables, 3 + i % 8, 3 + (i >> 3) % 8, ZERO, 3 + (i >> 6) % 8, ONE) for i in range(n_constraints)]
    return c


_BUILDERS = {
    "n8": lambda: _n8(2), "n8_nopub": lambda: _n8(0), "n5": _n5, "n32_k2": _n32_k2, "n256": _n256, "n1000_k1": _n1000_k1,
    "n1024": lambda: _plain(10, 2, 1024), "n4096": lambda: _plain(12, 3, 4096),
    "s14": lambda: structured(14, 16000, 16001), "s16": lambda: structured(16, 65520, 70000),
}
SMALL = ("n8", "n8_nopub", "n5", "n32_k2", "n256", "n1000_k1")      # every array against the model's
ALL = SMALL + ("n1024", "n4096", "s14", "s16")


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def worked_case():
    """rule 3's worked case: n_public = 1, constraints (1, 2, 3) and (3, 1, 0), log_n = 3"""
    return sm.Setup(4, 1, [(1, 2, 3, ZERO, ZERO, ZERO, ZERO, ZERO), (3, 1, 0, ZERO, ZERO, ZERO, ZERO, ZERO)], [0, 1, R - 1], log_n=3)


WORKED_PERM = {1: 10, 10: 1, 9: 9, 2: 17, 17: 2, 0: 23, 3: 0, 4: 3, 8: 7, 11: 8, 16: 15, 18: 16, 23: 22}


def one_cell_changed(c):
    """the same circuit with one cell of one constraint pointing at another variable (a foreign key for the verifier): the
    constraints and the index of the edited one"""
    cons = list(c.constraints)
    at = next(i for i, con in enumerate(cons) if con[3] != MINUS_ONE and con[1] != con[2])
    con = cons[at]
    cons[at] = (con[0], con[2], con[1]) + tuple(con[3:])
    return cons, at


class AsInstance:
    """a circuit and its model in the shape tools/gnark_bsb22_model.py's prove / verifying_key take an Instance in"""

    def __init__(self, c):
        m = c.model()
        self.c, self.m = c, m
        self.n, self.log_n, self.k, self.k1, self.k2 = m.n, m.log_n, c.k, c.k1, c.k2
        self.public_inputs = c.public_inputs
        self.fixed = {name: m.values[name] for name in ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")}
        self.qcp = m.qcp
        self.commit_rows = [i["row"] for i in m.info]
        self.committed = [i["committed"] for i in m.info]
        self.last_row = m.used - 1

    def complete(self, cs):
        return self.m.wires(self.c.complete(cs))
