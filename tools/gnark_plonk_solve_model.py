#!/usr/bin/env python3
"""gnark's witness solver for a PLONK SparseR1CS over BN254 on big integers, sequential: from the public and secret inputs to the
whole variable vector, constraint by constraint, with the four hint kinds the project knows.  The yardstick of
nlx_bn254_plonk_solver_* (csrc/bn254_plonk_solve.hpp and .hip); it shares no code with the device side.
The field comes from the frozen oracle/bn254_py.py, the commitment hint's value from tools/gnark_bsb22_model.py rule 3.

Status of every rule: RECALLED from gnark v0.9 (constraint/bn254/solver.go, solveSparseR1C, the blueprints' levels), UNPINNED -
there is no Go source and no gnark-solved witness to compare with; parity with gnark's solver is not claimed.  Each rule is
written once, here.

  rule 1  given         variables [0, n_public + n_secret) are given                                          (Solver.solve)
  rule 2  counting      a cell counts only where its coefficient can determine it: L when ql != 0 or qm != 0, R when
                        qr != 0 or qm != 0, O when qo != 0; other cells (placeholders on variable 0) are ignored  (counting)
  rule 3  skipped       the committed constraints of every commitment set and each commitment's own constraint are
                        skipped, as gnark skips COMMITTED / COMMITMENT rows                                   (Solver.__init__)
  rule 4  a constraint  walked in index order.  No unassigned counting variable: check-only,
                        ql l + qr r + qm l r + qo o + qk == 0.  Exactly one, in exactly one counting cell: it is solved -
                        L: l = -(qr r + qo o + qk) / (ql + qm r), R symmetric, O: o = -(ql l + qr r + qm l r + qk) / qo
                                                                                                              (solve_item)
  rule 5  hints         each carries `before`, the constraint in front of which it runs; `before` does not descend over the
                        list (gnark's instruction order).  INV_ZERO: x^-1, or 0 for 0.  N_BITS: nb in 1 .. 256 outputs,
                        output i = bit i of the canonical integer.  QUO_REM64: a parameter 1 <= m < 2^64, outputs q, r with
                        canonical(x) = q m + r, 0 <= r < m.  COMMIT j: implied by commitment j, before = j's own constraint
                        (after the listed hints of the same `before`); inputs = the L variables of set j's committed
                        constraints, output = the L variable of its own constraint, value = c_j               (run_hint)
  rule 6  refusals      when the schedule is made, the message naming the constraint or hint: two unassigned counting
                        variables in one constraint; the unassigned variable in two counting cells (quadratic); a hint input
                        not assigned by `before`; a hint output that is given or assigned twice; `before` descending or
                        > n_constraints                                                                       (ScheduleError)
  rule 7  unassigned    a variable that no counting cell, hint or input assigns stays 0 and is counted        (unassigned)
  rule 8  failures      DIV_ZERO: the divisor of a solving constraint is 0, WHATEVER the numerator - our rule, possibly a
                        deviation from gnark (which may accept 0 / 0); UNSATISFIED: a check-only constraint is nonzero.  The
                        solver stops at the first failure in index order: (kind, constraint, value), value = the numerator
                        or the constraint's value, canonical                                                  (Solver.solve)
  rule 9  levels        an item's level is 1 + the highest level among the assigners of its (counting) operands; inputs are
                        level 0                                                                               (levels)
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
sys.path.insert(0, _HERE)
import bn254_py as bn  # noqa: E402

R = bn.R
CHECK, SOLVE_L, SOLVE_R, SOLVE_O, INV_ZERO, N_BITS, QUO_REM64, COMMIT, SKIPPED = range(9)
HINT_KINDS = {"inv_zero": INV_ZERO, "n_bits": N_BITS, "quo_rem64": QUO_REM64}
OK, DIV_ZERO, UNSATISFIED = 0, 1, 2
NONE = 0xFFFFFFFF
POISON = object()


class ScheduleError(ValueError):
    """rule 6; .where = ("constraint" | "hint", index)"""

    def __init__(self, kind, index, text):
        super().__init__("%s %d: %s" % (kind, index, text))
        self.where = (kind, index)


def counting(q):
    """rule 2 -> (L counts, R counts, O counts) from the five coefficient values"""
    ql, qr, qm, qo, _ = q
    return (ql != 0 or qm != 0, qr != 0 or qm != 0, qo != 0)


def solve_item(form, q, l, r, o):
    """rule 4 -> (kind, the solved value or None, the numerator or the constraint's value)"""
    ql, qr, qm, qo, qk = q
    if form == CHECK:
        v = (ql * l + qr * r + qm * l * r + qo * o + qk) % R
        return (UNSATISFIED if v else OK), None, v
    if form == SOLVE_O:
        num, div = (ql * l + qr * r + qm * l * r + qk) % R, qo
    elif form == SOLVE_L:
        num, div = (qr * r + qo * o + qk) % R, (ql + qm * r) % R
    else:
        num, div = (ql * l + qo * o + qk) % R, (qr + qm * l) % R
    if div == 0:
        return DIV_ZERO, None, num
    return OK, (-num) * pow(div, R - 2, R) % R, num


def run_hint(kind, x, param):
    """rule 5, the arithmetic kinds -> the outputs"""
    x %= R
    if kind == INV_ZERO:
        return [pow(x, R - 2, R) if x else 0]
    if kind == N_BITS:
        return [(x >> i) & 1 for i in range(param)]
    return [x // param, x % param]


class Solver:
    """constraints: (xa, xb, xc, ql, qr, qm, qo, qk) - three variable ids, five ids into coeffs; sets: the commitments
    ({"committed": ascending constraint indices, "constraint": its own}); hints: ("inv_zero", before, x, y),
    ("n_bits", before, x, outs), ("quo_rem64", before, x, m, q, r).  Making it IS making the schedule: rule 6 raises here."""

    def __init__(self, n_variables, n_public, n_secret, constraints, coeffs, sets=(), hints=()):
        self.n_variables, self.n_given, self.constraints = n_variables, n_public + n_secret, list(constraints)
        self.q = [tuple(int(coeffs[i]) % R for i in con[3:8]) for con in self.constraints]
        self.sets = [{"committed": list(s["committed"]), "constraint": int(s["constraint"])} for s in sets]
        nc = len(self.constraints)
        if self.n_given > n_variables:
            raise ValueError("more inputs than variables")
        skipped = set()
        for s in self.sets:
            skipped.update(s["committed"])
            skipped.add(s["constraint"])
        # the hints as (kind, before, inputs, outputs, param), the commitments' among them, in running order
        self.hints, last = [], 0
        for h, t in enumerate(hints):
            kind, before, x = HINT_KINDS[t[0]], int(t[1]), int(t[2])
            if before < last or before > nc:
                raise ScheduleError("hint", h, "before = %d descends or exceeds the %d constraints" % (before, nc))
            last = before
            if kind == INV_ZERO:
                outs, param = [int(t[3])], 0
            elif kind == N_BITS:
                outs, param = [int(v) for v in t[3]], len(t[3])
                if not 1 <= param <= 256:
                    raise ScheduleError("hint", h, "N_BITS takes 1 .. 256 outputs")
            else:
                outs, param = [int(t[4]), int(t[5])], int(t[3])
                if not 1 <= param < 1 << 64:
                    raise ScheduleError("hint", h, "QUO_REM64 takes 1 <= m < 2^64")
            self.hints.append((kind, before, [x], outs, param))
        self.n_listed = len(self.hints)
        for j, s in enumerate(self.sets):
            self.hints.append((COMMIT, s["constraint"], [self.constraints[c][0] for c in s["committed"]], [self.constraints[s["constraint"]][0]], j))
        by_before = {}
        for h, hint in enumerate(self.hints):
            by_before.setdefault(hint[1], []).append(h)
        # one pass: assigners always come earlier, so the levels fall out of it
        level_of = [0 if v < self.n_given else None for v in range(n_variables)]      # per variable: its assigner's level
        self.form, self.level, self.assigns = [SKIPPED] * nc, [0] * nc, [NONE] * nc
        self.hint_level = [0] * len(self.hints)

        def do_hints(before):
            for h in by_before.get(before, ()):
                _, _, ins, outs, _ = self.hints[h]
                for v in ins:
                    if level_of[v] is None:
                        raise ScheduleError("hint", h, "input variable %d is not assigned in front of constraint %d" % (v, before))
                lv = 1 + max([level_of[v] for v in ins] + [0])
                for v in outs:
                    if level_of[v] is not None:
                        raise ScheduleError("hint", h, "output variable %d is given or assigned twice" % v)
                    level_of[v] = lv
                self.hint_level[h] = lv

        for c, con in enumerate(self.constraints):
            do_hints(c)
            if c in skipped:
                continue
            cells = [v for v, counts in zip(con[:3], counting(self.q[c])) if counts]
            unknown = [v for v in cells if level_of[v] is None]
            if len(set(unknown)) > 1:
                raise ScheduleError("constraint", c, "two unassigned variables (%d, %d)" % tuple(sorted(set(unknown))[:2]))
            if len(unknown) > 1:
                raise ScheduleError("constraint", c, "variable %d is unassigned in two cells (quadratic)" % unknown[0])
            lv = 1 + max([level_of[v] for v in cells if level_of[v] is not None] + [0])
            self.level[c] = lv
            if not unknown:
                self.form[c] = CHECK
                continue
            v = unknown[0]
            where = [i for i, (x, counts) in enumerate(zip(con[:3], counting(self.q[c]))) if counts and x == v][0]
            self.form[c], self.assigns[c] = (SOLVE_L, SOLVE_R, SOLVE_O)[where], v
            level_of[v] = lv
        do_hints(nc)
        self.unassigned = sum(1 for lv in level_of if lv is None)
        self._by_before = by_before

    def levels(self):
        """rule 9 -> {"constraints": a level per constraint (0 for a skipped one), "hints": per listed hint, "commits": per commitment}"""
        return {"constraints": list(self.level), "hints": self.hint_level[:self.n_listed], "commits": self.hint_level[self.n_listed:]}

    def const_divisor(self, c):
        """is constraint c's divisor a coefficient alone (qo, or ql / qr with qm = 0)?"""
        return self.form[c] == SOLVE_O or (self.form[c] in (SOLVE_L, SOLVE_R) and self.q[c][2] == 0)

    def solve(self, inputs, commit=None, stop=True):
        """inputs: the n_public + n_secret given values; commit(j, committed values) -> c_j.  -> (values, failure): failure is
        None or (kind, constraint, value) of the first one.  With stop=False the walk goes on past failures the way the device
        does - a failing solve poisons its variable, an item with a poisoned operand fails nothing and poisons what it would
        assign - and returns (values with None where poisoned, first failure, failures, poisoned variables)."""
        assert len(inputs) == self.n_given
        vals = [int(x) % R for x in inputs] + [0] * (self.n_variables - self.n_given)
        first, failures, poisoned = None, 0, 0

        def hints(before):
            nonlocal poisoned
            for h in self._by_before.get(before, ()):
                kind, _, ins, outs, param = self.hints[h]
                xs = [vals[v] for v in ins]
                if any(x is POISON for x in xs):
                    res = [POISON] * len(outs)
                    poisoned += len(outs)
                elif kind == COMMIT:
                    res = [int(commit(param, xs)) % R]
                else:
                    res = run_hint(kind, xs[0], param)
                for v, x in zip(outs, res):
                    vals[v] = x

        for c, con in enumerate(self.constraints):
            hints(c)
            if self.form[c] == SKIPPED:
                continue
            ops = [vals[v] if counts else 0 for v, counts in zip(con[:3], counting(self.q[c]))]
            if self.form[c] != CHECK:
                ops[self.form[c] - SOLVE_L] = 0
            if any(x is POISON for x in ops):
                if self.form[c] != CHECK:
                    vals[self.assigns[c]] = POISON
                    poisoned += 1
                continue
            kind, out, value = solve_item(self.form[c], self.q[c], *ops)
            if kind != OK:
                failures += 1
                if first is None:
                    first = (kind, c, value)
                if stop:
                    return vals, first
                if self.form[c] != CHECK:
                    vals[self.assigns[c]] = POISON
                    poisoned += 1
            elif out is not None:
                vals[self.assigns[c]] = out
        hints(len(self.constraints))
        if stop:
            return vals, None
        return [None if x is POISON else x for x in vals], first, failures, poisoned


def bsb22_committer(setup_model, srs, commit_blinding, tau=None):
    """the COMMIT hint's value as gnark_bsb22_model rule 3 defines it, for a gnark_plonk_setup_model.Setup: -> (commit(j, committed
    values) -> c_j, the list the points [PI2_j] are appended to)"""
    import gnark_bsb22_model as gb
    com, points = gb.committer(srs, tau), []

    def commit(j, xs):
        info = setup_model.info[j]
        v = [0] * setup_model.n
        for row, x in zip(info["committed"], xs):
            v[row] = x
        v[info["row"]] = int(commit_blinding[2 * j]) % R
        v[info["last_row"]] = int(commit_blinding[2 * j + 1]) % R
        points.append(com(bn.ntt(v, inverse=True)))
        return gb.hash_to_field(bn.g1_marshal(points[-1]))

    return commit, points


if __name__ == "__main__":
    # x * y = z, then z^-1 by hint, then z * inv == 1 as a check
    coeffs = [0, 1, R - 1]
    s = Solver(5, 1, 2, [(1, 2, 3, 0, 0, 1, 2, 0), (3, 4, 0, 0, 0, 1, 0, 2)], coeffs, hints=[("inv_zero", 1, 3, 4)])
    print(s.levels(), s.solve([1, 6, 7]))
