#!/usr/bin/env python3
"""gnark's plonk.Setup(spr, srs) over BN254 on big integers: from a sparse constraint system (gnark's SparseR1CS: per constraint
three variable ids and five coefficient ids) to the trace on H - the selectors, the Bsb22 selectors qcp_j, the copy permutation
and s1 s2 s3 - plus the gather from a solved variable vector to the l r o columns and the test SRS from a trapdoor.  The
yardstick of nlx_bn254_plonk_setup (csrc/bn254_plonk_setup.hip); it shares no code with the device side.
Field, NTT and group come from the frozen oracle/bn254_py.py.

Status of every rule: RECALLED from gnark v0.9 backend/plonk/bn254 setup.go (and gnark-crypto kzg.NewSRS), UNPINNED - there is
no Go source and no gnark-produced key to compare with; parity with gnark-produced keys is not claimed.  Each rule is written
once, here.  N = n_public + n_constraints, n = 2^log_n >= N, u = the coset shift.

  rule 1  rows          row i < n_public: ql = -1, qr = qm = qo = qk = 0, cells L = variable i, R = O = variable 0;
                        row n_public + c = constraint c: its selectors from the coefficient table, its cells (xa, xb, xc);
                        rows N .. n - 1: every selector 0, every cell variable 0.  qk holds the constraints' constants only:
                        the public inputs enter at proof time                                                 (rows)
  rule 2  commitments   commitment j names committed constraint indices (ascending) and one commitment constraint; the rows
                        are those indices + n_public; qcp_j = 1 on j's committed rows, 0 elsewhere; last_row = N - 1.  The
                        constraints' own selectors (ql = -1 on those rows) are the circuit's business        (commitments)
  rule 3  permutation   over positions p = col * n + row, col 0 1 2 = L R O: walking p upward, perm[p] = the previous
                        position holding the same variable; the first position of a variable takes that variable's LAST
                        position; a variable seen once maps to itself (gnark's buildPermutation links a position to its
                        predecessor)                                                                          (permutation)
  rule 4  sigma         s_col(w^row) = id[perm[col * n + row]], id[c * n + i] = (1, k1, k2)[c] * w^i; gnark: k1 = u,
                        k2 = u^2                                                                              (sigma)
  rule 5  SRS           kzg.NewSRS(size, tau), test use only: G1 = [tau^i]_1 for i < size, G2 = [1]_2, [tau]_2  (kzg_srs)
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import bn254_py as bn  # noqa: E402

R = bn.R
SELECTORS = ("ql", "qr", "qm", "qo", "qk")


def smallest_log_n(n_used):
    log_n = 3
    while (1 << log_n) < n_used:
        log_n += 1
    return log_n


# ---- rule 1 ----
def rows(n_public, constraints, coeffs, log_n):
    """constraints: (xa, xb, xc, ql, qr, qm, qo, qk) per constraint - three variable ids, five ids into coeffs.
    -> ({name: n values}, [3][n] variable ids)"""
    n, used = 1 << log_n, n_public + len(constraints)
    assert used <= n
    sel = {name: [0] * n for name in SELECTORS}
    cells = [[0] * n for _ in range(3)]
    for i in range(n_public):
        sel["ql"][i] = R - 1
        cells[0][i] = i
    for c, con in enumerate(constraints):
        i = n_public + c
        cells[0][i], cells[1][i], cells[2][i] = con[0], con[1], con[2]
        for name, cid in zip(SELECTORS, con[3:8]):
            sel[name][i] = int(coeffs[cid]) % R
    return sel, cells


# ---- rule 2 ----
def commitments(n_public, n_constraints, sets, log_n):
    """sets: ({"committed": ascending constraint indices, "constraint": the commitment constraint}, ..)
    -> ([qcp_j values], ResidentKey's commitment description)"""
    n = 1 << log_n
    qcp, info = [], []
    for s in sets:
        committed = [int(c) + n_public for c in s["committed"]]
        assert committed == sorted(set(committed)) and all(n_public <= i < n_public + n_constraints for i in committed)
        q = [0] * n
        for i in committed:
            q[i] = 1
        qcp.append(q)
        info.append({"committed": committed, "row": int(s["constraint"]) + n_public, "last_row": n_public + n_constraints - 1})
    return qcp, info


# ---- rule 3 ----
def permutation(cells):
    n = len(cells[0])
    flat = cells[0] + cells[1] + cells[2]
    perm, previous, first = [0] * (3 * n), {}, {}
    for p, v in enumerate(flat):
        if v in previous:
            perm[p] = previous[v]
        else:
            first[v] = p
        previous[v] = p
    for v, p in first.items():
        perm[p] = previous[v]          # the variable's last position
    return perm


# ---- rule 4 ----
def sigma(perm, log_n, k1, k2):
    n = 1 << log_n
    w = bn.root_of_unity(log_n)
    powers, x = [], 1
    for _ in range(n):
        powers.append(x)
        x = x * w % R
    shift = (1, k1 % R, k2 % R)
    s = [shift[q // n] * powers[q % n] % R for q in perm]
    return s[:n], s[n:2 * n], s[2 * n:]


def sigma_value(q, log_n, k1, k2):
    """id[q] alone (the sizes where the whole table is too slow)"""
    n = 1 << log_n
    return (1, k1 % R, k2 % R)[q // n] * pow(bn.root_of_unity(log_n), q % n, R) % R


def sigma_cells(perm, log_n):
    """the witness checker's encoding of the permutation: col << 30 | row"""
    n = 1 << log_n
    return [(q // n) << 30 | (q % n) for q in perm]


class Setup:
    """the whole of plonk.Setup: .values (Instance.key_values()'s shape), .cells, .perm, .info (ResidentKey's commitments)"""

    def __init__(self, n_variables, n_public, constraints, coeffs, k1=5, k2=25, commitments_=(), log_n=0, with_sigma=True):
        self.n_variables, self.n_public, self.n_constraints = n_variables, n_public, len(constraints)
        self.used = n_public + len(constraints)
        self.log_n = log_n or smallest_log_n(self.used)
        self.n, self.k1, self.k2, self.k = 1 << self.log_n, k1, k2, len(commitments_)
        assert n_variables >= max(1, n_public) and all(0 <= v < n_variables for con in constraints for v in con[:3])
        sel, self.cells = rows(n_public, constraints, coeffs, self.log_n)
        self.qcp, self.info = commitments(n_public, len(constraints), commitments_, self.log_n)
        self.perm = permutation(self.cells)
        self.values = dict(sel)
        if with_sigma:
            self.values["s1"], self.values["s2"], self.values["s3"] = sigma(self.perm, self.log_n, k1, k2)
        for j, q in enumerate(self.qcp):
            self.values["qcp%d" % j] = q

    def sigma_cells(self):
        return sigma_cells(self.perm, self.log_n)

    def wires(self, variables):
        """the solver's last step: l[row] = variables[cell]"""
        return tuple([int(variables[v]) % R for v in col] for col in self.cells)

    def classes(self):
        """variable -> its positions, ascending"""
        out = {}
        for p, v in enumerate(self.cells[0] + self.cells[1] + self.cells[2]):
            out.setdefault(v, []).append(p)
        return out


# ---- rule 5 ----
def kzg_srs(tau, size):
    """-> ([tau^i]_1 for i < size, [1]_2, [tau]_2)"""
    return bn.kzg_srs(tau, size), bn.G2, bn.g2_mul(tau, bn.G2)


if __name__ == "__main__":
    s = Setup(4, 1, [(1, 2, 3, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0)], [0], log_n=3)
    print("perm =", s.perm)
