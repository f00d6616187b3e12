"""Shared cases of the Groth16 setup tests (tests/test_groth16_setup_cases_cpu.py validates them without a GPU,
tests/test_gpu_bn254_groth16_setup.py holds the device against them): the aimed R1CS instances, each with its trapdoor, and
`setup_logs`, the discrete logs of every array of gnark's keys - what a setup's points must be multiples of the generators by -
from the model's wire_polys_at / k_logs, without making a point.  The models are tools/groth16_model.py (rule 3) and
tools/groth16_commit_model.py (rule 1): recalled from gnark v0.9, unpinned.

The generated instances: every shape of gm.SHAPES once, and every size of 8, 13, 50, 200 and 333 constraints at least once (333
is no power of two and leaves 179 padding rows; `long` has rows of 300 terms; all_a / all_b put one row over every wire).  No
generated instance gives one wire more than a dozen terms of a matrix, so the hand-made ones carry the columns' edge cases:
  cancel     wire 1 occurs in A twice in one row, with c and -c, and nowhere else in A: it occurs, and A_1(tau) = 0
  one_every  wire 0 (ONE) sits in every row of A: at 12 constraints a short column, at 100 one of more than 64 terms (the
             device sums such a wire with a whole wave)"""
import functools
import os
import random
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_commit_model as cm  # noqa: E402
import groth16_model as gm  # noqa: E402

bn, R = gm.bn, gm.R
inv = gm.inv

GENERATED = [("common", 8), ("public3", 13), ("long", 50), ("all_a", 200), ("all_b", 333), ("empty", 13), ("absent", 50), ("unit", 200),
             ("general", 8)]
COMMITTED = [("common", 16, [3]), ("public3", 24, [2, 0]), ("unit", 40, [1, 4, 2])]        # k = 1, 2, 3; an empty set among them
CASE_NAMES = ["%s-%d" % c for c in GENERATED] + ["cancel", "one_every-12", "one_every-100"]
COMMITTED_NAMES = ["%s-%d-k%d" % (s, n, len(c)) for s, n, c in COMMITTED]


class HandInstance(gm.Instance):
    """an instance from its rows: rows[m][row] = [(wire, coefficient id)], a coefficient table and a satisfying witness"""

    def __init__(self, rows, coeffs, witness, n_public):
        self.rows, self.coeffs, self.witness = rows, list(coeffs), list(witness)
        self.n_constraints, self.n_public, self.n_wires = len(rows["A"]), n_public, len(witness)
        self.log_n = max(1, (self.n_constraints - 1).bit_length())
        self.n = 1 << self.log_n
        self.csr = {}
        for name in "ABC":
            row_ptr, wire, cid = [0], [], []
            for r_ in rows[name]:
                wire += [i for i, _ in r_]
                cid += [c for _, c in r_]
                row_ptr.append(len(wire))
            self.csr[name] = (row_ptr, wire, cid)
        assert self.satisfied()


def cancel_instance(rng):
    c = rng.randrange(2, R - 1)
    coeffs = [1, c, R - c]
    w = [1] + [rng.randrange(R) for _ in range(3)]
    w.append(w[2] * w[3] % R)                         # row 0: (c w1 - c w1 + w2) * w3 = w4
    w.append(w[2] * w[1] % R)                         # row 1: w2 * w1 = w5 - wire 1 is used, in B
    w.append((w[4] + w[0]) * w[5] % R)                # row 2: (w4 + ONE) * w5 = w6
    rows = {"A": [[(1, 1), (2, 0), (1, 2)], [(2, 0)], [(4, 0), (0, 0)]],
            "B": [[(3, 0)], [(1, 0)], [(5, 0)]],
            "C": [[(4, 0)], [(5, 0)], [(6, 0)]]}
    return HandInstance(rows, coeffs, w, 1)


def one_every_instance(n_constraints, rng, n_public=1):
    """row r: (k ONE + w_s) * w_t = a new wire; s, t among the wires that exist"""
    coeffs = [1, R - 1] + [rng.randrange(2, R - 1) for _ in range(6)]
    w = [1] + [rng.randrange(R) for _ in range(n_public - 1 + 3)]
    rows = {"A": [], "B": [], "C": []}
    for _ in range(n_constraints):
        k, s, t = rng.randrange(len(coeffs)), rng.randrange(1, len(w)), rng.randrange(1, len(w))
        rows["A"].append([(0, k), (s, 0)])
        rows["B"].append([(t, 0)])
        rows["C"].append([(len(w), 0)])
        w.append((coeffs[k] + w[s]) * w[t] % R)
    return HandInstance(rows, coeffs, w, n_public)


@functools.lru_cache(maxsize=None)
def case(name):
    """(instance, trapdoor) of one named case of CASE_NAMES / COMMITTED_NAMES"""
    rng = random.Random("groth16-setup-" + name)
    if name == "cancel":
        inst = cancel_instance(rng)
    elif name.startswith("one_every-"):
        inst = one_every_instance(int(name.split("-")[1]), rng)
    elif name in COMMITTED_NAMES:
        shape, n, counts = COMMITTED[COMMITTED_NAMES.index(name)]
        inst = cm.CommittedInstance(n, rng, counts, **gm.SHAPES[shape])
        return inst, cm.Trapdoor.random(rng)
    else:
        shape, n = name.rsplit("-", 1)
        inst = gm.Instance(int(n), rng, **gm.SHAPES[shape])
    return inst, gm.Trapdoor.random(rng)


def setup_logs(inst, td):
    """The discrete logs of every key array, in the layout of gm.setup's / cm.setup's (pk, vk) with two additions to vk: g1_alpha,
    g2_beta, g2_delta, and for an instance with commitments pedersen_g = 1, pedersen_g_root_sigma_neg = -sigma (rule 1 takes
    BasisExpSigma = sigma Basis: tools/bn254_pairing_model.py pedersen_vk)."""
    n = inst.n
    at, bt, _ = gm.wire_polys_at(inst, td.tau)
    k_all = cm.k_logs(inst, td)
    zh = (pow(td.tau, n, R) - 1) % R
    dinv, ginv = inv(td.delta), inv(td.gamma)
    commitments = getattr(inst, "commitments", [])
    kept = inst.k_wires() if commitments else list(range(inst.n_public, inst.n_wires))
    pk = {"infinity_a": [x == 0 for x in at], "infinity_b": [x == 0 for x in bt],
          "g1_a": [x for x in at if x], "g1_b": [x for x in bt if x], "g2_b": [x for x in bt if x],
          "g1_k": [k_all[i] * dinv % R for i in kept],
          "g1_z": [pow(td.tau, i, R) * zh % R * dinv % R for i in range(n - 1)],
          "g1_alpha": td.alpha, "g1_beta": td.beta, "g1_delta": td.delta, "g2_beta": td.beta, "g2_delta": td.delta}
    vk = {"g1_alpha": td.alpha, "g2_beta": td.beta, "g2_gamma": td.gamma, "g2_delta": td.delta,
          "ic": [k_all[i] * ginv % R for i in range(inst.n_public)] + [k_all[c["wire"]] * ginv % R for c in commitments]}
    if commitments:
        pk["commitments"] = [{"basis": [k_all[i] * ginv % R for i in c["private"]],
                              "basis_exp_sigma": [k_all[i] * ginv % R * td.sigma % R for i in c["private"]]} for c in commitments]
        vk["pedersen_g"], vk["pedersen_g_root_sigma_neg"] = 1, (R - td.sigma) % R
    return pk, vk


def r1cs_arrays(np, fr_pack, inst):
    """the instance's matrices as the binding takes them"""
    out = {m: (np.array(inst.csr[m][0], dtype=np.uint64), np.array(inst.csr[m][1], dtype=np.uint32), np.array(inst.csr[m][2], dtype=np.uint32))
           for m in "ABC"}
    out["coeffs"] = fr_pack(inst.coeffs)
    return out
