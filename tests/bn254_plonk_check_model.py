"""The yardstick of nlx_bn254_plonk_check_witness on big integers: given a key's values on H
(Instance.key_values() / bn.plonk_witness's dict), the wires, the public inputs and the c_j, the report as a dict with the
fields of include/nlx.h's nlx_bn254_plonk_witness_report (cache_bytes apart: that is the key's history, not the witness's).
Sigma is decoded by a dictionary of the 3 n identity values; "first" follows the header: gates by the lowest row, copies by
the lowest row and then the lowest wire, commitments by the lowest index.

A plain module (not a conftest); it also builds the test instances and the seeded single-cell mutations that
tests/golden/bn254_plonk_check_cells.json records (tests/golden/gen_bn254_plonk_check_cells.py writes the file)."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bsb22_model as gm  # noqa: E402

bn = gm.bn
R = gm.R
CHECK_GATES, CHECK_COPIES, CHECK_COMMITS, CHECK_ALL = 1, 2, 4, 7
WIRES = ("l", "r", "o")
GOLDEN = os.path.join(HERE, "golden", "bn254_plonk_check_cells.json")
FIELDS = ("checked", "satisfied", "gate_rows_bad", "gate_rows_skipped", "gate_row", "gate_value", "copy_cells_bad", "copy_row", "copy_wire",
          "copy_to_row", "copy_to_wire", "copy_value", "copy_to_value", "commits_bad", "commit_index", "commit_row", "commit_have",
          "commit_want")


def decode_sigma(values, k1, k2):
    """s1 s2 s3 -> [wire][row] = (to_wire, to_row), by a dictionary of the 3 n identity values; KeyError for a value in no coset"""
    n = len(values["s1"])
    w = bn.root_of_unity(n.bit_length() - 1)
    ident, x = {}, 1
    for i in range(n):
        for c, k in enumerate((1, k1, k2)):
            ident[k * x % R] = (c, i)
        x = x * w % R
    assert len(ident) == 3 * n, "the cosets H, k1 H, k2 H are not disjoint"
    return [[ident[int(v) % R] for v in values[name]] for name in ("s1", "s2", "s3")]


def gate_value(values, wires, i, pi, m):
    l, r, o = (int(wires[c][i]) % R for c in range(3))
    return (values["ql"][i] * l + values["qr"][i] * r + values["qm"][i] * l * r + values["qo"][i] * o + values["qk"][i] + pi + m * l) % R


def check(values, l, r, o, public_inputs=(), cs=None, info=(), k1=5, k2=25, what=CHECK_ALL):
    """cs: the c_j the COMMITS pass computes (needed when `what` holds CHECK_COMMITS and the key has commitments);
    info: Instance.commitment_info()"""
    n, k = len(values["ql"]), len(info)
    wires = [[int(x) % R for x in col] for col in (l, r, o)]
    if not k:
        what &= ~CHECK_COMMITS
    rep = dict.fromkeys(FIELDS, 0)
    rep["checked"] = what
    with_c = bool(what & CHECK_COMMITS)
    if with_c:
        for j in range(k):
            have, want = wires[0][info[j]["row"]], int(cs[j]) % R
            if have != want:
                if not rep["commits_bad"]:
                    rep.update(commit_index=j, commit_row=info[j]["row"], commit_have=have, commit_want=want)
                rep["commits_bad"] += 1
    if what & CHECK_GATES:
        pi, mult, skip = {}, [0] * n, set()
        for i, x in enumerate(public_inputs):
            pi[i] = int(x) % R
        for j in range(k):
            for i in info[j]["committed"]:
                mult[i] += 1
            if with_c:
                pi[info[j]["row"]] = int(cs[j]) % R
            else:
                skip.add(info[j]["row"])
        rep["gate_rows_skipped"] = len(skip)
        for i in range(n):
            if i in skip:
                continue
            v = gate_value(values, wires, i, pi.get(i, 0), mult[i])
            if v:
                if not rep["gate_rows_bad"]:
                    rep.update(gate_row=i, gate_value=v)
                rep["gate_rows_bad"] += 1
    if what & CHECK_COPIES:
        cells = decode_sigma(values, k1, k2)
        for i in range(n):
            for c in range(3):
                tc, ti = cells[c][i]
                if wires[c][i] != wires[tc][ti]:
                    if not rep["copy_cells_bad"]:
                        rep.update(copy_row=i, copy_wire=c, copy_to_row=ti, copy_to_wire=tc, copy_value=wires[c][i], copy_to_value=wires[tc][ti])
                    rep["copy_cells_bad"] += 1
    rep["satisfied"] = int(not (rep["gate_rows_bad"] or rep["copy_cells_bad"] or rep["commits_bad"]))
    return rep


# ---- the instances of the tests: one definition, shared by the CPU and the GPU file and by the golden generator ----
class Case:
    """values (the key's), wires l r o, public inputs, the commitments' description, their blinding, the test SRS's trapdoor"""

    def __init__(self, log_n, k, n_pi, seed=0):
        rng = random.Random(35000 + 1000 * k + 10 * log_n + n_pi + 7919 * seed)
        self.log_n, self.n, self.k, self.n_pi = log_n, 1 << log_n, k, n_pi
        self.k1, self.k2 = 5, 25
        self.tau = rng.randrange(1, R)
        self.blind = [rng.randrange(R) for _ in range(9)]
        self.cblind = [rng.randrange(R) for _ in range(2 * k)]
        if k:
            inst = self.inst = gm.Instance(log_n, k, rng, n_pi=n_pi, chain=True)
            self.values, self.info, self.pubs = inst.key_values(), inst.commitment_info(), list(inst.public_inputs)   # shares the lists

            def set_o(i, x):
                inst.values.append(x)
                inst.cells[2][i] = len(inst.values) - 1
            self._aim(rng, lambda i: inst.values[inst.cells[2][i]], set_o)
            self.wires, self.cs = self.solve(self.cblind)
        else:
            p = bn.plonk_witness(log_n, rng, 5, 25, 11, 13)
            self.inst = None
            self.pubs = [rng.randrange(R) for _ in range(n_pi)]
            p["qk"] = [(a - (self.pubs[i] if i < n_pi else 0)) % R for i, a in enumerate(p["qk"])]
            self.wires = [list(p.pop(c)) for c in WIRES]
            p.pop("z")
            self.values, self.info, self.cs = p, [], []
            self._aim(rng, lambda i: self.wires[2][i], lambda i, x: self.wires[2].__setitem__(i, x))

    def _aim(self, rng, get_o, set_o):
        """Two cells of the O wire, on rows without a role in a commitment, that the generators do not produce:
        gate_only - (2, row) holds a value of its own and is its own cycle: changing it breaks its gate and no copy;
        copy_only - (2, row) sits in a cycle with other cells and its row has qo = 0: changing it breaks copies and no gate.
        The instance stays satisfied: qk is refitted on both rows, sigma is re-linked around the first cell."""
        v, n = self.values, self.n
        free = [i for i in range(n) if not any(i == c["row"] or i in c["committed"] for c in self.info)]
        sig = (v["s1"], v["s2"], v["s3"])
        cells = decode_sigma(v, self.k1, self.k2)
        b = free[-1]
        if cells[2][b] != (2, b):
            pc, pi = next((c, i) for c in range(3) for i in range(n) if cells[c][i] == (2, b))
            sig[pc][pi], sig[2][b] = sig[2][b], sig[pc][pi]
            cells[pc][pi], cells[2][b] = cells[2][b], (2, b)
        fresh = rng.randrange(R)
        v["qk"][b] = (v["qk"][b] + v["qo"][b] * (get_o(b) - fresh)) % R
        set_o(b, fresh)
        a = next(i for i in free if i != b and cells[2][i] != (2, i))
        v["qk"][a] = (v["qk"][a] + v["qo"][a] * get_o(a)) % R
        v["qo"][a] = 0
        self.gate_only, self.copy_only = (2, b), (2, a)

    def c_values(self, l, cblind):
        """the c_j of a FINISHED L wire, as the prover's round 0 and the checker compute them (the commitment through the trapdoor)"""
        out = []
        for j in range(self.k):
            co = bn.ntt(gm.pi2_values(self.inst, j, l, cblind[2 * j], cblind[2 * j + 1]), inverse=True)
            out.append(gm.hash_to_field(bn.g1_marshal(bn.g1_mul(bn.eval_poly(co, self.tau), bn.G1))))
        return out

    def solve(self, cblind):
        cs = []
        for j in range(self.k):
            cs.append(self.c_values(self.inst.complete(cs)[0], cblind)[j])
        return [list(c) for c in self.inst.complete(cs)], cs

    def check(self, wires=None, pubs=None, cblind=None, what=CHECK_ALL):
        wires = self.wires if wires is None else wires
        cs = self.c_values(wires[0], self.cblind if cblind is None else cblind) if self.k and what & CHECK_COMMITS else None
        return check(self.values, wires[0], wires[1], wires[2], self.pubs if pubs is None else pubs, cs, self.info, self.k1, self.k2, what)


def mutations(case, count, seed):
    """`count` seeded single-cell mutations of a case's wires: (wire, row, new value) - half take a fresh value, half another
    cell's (a value that is at home elsewhere in the trace)"""
    rng = random.Random(seed)
    out = []
    for t in range(count):
        c, i = rng.randrange(3), rng.randrange(case.n)
        v = rng.randrange(R) if t % 2 == 0 else case.wires[rng.randrange(3)][rng.randrange(case.n)]
        if v == case.wires[c][i]:
            v = (v + 1) % R
        out.append((c, i, v))
    return out


def mutated(case, cell):
    c, i, v = cell
    wires = [list(col) for col in case.wires]
    wires[c][i] = v
    return wires


GOLDEN_CASES = ((5, 0, 3), (5, 2, 2), (8, 0, 0), (8, 1, 2))   # (log_n, k, n_pi): ten mutations each


def golden_records():
    """forty seeded single-cell mutations at 2^5 and 2^8 and the yardstick's report of each (values as hex strings)"""
    out = []
    for log_n, k, n_pi in GOLDEN_CASES:
        case = Case(log_n, k, n_pi)
        for cell in mutations(case, 10, 100 * log_n + k):
            rep = case.check(mutated(case, cell))
            out.append({"log_n": log_n, "k": k, "n_pi": n_pi, "wire": cell[0], "row": cell[1], "value": "%x" % cell[2],
                        "report": {f: ("%x" % v if f.endswith(("_value", "_have", "_want")) else v) for f, v in rep.items()}})
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
