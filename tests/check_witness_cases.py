"""Yardsticks of the witness checker's tests (nlx_circuit_check_witness): the circuits, the mutations, a dictionary decode of sigma
and an exact restatement of four gates.  tests/test_check_witness_cpu.py checks these against the CPU oracle,
tests/test_gpu_check_witness.py uses them.

A plain module (not a conftest).  Run as a script it rewrites tests/golden/check_witness_cells.json from the oracle's verdicts."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import POW2_GEN, P  # noqa: E402

ALL19 = dict(pct_poseidon=10, pct_arithmetic=10, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=20, pct_u32=30)
LOOKUP = dict(seed=5, num_luts=1, lut_bits=6, num_lookups=100)     # 2^9 rows: lookup_rows = [1, 4, 6]
# the circuits of the random single-cell mutations: key of the golden file -> (log_n, seed, gate mix)
CELL_CIRCUITS = {"8": (8, 21, ALL19), "5": (5, 1, {})}
GOLDEN = os.path.join(HERE, "golden", "check_witness_cells.json")
(NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC, BASE_SUM, POSEIDON) = range(6)
RESTATED = (CONSTANT, PUBLIC_INPUT, ARITHMETIC, BASE_SUM)
ROUTED, NUM_WIRES = 80, 135


def sigma_cells(syn):
    """sigma decoded with a dictionary of every k_j w^i (test_oracle_prover.py::test_sigma_is_a_permutation_respecting_copies):
    (to_col, to_row), each (80, n)"""
    n = 1 << syn.log_n
    w = pow(POW2_GEN, 1 << (32 - syn.log_n), P)
    sub = [1] * n
    for i in range(1, n):
        sub[i] = sub[i - 1] * w % P
    ids = {}
    for j in range(ROUTED):
        k = int(syn.k_is[j])
        for i in range(n):
            ids[k * sub[i] % P] = (j, i)
    assert len(ids) == ROUTED * n
    to_col = np.zeros((ROUTED, n), dtype=np.int64)
    to_row = np.zeros((ROUTED, n), dtype=np.int64)
    for j in range(ROUTED):
        for i in range(n):
            to_col[j, i], to_row[j, i] = ids[int(syn.sigmas[j, i])]
    return to_col, to_row


def row_gates(syn):
    """the index into syn.gates of every row's gate: the one whose selector column holds its index there"""
    n = 1 << syn.log_n
    out = np.full(n, -1, dtype=np.int64)
    for g in syn.gates:
        rows = syn.constants[g.selector_index] == np.uint64(g.index)
        assert np.all(out[rows] == -1)
        out[rows] = g.index
    assert np.all(out >= 0)
    return out


def first_rows_by_kind(syn):
    """{gate kind: its first row}, NoopGate left out"""
    rg = row_gates(syn)
    out = {}
    for row, gi in enumerate(rg):
        kind = syn.gates[int(gi)].kind
        if kind != NOOP:
            out.setdefault(kind, row)
    return out


def random_cells(log_n):
    """forty single-cell mutations (column, row, increment) in the style of
    test_gpu_bn128_prove.py::test_unsatisfied_witness_is_refused: any of the 135 columns, any row, the value raised by 1 .. 5;
    column, row and increment are drawn cell by cell"""
    rng = np.random.default_rng(7)
    return [(int(rng.integers(0, NUM_WIRES)), int(rng.integers(0, 1 << log_n)), 1 + int(rng.integers(0, 5))) for _ in range(40)]


def mutated(wires, col, row, inc=1):
    w = wires.copy()
    w[col, row] = (int(w[col, row]) + inc) % P
    return w


def restate(syn, wires, row, pih):
    """the constraints of ConstantGate, PublicInputGate, ArithmeticGate or BaseSumGate on one row, in plonky2's order, as python
    ints (None for another gate)"""
    g = syn.gates[int(row_gates(syn)[row])]
    c0 = syn.num_selectors + syn.num_lookup_selectors      # first gate constant
    W = lambda i: int(wires[i, row])                       # noqa: E731
    C = lambda i: int(syn.constants[c0 + i, row])          # noqa: E731
    if g.kind == CONSTANT:
        return [(C(i) - W(i)) % P for i in range(g.param0)]
    if g.kind == PUBLIC_INPUT:
        return [(W(i) - int(pih[i])) % P for i in range(4)]
    if g.kind == ARITHMETIC:
        return [(W(4 * i + 3) - (W(4 * i) * W(4 * i + 1) * C(0) + W(4 * i + 2) * C(1))) % P for i in range(g.param0)]
    if g.kind == BASE_SUM:
        B, nl = g.param0, g.param1
        out = [(sum(W(1 + i) * B ** i for i in range(nl)) - W(0)) % P]
        for i in range(nl):
            prod = 1
            for t in range(B):
                prod = prod * (W(1 + i) - t) % P
            out.append(prod)
        return out
    return None


def first_nonzero(constraints):
    return next(((i, v) for i, v in enumerate(constraints) if v), None)


def oracle_verdicts(nlx, orc, key):
    """[column, row, increment, 1 if the oracle's verifier accepts the oracle's proof of the mutated witness] per random cell"""
    log_n, seed, kw = CELL_CIRCUITS[key]
    syn = nlx.SyntheticCircuit(log_n, seed=seed, **kw)
    ref = orc.Circuit.from_synthetic(syn)
    try:
        return [[c, r, inc, int(ref.verify(ref.prove(mutated(syn.wires, c, r, inc), syn.public_inputs)) == 1)]
                for c, r, inc in random_cells(log_n)]
    finally:
        ref.close()


def golden_cells():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
    import nlxpkg
    import oracle_py
    oracle_py.dll()
    pkg = nlxpkg.load()
    with open(GOLDEN, "w") as f:
        json.dump({k: oracle_verdicts(pkg, oracle_py, k) for k in CELL_CIRCUITS}, f)
        f.write("\n")
