"""GPU tests of nlx_circuit_check_witness (csrc/prover.hip, the checker kernels of csrc/prover_kernels.hip and csrc/lookup_arg.hip):
verdicts against the CPU oracle's (tests/golden/check_witness_cells.json, pinned by tests/test_check_witness_cpu.py), locations
against the mutations, constraint indices and values against the exact restatement of tests/check_witness_cases.py."""
import ctypes

import numpy as np
import pytest

import check_witness_cases as cw
import quotient_aims as qa
from conftest import P

pytestmark = pytest.mark.gpu

NLX_E_INVAL = -1
GATES, COPIES, LOOKUPS, ALL = 1, 2, 4, 7
BN = "poseidon_bn128"


class Case:
    def __init__(self, nlx, ctx, log_n, hasher="poseidon_goldilocks", **kw):
        self.syn = nlx.SyntheticCircuit(log_n, **kw)
        self.cd = nlx.CircuitData.from_synthetic(ctx, self.syn, hasher=hasher)
        self.n = 1 << log_n

    def check(self, wires, what=ALL):
        """the report, after asserting that the call left the witness buffer as it was"""
        before = wires.copy() if isinstance(wires, np.ndarray) else wires.clone()
        rep = self.cd.check_witness(wires, self.syn.public_inputs, what)
        if isinstance(wires, np.ndarray):
            assert np.array_equal(wires, before)
        else:
            assert bool((wires == before).all())
        return rep


@pytest.fixture(scope="module")
def c5(nlx, ctx):
    c = Case(nlx, ctx, 5, seed=1)
    yield c
    c.cd.close()


@pytest.fixture(scope="module")
def c8(nlx, ctx):
    c = Case(nlx, ctx, 8, seed=21, **cw.ALL19)
    yield c
    c.cd.close()


@pytest.fixture(scope="module")
def c10(nlx, ctx):
    c = Case(nlx, ctx, 10, seed=21, **cw.ALL19)
    yield c
    c.cd.close()


@pytest.fixture(scope="module")
def clk(nlx, ctx):
    c = Case(nlx, ctx, 9, **cw.LOOKUP)
    yield c
    c.cd.close()


def _clean(rep, checked):
    assert rep.ok and rep.satisfied == 1 and rep.checked == checked
    assert (rep.gate_rows_bad, rep.copy_cells_bad, rep.lookup_slots_bad) == (0, 0, 0)
    assert "satisfies" in str(rep)
    rep.raise_if_unsatisfied()


@pytest.mark.parametrize("name,checked", [("c5", 3), ("c8", 3), ("c10", 3), ("clk", 7)])
def test_satisfied_witnesses_host_and_device(request, name, checked):
    import torch
    c = request.getfixturevalue(name)
    _clean(c.check(c.syn.wires), checked)
    dev = torch.from_numpy(c.syn.wires.view(np.int64)).cuda()
    _clean(c.check(dev), checked)
    _clean(c.check(dev), checked)                         # a later check: the cached constants on H and sigma cells
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), c.syn.wires)


def test_satisfied_under_the_bn128_config(nlx, ctx):
    c = Case(nlx, ctx, 8, hasher=BN, seed=21, **cw.ALL19)
    try:
        _clean(c.check(c.syn.wires), 3)
        rep = c.check(cw.mutated(c.syn.wires, 0, 0))
        assert not rep.ok and rep.gate_row == 0 and rep.gate_kind == cw.PUBLIC_INPUT
    finally:
        c.cd.close()


@pytest.mark.parametrize("key", ["8", "5"])
def test_verdicts_equal_the_oracles_and_name_the_cell(request, key):
    import torch
    c = request.getfixturevalue("c" + key)
    to_col, to_row = cw.sigma_cells(c.syn)
    said_bad = 0
    for col, row, inc, satisfied in cw.golden_cells()[key]:
        w = cw.mutated(c.syn.wires, col, row, inc)
        rep = c.check(w)
        assert rep.satisfied == satisfied, (col, row, str(rep))
        assert c.check(torch.from_numpy(w.view(np.int64)).cuda()).satisfied == satisfied
        if not satisfied:
            said_bad += 1
            at_row = rep.gate_rows_bad > 0 and rep.gate_row == row
            at_copy = rep.copy_cells_bad > 0 and (col, row) in ((rep.copy_col, rep.copy_row), (rep.copy_to_col, rep.copy_to_row))
            assert at_row or at_copy, (col, row, str(rep))
            assert str(rep).startswith("the witness does not satisfy the circuit: ")
            with pytest.raises(ValueError):
                rep.raise_if_unsatisfied()
    assert 10 <= said_bad <= 30


def test_every_gate_kind_is_named_with_its_constraint(orc, c8):
    syn = c8.syn
    pih = orc.hash_no_pad(syn.public_inputs)
    names = {cw.CONSTANT: "ConstantGate", cw.PUBLIC_INPUT: "PublicInputGate", cw.ARITHMETIC: "ArithmeticGate", cw.BASE_SUM: "BaseSumGate",
             cw.POSEIDON: "PoseidonGate"}
    first = cw.first_rows_by_kind(syn)
    assert len(first) == 18
    for kind, row in first.items():
        w = cw.mutated(syn.wires, 0, row)
        rep = c8.check(w)
        assert not rep.ok and rep.gate_rows_bad == 1 and rep.gate_row == row and rep.gate_kind == kind, (kind, row, str(rep))
        assert syn.gates[rep.gate_index].kind == kind and syn.constants[syn.gates[rep.gate_index].selector_index, row] == rep.gate_index
        if kind in cw.RESTATED:
            assert (rep.gate_constraint, rep.gate_value) == cw.first_nonzero(cw.restate(syn, w, row, pih)), (kind, str(rep))
        if kind in names:
            assert "row %d (%s" % (row, names[kind]) in str(rep)


def test_first_means_the_lowest_row(c10):
    syn = c10.syn
    rg = cw.row_gates(syn)
    rows = [r for r in range(c10.n) if syn.gates[int(rg[r])].kind == cw.BASE_SUM]     # wire 0 is the sum: constraint 0 reads it
    lo = next(r for r in rows if r < 256)
    hi = next(r for r in rows if r >= 512)
    w = cw.mutated(cw.mutated(syn.wires, 0, hi), 0, lo)
    rep = c10.check(w, GATES)
    assert rep.checked == GATES and rep.gate_rows_bad == 2 and rep.gate_row == lo and rep.gate_constraint == 0
    assert rep.gate_value == P - 1                        # sum - (wire 0 + 1)
    rep = c10.check(cw.mutated(syn.wires, 0, hi), GATES)
    assert rep.gate_rows_bad == 1 and rep.gate_row == hi


def test_copies_are_exact(c10):
    syn, n = c10.syn, c10.n
    to_col, to_row = cw.sigma_cells(syn)
    cols, rows = np.meshgrid(np.arange(cw.ROUTED), np.arange(n), indexing="ij")
    moved = (to_col != cols) | (to_row != rows)
    cells = sorted(zip(rows[moved].tolist(), cols[moved].tolist()))                  # (row, column), lowest row first
    far = next((r, c) for r, c in cells if to_row[c, r] // 256 != r // 256)          # the copy lives in another block of rows
    wide = next((r, c) for r, c in cells if c >= 64)
    picks = [cells[0], cells[-1], far, wide] + [cells[(i * len(cells)) // 7] for i in range(1, 7)]
    assert len(picks) == 10 and cells[0][0] == min(r for r, _ in cells) and cells[-1][0] == max(r for r, _ in cells)
    for row, col in picks:
        w = cw.mutated(syn.wires, col, row)
        bad = w[:cw.ROUTED] != w[to_col, to_row]
        want = sorted(zip(rows[bad].tolist(), cols[bad].tolist()))
        assert len(want) == 2 and (row, col) in want
        rep = c10.check(w, COPIES)
        assert not rep.ok and rep.checked == COPIES and rep.copy_cells_bad == 2 and rep.gate_rows_bad == 0
        r0, c0 = want[0]
        assert (rep.copy_row, rep.copy_col) == (r0, c0)
        assert (rep.copy_to_row, rep.copy_to_col) == (to_row[c0, r0], to_col[c0, r0])
        assert rep.copy_value == int(w[c0, r0]) and rep.copy_to_value == int(w[to_col[c0, r0], to_row[c0, r0]])
        assert "copy: wire %d of row %d" % (c0, r0) in str(rep)
        gates_only = c10.check(w, GATES)
        assert gates_only.checked == GATES and gates_only.copy_cells_bad == 0 and "copy" not in str(gates_only)


def test_gates_alone_on_worst_case_poseidon_rows(c10):
    syn = c10.syn
    rg = cw.row_gates(syn)
    prow_at = [r for r in range(c10.n) if syn.gates[int(rg[r])].kind == cw.POSEIDON]
    _gate_rows, prows = qa.gate_aim_rows()
    assert len(prow_at) >= 64
    w = syn.wires.copy()
    for off in range(0, len(prows), len(prow_at)):         # every aim once, as many rows at a time as the circuit has
        for j, r in enumerate(prow_at):
            w[:, r] = np.array(prows[(off + j) % len(prows)][1], dtype=np.uint64)
        rep = c10.check(w, GATES)
        assert rep.ok and rep.gate_rows_bad == 0 and rep.checked == GATES, (off, str(rep))
    victim = prow_at[len(prow_at) // 2]
    w[70, victim] = (int(w[70, victim]) + 1) % P            # partial round 5's S-box input
    rep = c10.check(w, GATES)
    assert rep.gate_rows_bad == 1 and rep.gate_row == victim and rep.gate_kind == cw.POSEIDON and rep.gate_constraint == 41 + 5
    assert "PoseidonGate" in str(rep)


def test_lookups(orc, clk):
    syn = clk.syn
    last_lu, last_lut, first_lut = (int(x) for x in syn.lookup_rows[0])
    assert (last_lu, last_lut, first_lut) == (1, 4, 6)
    # a real slot's output, then its input
    rep = clk.check(cw.mutated(syn.wires, 1, 1))
    assert not rep.ok and rep.lookup_slots_bad == 1 and (rep.lookup_row, rep.lookup_slot, rep.lookup_table) == (1, 0, 0)
    assert rep.lookup_input == int(syn.wires[0, 1]) and rep.lookup_output == int(syn.wires[1, 1]) + 1
    assert "LookupGate" in str(rep)
    w = syn.wires.copy()
    w[0, 1] = 70000
    rep = clk.check(w, LOOKUPS)
    assert rep.checked == LOOKUPS and rep.lookup_slots_bad == 1 and (rep.lookup_row, rep.lookup_slot) == (1, 0) and rep.lookup_input == 70000
    # a table entry: entry 0 sits in slot 0 of row first_lut
    rep = clk.check(cw.mutated(syn.wires, 0, first_lut), LOOKUPS)
    assert rep.lookup_slots_bad == 1 and (rep.lookup_row, rep.lookup_slot) == (first_lut, 0) and "LookupTableGate" in str(rep)
    # junk where nlx_prove writes: a padding slot of the last LookupGate row (100 lookups = 2 rows of 40 and 20) and a multiplicity
    w = syn.wires.copy()
    w[2 * 30, last_lut - 1] = 12345
    w[2 * 30 + 1, last_lut - 1] = 54321
    w[2, first_lut] = 999
    rep = clk.check(w)
    assert rep.ok and rep.checked == ALL and rep.lookup_slots_bad == 0, str(rep)
    ref = orc.Circuit.from_synthetic(syn)
    try:
        assert ref.verify(clk.cd.prove(w, syn.public_inputs)) == 1
    finally:
        ref.close()


def test_arguments(nlx, c8):
    dll, syn, cd = nlx.lib.dll, c8.syn, c8.cd
    pis = np.ascontiguousarray(syn.public_inputs, dtype=np.uint64)
    rep = nlx.plonk.WitnessReport()
    rep.gate_rows_bad = 77
    for what in (0, 8):
        assert dll.nlx_circuit_check_witness(cd.handle, syn.wires.ctypes.data, pis.ctypes.data, what, ctypes.byref(rep)) == NLX_E_INVAL
        assert rep.gate_rows_bad == 0 and rep.checked == 0          # zero-filled before anything else
    assert dll.nlx_circuit_check_witness(cd.handle, syn.wires.ctypes.data, pis.ctypes.data, ALL, None) == NLX_E_INVAL
    assert dll.nlx_circuit_check_witness(cd.handle, None, pis.ctypes.data, ALL, ctypes.byref(rep)) == NLX_E_INVAL
    rep = cd.check_witness(syn.wires, syn.public_inputs, LOOKUPS)   # a circuit without tables: nothing to check
    assert rep.checked == 0 and rep.satisfied == 1
    assert cd.check_witness(syn.wires, syn.public_inputs, "gates+copies").checked == 3


def test_a_check_moves_no_proof_byte(c8):
    syn, cd = c8.syn, c8.cd
    before = cd.prove(syn.wires, syn.public_inputs)
    assert not cd.check_witness(cw.mutated(syn.wires, 0, 0), syn.public_inputs).ok
    assert cd.check_witness(syn.wires, syn.public_inputs).ok
    assert cd.prove(syn.wires, syn.public_inputs) == before
