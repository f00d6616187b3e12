"""CPU tests of the witness checker's yardsticks (tests/check_witness_cases.py): what tests/test_gpu_check_witness.py expects of
nlx_circuit_check_witness is decided here, by the CPU oracle's prover and verifier, and needs no GPU."""
import numpy as np
import pytest

import check_witness_cases as cw
from conftest import P


@pytest.fixture(scope="module")
def syn8(nlx):
    return nlx.SyntheticCircuit(8, seed=21, **cw.ALL19)


@pytest.fixture(scope="module")
def ref8(orc, syn8):
    ref = orc.Circuit.from_synthetic(syn8)
    yield ref
    ref.close()


def test_sigma_decode_is_a_permutation(syn8):
    n = 1 << 8
    to_col, to_row = cw.sigma_cells(syn8)
    assert len(set(zip(to_col.ravel().tolist(), to_row.ravel().tolist()))) == cw.ROUTED * n
    cols, rows = np.meshgrid(np.arange(cw.ROUTED), np.arange(n), indexing="ij")
    moved = (to_col != cols) | (to_row != rows)
    assert int(moved.sum()) == 1438
    assert np.array_equal(syn8.wires[:cw.ROUTED], syn8.wires[to_col, to_row])    # sigma only links equal values
    rg = cw.row_gates(syn8)
    noop_rows = np.array([syn8.gates[int(g)].kind == cw.NOOP for g in rg])
    assert not moved[:, noop_rows].any()


def test_every_gate_kind_rejects_its_first_row_mutated(syn8, ref8):
    first = cw.first_rows_by_kind(syn8)
    assert sorted(first) == list(range(1, 19))            # the 18 gate kinds with constraints
    for kind, row in first.items():
        for wire in (0, 1):
            assert ref8.verify(ref8.prove(cw.mutated(syn8.wires, wire, row), syn8.public_inputs)) < 1, (kind, row, wire)


@pytest.mark.parametrize("key,unsat", [("8", 18), ("5", 15)])
def test_random_cells_against_the_oracle(nlx, orc, key, unsat):
    got = cw.oracle_verdicts(nlx, orc, key)
    assert sum(1 - v[3] for v in got) == unsat and len(got) == 40
    assert min(unsat, 40 - unsat) >= 10                    # a checker can neither always say "bad" nor always "fine"
    assert got == cw.golden_cells()[key]


def test_lookup_mutations(nlx, orc):
    syn = nlx.SyntheticCircuit(9, **cw.LOOKUP)
    assert syn.lookup_rows.tolist() == [[1, 4, 6]]
    ref = orc.Circuit.from_synthetic(syn)
    try:
        assert ref.verify(ref.prove(syn.wires, syn.public_inputs)) == 1
        assert ref.verify(ref.prove(cw.mutated(syn.wires, 1, 1), syn.public_inputs)) < 1
        w = syn.wires.copy()
        w[0, 1] = 70000
        with pytest.raises(ValueError):
            ref.set_lookup_wires(w)
    finally:
        ref.close()


def test_restatement_is_zero_on_the_witness_and_sees_mutations(orc, syn8):
    pih = orc.hash_no_pad(syn8.public_inputs)
    seen = set()
    for row in range(1 << 8):
        cs = cw.restate(syn8, syn8.wires, row, pih)
        if cs is not None:
            assert not any(cs), row
            seen.add(syn8.gates[int(cw.row_gates(syn8)[row])].kind)
    assert seen == set(cw.RESTATED)
    for kind in cw.RESTATED:                               # and wire 0 of each kind's first row is read by constraint 0
        row = cw.first_rows_by_kind(syn8)[kind]
        idx, val = cw.first_nonzero(cw.restate(syn8, cw.mutated(syn8.wires, 0, row), row, pih))
        assert idx == 0 and 0 < val < P
