"""The witness checker on gate evaluators that hand over LOOSE constraint values (csrc/prover_kernels.hip eval_gate: a satisfied
constraint may arrive as p instead of 0): a satisfying all-gate witness at 2^9 rows is still clean, and a broken one still
names the same row, gate and constraint - the cases and the exact restatement of tests/check_witness_cases.py."""
import numpy as np
import pytest

import check_witness_cases as cw
from conftest import P

pytestmark = pytest.mark.gpu

GATES, ALL = 1, 7


@pytest.fixture(scope="module")
def c9(nlx, ctx):
    syn = nlx.SyntheticCircuit(9, seed=21, **cw.ALL19)
    cd = nlx.CircuitData.from_synthetic(ctx, syn)
    yield syn, cd
    cd.close()


def test_a_satisfying_all_gate_witness_is_clean(c9):
    import torch
    syn, cd = c9
    assert len(cw.first_rows_by_kind(syn)) == 18            # every gate kind but the no-op is on some row
    for wires in (syn.wires, torch.from_numpy(syn.wires.view(np.int64)).cuda()):
        for what in (ALL, GATES):
            rep = cd.check_witness(wires, syn.public_inputs, what)
            assert rep.ok and rep.satisfied == 1 and (rep.gate_rows_bad, rep.copy_cells_bad, rep.lookup_slots_bad) == (0, 0, 0), str(rep)


def test_a_broken_witness_names_the_same_row_gate_and_constraint(orc, c9):
    syn, cd = c9
    pih = orc.hash_no_pad(syn.public_inputs)
    for kind, row in cw.first_rows_by_kind(syn).items():
        w = cw.mutated(syn.wires, 0, row)
        rep = cd.check_witness(w, syn.public_inputs, GATES)
        assert not rep.ok and rep.gate_rows_bad == 1 and rep.gate_row == row and rep.gate_kind == kind, (kind, row, str(rep))
        assert syn.gates[rep.gate_index].kind == kind
        assert 0 < rep.gate_value < P
        if kind in cw.RESTATED:
            assert (rep.gate_constraint, rep.gate_value) == cw.first_nonzero(cw.restate(syn, w, row, pih)), (kind, str(rep))

