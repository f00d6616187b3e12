"""CPU: the yardstick of the BN254 PLONK witness checker (tests/bn254_plonk_check_model.py) pinned against
the frozen models at log_n 3 .. 6 - oracle/bn254_py.py's plonk_witness and tools/gnark_bsb22_model.py's Instance, grand product
and gate identity - and tests/golden/bn254_plonk_check_cells.json pinned against the yardstick."""
import random

import pytest

import bn254_plonk_check_model as model

gm, bn, R = model.gm, model.bn, model.R
SHAPES = [(0, 0), (0, 3), (1, 2), (2, 2)]   # (k, n_pi)


@pytest.fixture(scope="module")
def cases():
    return {(log_n, k, n_pi): model.Case(log_n, k, n_pi) for log_n in (3, 4, 5, 6) for k, n_pi in SHAPES}


def _closes(case, wires):
    """the model's own grand product (tools/gnark_bsb22_model.py: it asserts that the product returns to 1)"""
    try:
        gm.grand_product(wires[0], wires[1], wires[2], case.values, case.n, 11, 13, case.k1, case.k2)
        return True
    except AssertionError:
        return False


def _row_sums(case, wires, cblind=None):
    """rule 1 of tools/gnark_bsb22_model.py on H, written as the quotient writes it: ql l + qr r + qm l r + qo o + qk + PI +
    sum_j qcp_j pi2_j, with pi2_j from the model's pi2_values"""
    v, n = case.values, case.n
    pi = list(case.pubs) + [0] * (n - len(case.pubs))
    cblind = case.cblind if cblind is None else cblind
    pi2 = []
    for j, c in enumerate(case.c_values(wires[0], cblind)):
        pi[case.info[j]["row"]] = c
        pi2.append(gm.pi2_values(case.inst, j, wires[0], cblind[2 * j], cblind[2 * j + 1]))
    out = []
    for i in range(n):
        l, r, o = (wires[c][i] for c in range(3))
        s = v["ql"][i] * l + v["qr"][i] * r + v["qm"][i] * l * r + v["qo"][i] * o + v["qk"][i] + pi[i]
        out.append((s + sum(v["qcp%d" % j][i] * pi2[j][i] for j in range(case.k))) % R)
    return out


@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_satisfying_witnesses_are_satisfied(cases, log_n, k, n_pi):
    case = cases[log_n, k, n_pi]
    rep = case.check()
    assert rep["satisfied"] == 1 and rep["checked"] == (7 if k else 3)
    assert all(rep[f] == 0 for f in model.FIELDS if f not in ("checked", "satisfied"))
    assert _closes(case, case.wires) and not any(_row_sums(case, case.wires))
    # without COMMITS the k commitment rows are left out
    rep = case.check(what=3)
    assert rep["satisfied"] == 1 and rep["checked"] == 3 and rep["gate_rows_skipped"] == k


@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_decode_is_the_generators_permutation(cases, log_n, k, n_pi):
    case = cases[log_n, k, n_pi]
    n = case.n
    cells = model.decode_sigma(case.values, case.k1, case.k2)
    assert sorted(t for col in cells for t in col) == [(c, i) for c in range(3) for i in range(n)]
    # the generators build one cycle per variable (Instance) / per value (plonk_witness): following sigma from a cell visits
    # exactly the cells that hold what it holds
    label = case.inst.cells if case.inst else case.wires
    classes = {}
    for c in range(3):
        for i in range(n):
            classes.setdefault(label[c][i], set()).add((c, i))
    for c in range(3):
        for i in range(n):
            seen, at = set(), (c, i)
            while at not in seen:
                seen.add(at)
                at = cells[at[0]][at[1]]
            assert at == (c, i) and seen == classes[label[c][i]]


@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_single_cell_mutations_against_the_models_own_machinery(cases, log_n, k, n_pi):
    case = cases[log_n, k, n_pi]
    for cell in model.mutations(case, 8, 900 + log_n):
        wires = model.mutated(case, cell)
        rep = case.check(wires)
        assert rep["satisfied"] == 0
        assert _closes(case, wires) == (rep["copy_cells_bad"] == 0)
        sums = _row_sums(case, wires)
        assert sum(1 for s in sums if s) == rep["gate_rows_bad"]
        if rep["gate_rows_bad"]:
            assert sums[rep["gate_row"]] == rep["gate_value"] != 0 and not any(sums[:rep["gate_row"]])
        if rep["copy_cells_bad"]:
            assert rep["copy_cells_bad"] >= 2 and (rep["copy_row"], rep["copy_wire"]) <= (cell[1], cell[0])
            assert rep["copy_value"] != rep["copy_to_value"]


@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_aimed_cells_break_one_kind_only(cases, log_n, k, n_pi):
    case = cases[log_n, k, n_pi]
    c, i = case.gate_only
    wires = model.mutated(case, (c, i, (case.wires[c][i] + 1) % R))
    rep = case.check(wires)
    assert (rep["gate_rows_bad"], rep["gate_row"], rep["copy_cells_bad"], rep["commits_bad"]) == (1, i, 0, 0)
    assert _closes(case, wires) and _row_sums(case, wires)[i] == rep["gate_value"] != 0
    c, i = case.copy_only
    wires = model.mutated(case, (c, i, case.wires[0][0] if case.wires[0][0] != case.wires[c][i] else 1))   # a value at home elsewhere
    rep = case.check(wires)
    assert rep["gate_rows_bad"] == 0 and rep["copy_cells_bad"] == 2 and rep["commits_bad"] == 0
    assert not _closes(case, wires) and not any(_row_sums(case, wires))


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_the_frozen_models_unsatisfied_witness_is_rejected(log_n):
    p = bn.plonk_witness(log_n, random.Random(60 + log_n), 5, 25, 11, 13, satisfied=False)
    rep = model.check(p, p["l"], p["r"], p["o"])
    assert rep["satisfied"] == 0 and rep["gate_rows_bad"] == 1 and rep["checked"] == 3


def test_first_means_lowest():
    case = model.Case(5, 0, 0)
    wires = [list(c) for c in case.wires]
    wires[2][20] = (wires[2][20] + 1) % R
    wires[1][7] = (wires[1][7] + 1) % R
    rep = case.check(wires)
    assert rep["gate_rows_bad"] == 2 and rep["gate_row"] == 7
    # the bad cells are each changed cell that has a partner and the cell sigma sends to it
    cells = model.decode_sigma(case.values, case.k1, case.k2)
    bad = set()
    for cell in ((1, 7), (2, 20)):
        if cells[cell[0]][cell[1]] != cell:
            bad |= {cell} | {(c, i) for c in range(3) for i in range(case.n) if cells[c][i] == cell}
    assert rep["copy_cells_bad"] == len(bad) and (rep["copy_row"], rep["copy_wire"]) == min((i, c) for c, i in bad)


def test_golden_file_is_the_yardsticks():
    got = model.load_golden()
    assert len(got) == 40 and {g["log_n"] for g in got} == {5, 8}
    assert got == model.golden_records()
    assert all(g["report"]["satisfied"] == 0 for g in got)
