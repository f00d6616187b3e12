"""CPU tests of the STARK trace checker's yardstick (tests/stark_check_cases.py): what tests/test_gpu_stark_check.py expects of
nlx_stark_check_trace / nlx_stark_check_rounds is decided here, by the oracle's prover and verifier, and needs no GPU."""
import numpy as np
import pytest

import stark_check_cases as sc
from conftest import P


@pytest.fixture(scope="module")
def S(nlx):
    return nlx.stark


@pytest.fixture(scope="module")
def fib4(S):
    st = S.Stark(S.fibonacci_air(), 4, S.StarkConfig(fri_num_queries=20))
    trace, pis = S.fibonacci_trace(4)
    return st, trace, pis


@pytest.fixture(scope="module")
def wide5(S):
    st = S.Stark(sc.free_wide_air(S), sc.CELLS_LOG_N, S.StarkConfig(fri_num_queries=20))
    trace, pis = sc.free_wide_trace(S, sc.CELLS_LOG_N)
    return st, trace, pis


def accepts(orc, st, trace, pis):
    return orc.stark_verify(st.desc, orc.stark_prove(st.desc, trace, pis)) == 1


def test_honest_single_round_traces(orc, fib4, wide5):
    for st, trace, pis in (fib4, wide5):
        rep = sc.check_stark(st, trace, pis)
        assert rep["satisfied"] == 1 and rep["rows_bad"] == 0 and rep["pairs_bad"] == 0 and not any(rep["per_constraint"])
        assert rep["n_constraints"] == st.air.num_constraints
        assert accepts(orc, st, trace, pis)


def test_honest_every_op_trace(orc, S):
    air = sc.every_op_air(S)
    st = S.Stark(air, sc.EO_LOG_N, S.StarkConfig(fri_num_queries=20))
    assert {int(w) & 0xFF for w in sc_words(st.program)} == set(range(22)), "every_op_air must use every opcode"
    assert sum(1 for w in sc_words(st.program) if int(w) & 0xFF == sc.SEGMENT) >= 2
    t0, pis = sc.every_op_round0()
    proof = orc.stark_prove_rounds(st.desc, sc.every_op_round_fn(t0), pis)
    assert orc.stark_verify(st.desc, proof) == 1
    values = orc.stark_values(st.desc, proof)                      # public inputs | alpha0, alpha1 | the round value
    assert len(values) == 2 + 2 + 1
    t1, rv = sc.every_op_round1(t0, values[2:4])
    assert rv == values[4:]
    rep = sc.check_stark(st, np.concatenate([t0, t1]), values)
    assert rep["satisfied"] == 1 and rep["n_constraints"] == air.num_constraints == 11 + 10 + 3 + 4 + 1
    # and for challenges of any other origin: a correct trace writer satisfies the constraints whatever they are
    t1b, rvb = sc.every_op_round1(t0, [5, 6])
    assert sc.check_stark(st, np.concatenate([t0, t1b]), list(pis) + [5, 6] + rvb)["satisfied"] == 1


def sc_words(program):
    """the instruction words: CONST immediates left out"""
    out, pc = [], 0
    while pc < len(program):
        out.append(program[pc])
        pc += 2 if int(program[pc]) & 0xFF == sc.CONST else 1
    return out


def test_fibonacci_wrap_pins_the_transition_predicate(fib4):
    st, trace, pis = fib4
    n = trace.shape[1]
    assert int(trace[0, 0]) != int(trace[1, n - 1])               # row n - 1 -> row 0 does not continue the sequence
    rep = sc.check_stark(st, trace, pis)
    assert rep["satisfied"] == 1
    # read as an every-row constraint it would fail exactly there
    table = sc.constraint_table(st.program)
    got = sc.run_program(st.program, trace[:, n - 1].tolist(), trace[:, 0].tolist(), [int(v) for v in pis])
    assert any(val and kind == sc.EMIT_TRANSITION for (_, val), (kind, _, _) in zip(got, table))


def test_mutated_cells_against_the_oracle(nlx, orc, wide5):
    st, trace, pis = wide5
    got = sc.oracle_cell_verdicts(nlx, orc)
    assert got == sc.golden_cells() and len(got) == sc.N_CELLS
    n_ok = sum(v[3] for v in got)
    assert min(n_ok, sc.N_CELLS - n_ok) >= 5                       # a checker can neither always say "bad" nor always "fine"
    for c, r, inc, verdict in got:
        rep = sc.check_stark(st, sc.mutated(trace, c, r, inc), pis)
        assert rep["satisfied"] == verdict, (c, r)
        assert (rep["pairs_bad"] == 0) == bool(verdict) and sum(rep["per_constraint"]) == rep["pairs_bad"]
        if not verdict:
            assert rep["row"] in ((r - 1) % (1 << sc.CELLS_LOG_N), r) and 0 < rep["value"] < P


def test_edge_cells(orc, S, fib4, wide5):
    st, trace, pis = wide5
    n = trace.shape[1]
    # the last row of a constrained column is read as `next` by row n - 2 (and as `local` only by constraints that are off there)
    bad = sc.mutated(trace, 0, n - 1)
    rep = sc.check_stark(st, bad, pis)
    assert (rep["satisfied"], rep["row"], rep["kind"]) == (0, n - 2, sc.EMIT_TRANSITION)
    assert not accepts(orc, st, bad, pis)
    # a wrong public input fails a first-row constraint at row 0
    for k in (0, 1):
        wrong = pis.copy()
        wrong[k] = (int(wrong[k]) + 1) % P
        rep = sc.check_stark(st, trace, wrong)
        assert (rep["satisfied"], rep["row"], rep["kind"], rep["rows_bad"], rep["pairs_bad"]) == (0, 0, sc.EMIT_FIRST, 1, 1)
        assert rep["constraint"] == st.air.num_constraints - 2 + k
        assert not accepts(orc, st, trace, wrong)
    # a wrong third Fibonacci input fails the last-row constraint at row n - 1
    st, trace, pis = fib4
    wrong = pis.copy()
    wrong[2] = (int(wrong[2]) + 1) % P
    rep = sc.check_stark(st, trace, wrong)
    assert (rep["satisfied"], rep["row"], rep["kind"], rep["constraint"], rep["value"]) == (0, trace.shape[1] - 1, sc.EMIT_LAST, 2, P - 1)
    assert not accepts(orc, st, trace, wrong)
