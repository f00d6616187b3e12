"""CPU tests: the sequential witness solver tools/gnark_plonk_solve_model.py - the yardstick of nlx_bn254_plonk_solver_* - against
the frozen models, on the circuits of tests/bn254_plonk_solve_cases.py: its vector satisfies the witness checker's model
(gates and copies) through gnark_plonk_setup_model.Setup.wires and, with commitments, gnark_bsb22_model's prover and trapdoor
verifier; the levels respect the dependencies; every refusal names its index; the failing inputs stop where the cases say."""
import random

import pytest

import bn254_plonk_check_model as check_model
import bn254_plonk_setup_cases as setup_cases
import bn254_plonk_solve_cases as cases

pm, R, gm, bn = cases.pm, cases.R, check_model.gm, check_model.bn


@pytest.mark.parametrize("name", cases.ALL)
def test_the_vector_satisfies_gates_and_copies(name):
    c = cases.case(name)
    values, _, cs = cases.solved(name)
    assert list(values[:c.n_public + c.n_secret]) == [x % R for x in c.inputs]
    m = c.model()
    l, r, o = m.wires(values)
    rep = check_model.check(m.values, l, r, o, c.public_inputs, list(cs) if c.k else None, m.info, c.k1, c.k2,
                            what=check_model.CHECK_GATES | check_model.CHECK_COPIES)
    assert rep["satisfied"] == 1, rep


@pytest.mark.parametrize("name", ["k2chain", "k1_1000"])
def test_with_commitments_the_bsb22_prover_and_verifier_accept(name):
    c = cases.case(name)
    values, points, cs = cases.solved(name)
    done = setup_cases.Circuit.__new__(setup_cases.Circuit)      # the same circuit, carrying the solved vector
    done.__dict__.update(c.__dict__)
    done.variables = list(values)
    inst = setup_cases.AsInstance(done)
    tau, cblind = cases.trapdoor(name), cases.commit_blinding(name)
    _, _, _, want_points, want_cs = gm.solve(inst, None, cblind, tau)
    assert list(cs) == want_cs and list(points) == want_points
    rng = random.Random(name)
    proof, data = gm.prove(inst, None, [rng.randrange(R) for _ in range(9)], cblind, tau)
    assert gm.verify_trapdoor(data, gm.verifying_key(inst, None, tau), inst.n, tau, c.k1, c.k2, c.public_inputs)


@pytest.mark.parametrize("name", cases.ALL)
def test_levels_respect_dependencies(name):
    c, m = cases.case(name), cases.model(name)
    assigner = {v: 0 for v in range(c.n_public + c.n_secret)}
    for i, (form, lv, v) in enumerate(zip(m.form, m.level, m.assigns)):
        if form in (pm.SOLVE_L, pm.SOLVE_R, pm.SOLVE_O):
            assert v not in assigner and c.constraints[i][form - pm.SOLVE_L] == v
            assigner[v] = lv
    for (kind, before, ins, outs, _), lv in zip(m.hints, m.hint_level):
        for v in outs:
            assert v not in assigner
            assigner[v] = lv
    for i, con in enumerate(c.constraints):
        if m.form[i] == pm.SKIPPED:
            assert m.level[i] == 0 and m.assigns[i] == pm.NONE
            continue
        ops = [v for col, (v, counts) in enumerate(zip(con[:3], pm.counting(m.q[i]))) if counts and v != m.assigns[i]]
        assert m.level[i] == 1 + max([assigner[v] for v in ops] + [0])
    for (kind, before, ins, outs, _), lv in zip(m.hints, m.hint_level):
        assert lv == 1 + max(assigner[v] for v in ins)
    lv = m.levels()
    assert lv["constraints"] == m.level and len(lv["hints"]) == len(c.hints) and len(lv["commits"]) == c.k
    assert m.unassigned == c.n_variables - len(assigner)


def test_the_shapes_are_the_ones_the_cases_promise():
    m = cases.model("ragged")
    width = {}
    for form, lv in zip(m.form, m.level):
        width[lv] = width.get(lv, 0) + 1
    assert tuple(width[lv] for lv in sorted(width)) == cases.RAGGED_WIDTHS
    assert cases.launches(m) == (4, 2) and cases.launches(m, fuse=False) == (11, 0)
    m = cases.model("chain300")
    assert max(m.level) == 300 and cases.launches(m) == (1, 1)
    m = cases.model("forms8")
    assert m.form == [pm.SOLVE_O, pm.SOLVE_O, pm.SOLVE_L, pm.SOLVE_L, pm.SOLVE_R, pm.CHECK]
    assert [m.const_divisor(i) for i in range(5)] == [True, True, True, False, False]
    c, m = cases.case("k2chain"), cases.model("k2chain")
    assert m.form[-1] == pm.SKIPPED and c.sets[1]["constraint"] == len(c.constraints) - 1
    assert c.c_var[0] in m.hints[-1][2] and m.hint_level[-1] > m.hint_level[-2]
    kinds = [h[0] for h in cases.model("hints").hints]
    assert (kinds.count(pm.N_BITS), kinds.count(pm.QUO_REM64), kinds.count(pm.INV_ZERO)) == (16, 15, 3)


def test_hints_compute_what_rule_5_says():
    c = cases.case("hints")
    values, _, _ = cases.solved("hints")
    for kind, before, x, *rest in c.hints:
        xv = values[x]
        if kind == "n_bits":
            assert [values[v] for v in rest[0]] == [(xv >> i) & 1 for i in range(len(rest[0]))]
        elif kind == "quo_rem64":
            m, q, rem = rest
            assert values[q] * m + values[rem] == xv and 0 <= values[rem] < m
        else:
            assert values[rest[0]] * xv % R == (1 if xv else 0) and (xv or values[rest[0]] == 0)


@pytest.mark.parametrize("what,constraints,hints,where", cases.refusals(), ids=[r[0] for r in cases.refusals()])
def test_every_refusal_names_its_index(what, constraints, hints, where):
    with pytest.raises(pm.ScheduleError) as e:
        pm.Solver(cases.REFUSAL_VARIABLES, 1, 1, constraints, cases.REFUSAL_COEFFS, (), hints)
    assert e.value.where == where and ("%s %d" % where) in str(e.value)


@pytest.mark.parametrize("name", ["two_divisors", "unsatisfied", "poisoned_check"])
def test_failing_inputs_stop_where_stated(name):
    c, m = cases.case("ragged"), cases.model("ragged")
    inputs, (kind, constraint), failures, poisoned = cases.failing(c)[name]
    _, first = m.solve(inputs)
    assert first[:2] == (kind, constraint)
    vals, first2, got_failures, got_poisoned = m.solve(inputs, stop=False)
    assert first2 == first and (got_failures, got_poisoned) == (failures, poisoned)
    assert sum(v is None for v in vals) == poisoned
    if name == "two_divisors":
        other = c.special["div2"]
        assert constraint < other and m.level[constraint] == 7 and m.level[other] == 2
    if name == "poisoned_check":
        assert m.form[c.special["downstream"]] == pm.CHECK and m.level[c.special["downstream"]] == 3
    if name == "unsatisfied":
        assert first[2] == R - 1 or first[2] == 1
