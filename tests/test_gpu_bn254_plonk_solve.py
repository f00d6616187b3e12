"""GPU: gnark's witness solver on the device, by levels (nlx_bn254_plonk_solver_*; csrc/bn254_plonk_solve.hpp and .hip,
near-light-client_amd/bn254_plonk.py Setup.solver / Solver) against the sequential big-integer model
tools/gnark_plonk_solve_model.py on the circuits of tests/bn254_plonk_solve_cases.py, which
tests/test_gnark_plonk_solve_model_cpu.py pins to the frozen models.  Every comparison is exact.  Parity with gnark's solver
stays unpinned."""
import random

import numpy as np
import pytest

import bn254_plonk_check_model as check_model
import bn254_plonk_solve_cases as cases

pytestmark = pytest.mark.gpu

pm, R, bn = cases.pm, cases.R, cases.bn
E_INVAL, E_RANGE = -1, -4
ACCEPT = 0


def _words(nlx, values):
    return nlx.bn254_pack([[bn.to_montgomery(int(v) % R) for v in values]])[0]


@pytest.fixture(scope="module")
def made(nlx, ctx):
    """name -> (Setup, {fuse: Solver}, ResidentKey or None), made once"""
    P = nlx.bn254_plonk
    kept = {}

    def get(name):
        if name not in kept:
            c = cases.case(name)
            s = P.Setup(ctx, **c.args())
            key = s.key(P.kzg_srs(ctx, cases.trapdoor(name), c.n + 3)[0]) if c.k else None
            kept[name] = (s, {fuse: s.solver(fuse=fuse, **c.solver_args()) for fuse in (True, False)}, key)
        return kept[name]
    yield get
    for s, solvers, key in kept.values():
        for x in list(solvers.values()) + [key, s]:
            if x is not None:
                x.close()


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "no_fuse"])
@pytest.mark.parametrize("name", cases.ALL)
def test_values_equal_the_models_word_for_word(nlx, ctx, made, name, fuse):
    """fused: device inputs and values_out; NO_FUSE: host ones"""
    import torch
    c, m = cases.case(name), cases.model(name)
    s, solvers, key = made(name)
    want, points, cs = cases.solved(name)
    inputs = _words(nlx, c.inputs)
    if fuse:
        inputs = torch.from_numpy(inputs.view(np.int64)).to("cuda:0")
    cblind = cases.commit_blinding(name) if c.k else None
    values, rep = solvers[fuse].solve(inputs, key, cblind, device="cuda:0" if fuse else None)
    assert rep.solved == 1 and rep.kind == 0 and rep.failures == 0 and rep.poisoned_variables == 0 and bool(rep)
    got = values.cpu().numpy().view(np.uint64) if fuse else values
    assert np.array_equal(got, _words(nlx, want))
    assert rep.launches == cases.launches(m, fuse)[0] and rep.levels_run == max(m.level + m.hint_level)
    if c.k:
        assert np.array_equal(rep.commit_points, nlx.bn254_g1_pack(list(points)))      # k2chain: gnark_bsb22_model.solve's, by the CPU file
        assert [nlx.bn254_plonk._from_words_mont(got[v]) for v in c.c_var] == list(cs)


@pytest.mark.parametrize("name", cases.ALL)
def test_schedule_and_info_equal_the_models(nlx, made, name):
    c, m = cases.case(name), cases.model(name)
    _, solvers, _ = made(name)
    assert nlx.bn254_plonk.SOLVER_FUSE == cases.FUSE
    for fuse in (True, False):
        sv = solvers[fuse]
        assert sv.read("level").tolist() == m.level and sv.read("form").tolist() == m.form and sv.read("assigns").tolist() == m.assigns
        info = sv.info()
        width = {}
        for lv in [lv for lv, f in zip(m.level, m.form) if f != pm.SKIPPED] + m.hint_level:
            width[lv] = width.get(lv, 0) + 1
        launches, runs = cases.launches(m, fuse)
        solves = [i for i, f in enumerate(m.form) if f in (pm.SOLVE_L, pm.SOLVE_R, pm.SOLVE_O)]
        kinds = [h[0] for h in m.hints]
        assert info.pop("resident_bytes") >= 177 * sum(width.values())
        assert info == {"levels": max(width), "widest_level": max(width.values()), "launches": launches, "fused_runs": runs,
                        "checks": m.form.count(pm.CHECK), "solve_l": m.form.count(pm.SOLVE_L), "solve_r": m.form.count(pm.SOLVE_R),
                        "solve_o": m.form.count(pm.SOLVE_O), "inv_zero": kinds.count(pm.INV_ZERO), "n_bits": kinds.count(pm.N_BITS),
                        "quo_rem64": kinds.count(pm.QUO_REM64), "commits": c.k, "constant_divisors": sum(m.const_divisor(i) for i in solves),
                        "value_divisors": sum(not m.const_divisor(i) for i in solves), "unassigned": m.unassigned}


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "no_fuse"])
@pytest.mark.parametrize("which", ["two_divisors", "unsatisfied", "poisoned_check"])
def test_failing_inputs_give_the_models_failure(nlx, made, which, fuse):
    c, m = cases.case("ragged"), cases.model("ragged")
    _, solvers, _ = made("ragged")
    inputs, (kind, constraint), failures, poisoned = cases.failing(c)[which]
    want, first, want_failures, want_poisoned = m.solve(inputs, stop=False)
    assert first[:2] == (kind, constraint) and (want_failures, want_poisoned) == (failures, poisoned)
    values, rep = solvers[fuse].solve(inputs, device=None)
    assert not rep and rep.solved == 0
    assert (rep.kind, rep.constraint, rep.value_int) == first and rep.level == m.level[constraint]
    assert rep.kind_name == {pm.DIV_ZERO: "DIV_ZERO", pm.UNSATISFIED: "UNSATISFIED"}[kind]
    assert (rep.failures, rep.poisoned_variables) == (failures, poisoned)
    assert "constraint %d " % constraint in rep.message
    with pytest.raises(ValueError, match="constraint %d " % constraint):
        rep.raise_if_unsolved()
    assert np.array_equal(values, _words(nlx, [0 if v is None else v for v in want]))      # a poisoned variable comes as 0


@pytest.mark.parametrize("what,constraints,hints,where", cases.refusals(), ids=[r[0] for r in cases.refusals()])
def test_every_refusal_names_its_index_and_allocates_nothing(nlx, ctx, what, constraints, hints, where):
    P = nlx.bn254_plonk
    s = P.Setup(ctx, cases.REFUSAL_VARIABLES, 1, constraints, cases.REFUSAL_COEFFS)
    before = ctx.memory()[1]
    with pytest.raises(ValueError, match="%s %d" % where) as e:
        s.solver(1, hints)
    assert e.value.__cause__.code == E_INVAL and ctx.memory()[1] == before
    s.close()


def test_key_and_range_refusals(nlx, ctx, made):
    P = nlx.bn254_plonk
    c = cases.case("k2chain")
    s, solvers, key = made("k2chain")
    cblind = cases.commit_blinding("k2chain")
    with pytest.raises(ValueError) as e:
        solvers[True].solve(c.inputs, None, cblind)
    assert e.value.__cause__.code == E_INVAL and "key" in str(e.value)
    with pytest.raises(ValueError) as e:
        solvers[True].solve(c.inputs, key, None)
    assert e.value.__cause__.code == E_INVAL
    _, plain, _ = made("forms8")
    with pytest.raises(ValueError) as e:
        plain[True].solve(cases.case("forms8").inputs, key, None)
    assert e.value.__cause__.code == E_INVAL
    # an input that is not below r: r itself on variable 1, and 2^256 - 1
    c8 = cases.case("forms8")
    for bad in (R, (1 << 256) - 1):
        words = _words(nlx, c8.inputs)
        words[1] = [(bad >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
        before = ctx.memory()[1]
        with pytest.raises(nlx.NlxError) as e:
            plain[False].solve(words, device=None)
        assert e.value.code == E_RANGE and "input 1 " in str(e.value) and ctx.memory()[1] == before
    with pytest.raises(nlx.NlxError) as e:
        s.solver(c.n_variables)                                          # more inputs than variables
    assert e.value.code == E_RANGE


@pytest.mark.parametrize("name", ["k1_1000", "plain4096"])
def test_end_to_end_from_the_inputs(nlx, ctx, name):
    """kzg_srs -> setup -> key -> solver -> solve -> wires -> check_resident(ALL) -> prove_resident -> verify; the proof's bytes
    equal those from the model-solved vector under the same blinding"""
    P = nlx.bn254_plonk
    c = cases.case(name)
    rng = random.Random("e2e" + name)
    tau = cases.trapdoor(name)
    g1, g2, g2_tau = P.kzg_srs(ctx, tau, c.n + 3, device="cuda:0")
    key, s = P.setup(ctx, c.n_variables, c.n_public, c.constraints, c.coeffs, g1, commitments=c.sets)
    solver = s.solver(**c.solver_args())
    cblind = cases.commit_blinding(name) if c.k else None
    values, rep = solver.solve(c.inputs, key if c.k else None, cblind)
    rep.raise_if_unsolved()
    l, r, o = s.wires(values)
    pubs = c.public_inputs
    check = P.check_resident(key, l, r, o, pubs, cblind)
    assert check.satisfied == 1 and check.checked == (7 if c.k else 3), check.message
    blind = [rng.randrange(R) for _ in range(9)]
    proof = P.prove_resident(key, l, r, o, pubs, blind, cblind)
    vk = P.VerifyingKey.from_resident(key, g2, g2_tau, c.n_public)
    v = vk.verify(proof, pubs)
    assert (int(v.accepted), int(v.reason)) == (1, ACCEPT)
    ml, mr, mo = s.wires(list(cases.solved(name)[0]))
    assert proof == P.prove_resident(key, ml, mr, mo, pubs, blind, cblind)
    for x in (vk, solver, key, s):
        x.close()
