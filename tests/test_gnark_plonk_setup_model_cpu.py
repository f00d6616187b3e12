"""CPU: the big-integer model of gnark's plonk.Setup (tools/gnark_plonk_setup_model.py, the yardstick of nlx_bn254_plonk_setup;
DESIGN.md section 37) against rule 3's worked case, against its own invariants on every case of tests/bn254_plonk_setup_cases.py,
and against the frozen models: its values with a satisfying variable vector pass the witness checker's yardstick
(tests/bn254_plonk_check_model.py) and prove and verify through tools/gnark_bsb22_model.py.  And the Python side of the binding
before the library is called: the descriptor's ctypes layout equals the C struct's, through the host compiler."""
import ctypes
import os
import random
import subprocess

import pytest

import bn254_plonk_check_model as check_model
import bn254_plonk_setup_cases as cases
from conftest import ROOT

gm, bn, R, sm = check_model.gm, check_model.bn, check_model.R, cases.sm


def test_worked_case_of_rule_3():
    s = cases.worked_case()
    assert s.n == 8 and s.used == 3
    where = s.classes()
    assert where[1] == [1, 10] and where[2] == [9] and where[3] == [2, 17]
    assert where[0] == [p for p in range(24) if p not in (1, 10, 9, 2, 17)]
    for p, q in cases.WORKED_PERM.items():
        assert s.perm[p] == q, (p, s.perm[p], q)
    assert s.values["ql"][0] == R - 1 and not any(s.values["ql"][1:]) and s.cells[0][:3] == [0, 1, 3]


@pytest.mark.parametrize("name", cases.ALL)
def test_permutation_invariants(name):
    """perm is a permutation; its cycles are exactly the variables' position sets; perm[p] < p except at a class's first position"""
    c = cases.case(name)
    m = sm.Setup(c.n_variables, c.n_public, c.constraints, c.coeffs, c.k1, c.k2, c.sets, c.log_n, with_sigma=False) if c.variables is None else c.model()
    perm, n = m.perm, m.n
    assert sorted(perm) == list(range(3 * n))
    where = m.classes()
    assert sum(len(v) for v in where.values()) == 3 * n
    for positions in where.values():
        assert positions == sorted(positions)
        cycle, p = [], positions[0]
        for _ in positions:
            cycle.append(p)
            p = perm[p]
        assert p == positions[0] and sorted(cycle) == positions          # one cycle, the whole class
        assert perm[positions[0]] == positions[-1]
        assert all(perm[b] == a for a, b in zip(positions, positions[1:]))   # every later position points at its predecessor
    assert m.sigma_cells()[n + 1] == (perm[n + 1] // n) << 30 | perm[n + 1] % n


def test_case_shapes():
    """the cases are what their names promise"""
    c = cases.case("n8")
    assert c.n_public + len(c.constraints) == 8 == c.n
    assert cases.case("n8_nopub").n_public == 0 and len(cases.case("n8_nopub").constraints) == 8
    assert cases.case("n5").n_public + len(cases.case("n5").constraints) == 5
    c = cases.case("n32_k2")
    where = c.model().classes()
    assert c.k == 2 and c.sets[1]["constraint"] == len(c.constraints) - 1 and c.model().info[1]["row"] == c.model().info[1]["last_row"]
    assert any(len(p) == 1 for p in where.values())
    assert any(con[0] == con[1] == con[2] != 0 for con in c.constraints)
    where = cases.case("n256").model().classes()
    # variable 0: 440 constraint cells, 15 of padding and the public row's three (its L too: variable 0 is public input 0)
    assert sorted(len(p) for p in where.values())[-2:] == [300, 458]
    c = cases.case("n1000_k1")
    assert (c.n_public, c.k, c.n_public + len(c.constraints)) == (3, 1, 1000)
    assert cases.case("s16").n_variables > 1 << 16 and cases.case("s14").log_n == 14


@pytest.mark.parametrize("name", cases.SMALL + ("n1024",))
def test_model_values_pass_the_witness_checker(name):
    c = cases.case(name)
    m = c.model()
    inst = cases.AsInstance(c)
    rng = random.Random(7)
    tau = rng.randrange(1, R)
    cblind = [rng.randrange(R) for _ in range(2 * c.k)]
    (l, r, o), _, _, _, cs = gm.solve(inst, None, cblind, tau)
    assert (l, r, o) == m.wires(c.complete(cs))
    rep = check_model.check(m.values, l, r, o, c.public_inputs, cs, m.info, c.k1, c.k2)
    assert rep["satisfied"] == 1 and rep["checked"] == (7 if c.k else 3), rep
    # one cell changed: the copy the checker names is the model's permutation
    bad = [list(col) for col in (l, r, o)]
    p = next(p for p in range(3 * m.n) if m.perm[p] != p and p % m.n >= c.n_public)
    bad[p // m.n][p % m.n] = (bad[p // m.n][p % m.n] + 1) % R
    rep = check_model.check(m.values, bad[0], bad[1], bad[2], c.public_inputs, cs, m.info, c.k1, c.k2, what=check_model.CHECK_COPIES)
    assert rep["copy_cells_bad"] == 2
    first = min((q % m.n, q // m.n) for q in (p, m.perm.index(p)))
    at = first[1] * m.n + first[0]
    assert (rep["copy_row"], rep["copy_wire"]) == first and rep["copy_to_wire"] * m.n + rep["copy_to_row"] == m.perm[at]


def _with_one_commitment(name, log_n, n_public, gates, n_free, seed):
    c = cases.Circuit(name, log_n, n_public, seed)
    free = cases._random_gates(c, gates, n_free)
    c.close_commitment(c.commitment([free[1], free[0]]))
    return c


@pytest.mark.parametrize("name", ["n8", "n5", "n8_k1", "n32_k0", "n32_k1", "n32_k2"])
def test_model_values_prove_and_verify(name):
    """2^3 and 2^5, k = 0 and 1 each (and k = 2): the frozen prover takes the model's key and a verifier with the same key accepts"""
    if name == "n8_k1":
        c = _with_one_commitment(name, 3, 1, 3, 3, 81)
    elif name == "n32_k1":
        c = _with_one_commitment(name, 5, 2, 20, 8, 321)
    elif name == "n32_k0":
        c = cases._plain(5, 2, 320)
    else:
        c = cases.case(name)
    inst = cases.AsInstance(c)
    rng = random.Random(11)
    tau = rng.randrange(1, R)
    blind, cblind = [rng.randrange(R) for _ in range(9)], [rng.randrange(R) for _ in range(2 * c.k)]
    _, data = gm.prove(inst, None, blind, cblind, tau=tau)
    assert len(data) == gm.proof_length(c.k)
    vk = gm.verifying_key(inst, None, tau)
    assert gm.verify_trapdoor(data, vk, inst.n, tau, c.k1, c.k2, c.public_inputs)
    if c.n_public:
        assert not gm.verify_trapdoor(data, vk, inst.n, tau, c.k1, c.k2, [(c.public_inputs[0] + 1) % R] + c.public_inputs[1:])


def test_srs_rule():
    g1, g2, g2_tau = sm.kzg_srs(5, 3)
    assert g1 == [bn.G1, bn.g1_mul(5, bn.G1), bn.g1_mul(25, bn.G1)] and g2 == bn.G2 and g2_tau == bn.g2_mul(5, bn.G2)


def test_setup_desc_layout_equals_the_header(nlx, tmp_path):
    P = nlx.bn254_plonk
    fields = [name for name, _ in P._PlonkSetupDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlx.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(nlx_bn254_plonk_setup_desc, %s));\n' % f for f in fields)
                   + '    printf("%zu\\n", sizeof(nlx_bn254_plonk_setup_desc));\n'
                   + '    printf("%d %d %d %d %d\\n", NLX_PLONK_SETUP_S1, NLX_PLONK_SETUP_QCP0, NLX_PLONK_SETUP_CELLS, NLX_PLONK_SETUP_SIGMA_CELLS,'
                   + ' NLX_BN254_PLONK_SETUP_INFO_WORDS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # the header is C
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:-5] == [getattr(P._PlonkSetupDesc, f).offset for f in fields] + [ctypes.sizeof(P._PlonkSetupDesc)]
    A = P.SETUP_ARRAYS
    assert got[-5:] == [A["s1"], A["qcp0"], A["cells"], A["sigma_cells"], P.SETUP_INFO_WORDS]


def test_shapes_the_binding_refuses(nlx):
    P = nlx.bn254_plonk
    with pytest.raises(ValueError, match="32-bit"):
        P.Setup(None, 2, 1, [(0, 0, -1, 0, 0, 0, 0, 0)], [0])
    with pytest.raises(ValueError):
        P.Setup(None, 2, 1, [(0, 0, 0, 0, 0, 0, 0)], [0])                # seven entries: no (m, 8) shape
    with pytest.raises(ValueError, match="four words"):
        P.Setup(None, 2, 1, [(0, 0, 0, 0, 0, 0, 0, 0)], [1 << 256])
    assert sum(int(w) << (64 * i) for i, w in enumerate(P._element_words(R))) == R   # not a residue: as it is, for the library to refuse
