"""GPU tests of the plonky2 verifier (nlx_verify, nlx_verify_batch): honest proofs of every code path are accepted, every named
tamper is rejected for the reason the oracle's sequential verifier gives and at the place the tamper sits, unsatisfied statements
fail the vanishing identity, and a batch gives each proof the verdict it gets alone.  The proofs under test are the ORACLE
prover's (and the GPU prover's on top); the oracle's verifier (orc_verify) is the reference for every verdict."""
import importlib

import numpy as np
import pytest

import check_witness_cases as cw
from conftest import P
from plonk_verify_cases import (ALL_CASES, CONSTRAINTS, FINAL_POLY, FRI_FOLD, FRI_PATH, MALFORMED, POW, PUBLIC_INPUTS, REASON_OF_ORACLE,
                                TRACE_PATH, case, flip, path_length_bytes, word_at)

pytestmark = pytest.mark.gpu

_circuits = {}


def circuit(nlx, ctx, orc, name):
    """the case's resident circuit (prover and verifier), built once a session"""
    if name not in _circuits:
        _circuits[name] = nlx.CircuitData.from_synthetic(ctx, case(nlx, orc, name).syn)
    return _circuits[name]


@pytest.mark.parametrize("name", ALL_CASES)
def test_honest_proofs_are_accepted(nlx, ctx, orc, name):
    c, cd = case(nlx, orc, name), circuit(nlx, ctx, orc, name)
    assert c.ref.verify(c.proof) == 1
    vd = cd.verifier_data()
    assert len(c.proof) == vd.proof_bytes == nlx.plonk.proof_layout(cd)["total"]
    v = cd.verify(c.proof)
    assert v.ok and v.reason == 0 and v.reason_name == "accept", str(v)
    v.raise_if_rejected()
    if name == "rows6-one-selector":
        assert c.syn.num_selectors == 1          # the filter without the UNUSED factor
    else:
        assert c.syn.num_selectors > 1
    # the prover the verifier ships with
    got = cd.prove(c.syn.wires, c.syn.public_inputs)
    assert cd.verify(got).ok
    # a verifier made from the verifying key alone gives the same verdicts
    key = nlx.VerifierData(ctx, c.syn.desc(), c.ref.constants_sigmas_cap(), c.ref.digest())
    try:
        assert key.proof_bytes == len(c.proof)
        bad = flip(c.proof, nlx.plonk.proof_layout(key)["wires"][0] + 5)
        assert bytes(key.verify(c.proof)) == bytes(v)
        assert bytes(key.verify(bad)) == bytes(cd.verify(bad)) and not key.verify(bad).ok
    finally:
        key.close()


def test_verifier_create_checks_the_digest(nlx, ctx, orc):
    c = case(nlx, orc, "rows5")
    d = c.syn.desc()
    dig = np.array(c.ref.digest(), dtype=np.uint64)
    for i in range(4):
        d.circuit_digest[i] = int(dig[i])
    nlx.VerifierData(ctx, d, c.ref.constants_sigmas_cap(), dig).close()     # a matching non-zero digest is fine
    d.circuit_digest[2] ^= 1
    with pytest.raises(nlx.NlxError) as e:
        nlx.VerifierData(ctx, d, c.ref.constants_sigmas_cap(), dig)
    assert e.value.code == -1
    # another digest is another circuit: its transcript differs from the first challenge on
    wrong = dig.copy()
    wrong[0] = (int(wrong[0]) + 1) % P
    key = nlx.VerifierData(ctx, c.syn.desc(), c.ref.constants_sigmas_cap(), wrong)
    v = key.verify(c.proof)
    assert not v.ok and v.reason == CONSTRAINTS
    key.close()


def test_unsatisfied_statements_one_per_gate_kind(nlx, ctx, orc):
    """wire 0 of the first row of every gate kind raised by one (tests/check_witness_cases.py), proved by the GPU prover, which
    writes a proof of an unsatisfied witness under the Goldilocks config"""
    c, cd = case(nlx, orc, "all-gates"), circuit(nlx, ctx, orc, "all-gates")
    first = cw.first_rows_by_kind(c.syn)
    assert len(first) == 18 and set(first) == set(range(1, 19))
    proofs = [cd.prove(cw.mutated(c.syn.wires, 0, row), c.syn.public_inputs) for _, row in sorted(first.items())]
    for (kind, row), bad, v in zip(sorted(first.items()), proofs, cd.verify_many(proofs)):
        assert c.ref.verify(bad) == -2, (kind, row)
        assert not v.ok and v.reason == CONSTRAINTS and v.challenge in (0, 1), (kind, row, str(v))


def test_unsatisfied_copy_and_lookup(nlx, ctx, orc):
    # one broken copy constraint
    c, cd = case(nlx, orc, "all-gates"), circuit(nlx, ctx, orc, "all-gates")
    to_col, to_row = cw.sigma_cells(c.syn)
    col, row = next((j, i) for i in range(1 << c.syn.log_n) for j in range(cw.ROUTED) if (to_col[j, i], to_row[j, i]) != (j, i))
    bad = cd.prove(cw.mutated(c.syn.wires, col, row), c.syn.public_inputs)
    assert c.ref.verify(bad) == -2
    v = cd.verify(bad)
    assert not v.ok and v.reason == CONSTRAINTS and v.challenge in (0, 1)
    # The lookup argument.  The prover writes the multiplicity wires itself (set_lookup_wires), so a wrong multiplicity cannot be
    # handed to it; what can is the other side of the same count: a looked-up output that its table does not pair with the input
    # (the multiplicities then count a pair that is not looked up), and a table entry that is not the descriptor's.
    c, cd = case(nlx, orc, "lookup-1-table"), circuit(nlx, ctx, orc, "lookup-1-table")
    last_lu, _last_lut, first_lut = (int(x) for x in c.syn.lookup_rows[0])
    for col, row in ((1, last_lu), (0, first_lut)):
        bad = cd.prove(cw.mutated(c.syn.wires, col, row), c.syn.public_inputs)
        assert c.ref.verify(bad) == -2, (col, row)
        v = cd.verify(bad)
        assert not v.ok and v.reason == CONSTRAINTS and v.challenge in (0, 1), (col, row, str(v))


def _tampers(proof, lay, d, lookups):
    """[(name, tampered proof, query or None, tree or None, layer or None)] - one bit each, placed with the layout"""
    q_last = len(lay["query"]) - 1
    out = [("%s cap" % n, flip(proof, lay["cap"][i][0] + 9 + 32 * i), None, None, None) for i, n in enumerate(("wires", "zs", "quotient"))]
    classes = ["constants", "sigmas", "wires", "zs", "zs_next", "partial_products", "quotient"] + (["lookup_zs", "lookup_zs_next"] if lookups else [])
    for k, name in enumerate(classes):
        assert lay[name][1] >= 16
        out.append(("%s opening" % name, flip(proof, lay[name][0] + lay[name][1] - 16 + k % 8, k % 5), None, None, None))
    out += [
        ("FRI commit cap", flip(proof, lay["fri_cap"][0][0] + 3), None, None, None),
        ("final polynomial", flip(proof, lay["final_poly"][0] + 16, 3), None, None, None),
        ("witness", flip(proof, lay["pow_witness"][0], 5), None, None, None),
        ("public input", flip(proof, lay["public_inputs"][0] + 8, 1), None, None, None),
        ("count word", flip(proof, lay["num_public_inputs"][0], 2), None, None, None),
        ("cut by 8", proof[:-8], None, None, None),
        ("extended by 8", proof + b"\0" * 8, None, None, None),
    ]
    for q in (0, q_last):
        Q = lay["query"][q]
        for t in range(4):
            out.append(("query %d row of tree %d" % (q, t), flip(proof, Q["row"][t][0] + 8 * (lay["tree_cols"][t] - 1) + 2), q, t, None))
        out.append(("query %d sibling of tree 0" % q, flip(proof, Q["path"][0][0] + 32 + 5, 7), q, 0, None))
        out.append(("query %d sibling of tree 3" % q, flip(proof, Q["path"][3][0] + Q["path"][3][1] - 1), q, 3, None))
        out.append(("query %d path-length byte of tree 2" % q, flip(proof, Q["path_len"][2][0]), q, 2, None))
        out.append(("query %d path-length byte of layer 0" % q, flip(proof, Q["layer"][0]["path_len"][0], 1), q, None, 0))
        out.append(("query %d layer sibling" % q, flip(proof, Q["layer"][0]["path"][0] + 7), q, None, 0))
    return out


@pytest.fixture(scope="module", params=["all-gates", "lookup-1-table"])
def tamper_target(request, nlx, ctx, orc):
    c, cd = case(nlx, orc, request.param), circuit(nlx, ctx, orc, request.param)
    assert cd.verify(c.proof).ok
    return c, cd, c.proof, nlx.plonk.proof_layout(cd)


def test_named_tampers(nlx, orc, tamper_target):
    c, cd, proof, lay = tamper_target
    tampers = _tampers(proof, lay, c.syn.desc(), c.syn.num_luts > 0)
    verdicts = cd.verify_many([t[1] for t in tampers])
    alone = {i: cd.verify(tampers[i][1]) for i in (0, 5, 12, len(tampers) - 1, len(tampers) - 3)}
    seen = set()
    for i, ((name, bad, q, tree, layer), v) in enumerate(zip(tampers, verdicts)):
        rc = c.ref.verify(bad)
        assert rc != 1 and not v.ok, name
        assert v.reason == REASON_OF_ORACLE[rc], (name, rc, str(v))
        seen.add(v.reason)
        if q is not None:
            assert v.query == q, (name, str(v))
        if tree is not None:
            assert v.tree == tree, (name, str(v))
        if layer is not None:
            assert v.layer == layer, (name, str(v))
        if i in alone:   # the single call agrees with the batch
            assert bytes(alone[i]) == bytes(v), name
    assert {MALFORMED, CONSTRAINTS, POW, TRACE_PATH, FRI_PATH} <= seen
    with pytest.raises(ValueError):
        verdicts[0].raise_if_rejected()
    assert "query" in verdicts[0].message and "tree" in verdicts[0].message and "layer" in verdicts[0].message


def test_word_alias_is_malformed(nlx, ctx, orc):
    """a word replaced by itself + p - the same field element, another word: malformed by the rule (the oracle's verifier does not
    look).  Only a value below 2^32 - 1 has such an alias in 64 bits, so the statement's public inputs are chosen small."""
    cd = circuit(nlx, ctx, orc, "rows5")
    syn = nlx.SyntheticCircuit(5, seed=1)              # the circuit of "rows5" again, with a witness of its own
    syn.set_public_inputs([5, 6, 7, 2 ** 32 - 2])
    ref = orc.Circuit.from_synthetic(syn)
    proof = ref.prove(syn.wires, syn.public_inputs)
    ref.close()
    assert cd.verify(proof, [5, 6, 7, 2 ** 32 - 2]).ok
    lay = nlx.plonk.proof_layout(cd)
    for k in (0, 3):
        at = lay["public_inputs"][0] + 8 * k
        w = int.from_bytes(proof[at:at + 8], "little")
        assert w == (5, 6, 7, 2 ** 32 - 2)[k] and w + P < 1 << 64
        v = cd.verify(proof[:at] + (w + P).to_bytes(8, "little") + proof[at + 8:])
        assert not v.ok and v.reason == MALFORMED, (k, str(v))


def test_layer_evaluations(nlx, orc, tamper_target):
    """layer 0's evaluation at the query's own position (the fold check) and at another one (the layer's path), for query 0 and
    the last: the position within the coset is x_index mod arity, which the verdict of a path tamper on the same query gives"""
    c, cd, proof, lay = tamper_target
    for q in (0, len(lay["query"]) - 1):
        Q = lay["query"][q]
        x_index = cd.verify(flip(proof, Q["path"][0][0])).x_index
        within = x_index % lay["arity"]
        own = flip(proof, Q["layer"][0]["evals"][0] + 16 * within + 4)
        other = flip(proof, Q["layer"][0]["evals"][0] + 16 * ((within + 1) % lay["arity"]) + 9)
        for bad, want in ((own, FRI_FOLD), (other, FRI_PATH)):
            rc = c.ref.verify(bad)
            v = cd.verify(bad)
            assert rc in (-7, -8) and REASON_OF_ORACLE[rc] == want == v.reason, (q, rc, str(v))
            assert (v.query, v.layer, v.x_index) == (q, 0, x_index)


def test_final_polynomial(nlx, ctx, orc):
    """No tamper of a default-config proof reaches the final polynomial's check: the proof of work or a path fails first.  With
    one query and no proof of work a flipped coefficient redraws the one query index out of 2^8, and the flips that leave it as it
    was - about 4096 / 256 - fail nowhere but there.  Found with the oracle; flips that lift a word to p or above are malformed by
    the rule and left out."""
    c, cd = case(nlx, orc, "rows5-one-query"), circuit(nlx, ctx, orc, "rows5-one-query")
    lay = nlx.plonk.proof_layout(cd)
    at, ln = lay["final_poly"]
    assert ln == 16 * 32 and lay["n_layers"] == 0
    found = []
    for byte in range(ln):
        for bit in range(8):
            bad = flip(c.proof, at + byte, bit)
            w0 = at + byte - byte % 8
            if c.ref.verify(bad) == -9 and int.from_bytes(bad[w0:w0 + 8], "little") < P:
                found.append(bad)
    assert found, "no flip of the final polynomial keeps the query index"
    for v in cd.verify_many(found):
        assert not v.ok and v.reason == FINAL_POLY and v.query == 0, str(v)


def test_public_inputs_argument(nlx, orc, tamper_target):
    c, cd, proof, lay = tamper_target
    assert cd.verify(proof, c.pis).ok
    wrong = list(c.pis)
    wrong[-1] = (wrong[-1] + 1) % P
    v = cd.verify(proof, wrong)
    assert not v.ok and v.reason == PUBLIC_INPUTS and v.reason_name == "public inputs"
    with pytest.raises(nlx.NlxError) as e:   # NLX_E_RANGE: not canonical
        cd.verify(proof, [P] + wrong[1:])
    assert e.value.code == -4
    vs = cd.verify_many([proof, proof], [c.pis, wrong])
    assert vs[0].ok and vs[1].reason == PUBLIC_INPUTS


def test_batch_of_65(nlx, ctx, orc):
    """more than a wave of proofs, three of them tampered in three different ways"""
    c, cd = case(nlx, orc, "rows5"), circuit(nlx, ctx, orc, "rows5")
    proof = c.proof
    lay = nlx.plonk.proof_layout(cd)
    bad = {2: flip(proof, lay["wires"][0] + 3),
           37: flip(proof, lay["query"][11]["row"][1][0] + 1),
           64: flip(proof, lay["query"][27]["path_len"][0][0])}
    proofs = [bad.get(i, proof) for i in range(65)]
    verdicts = cd.verify_many(proofs)
    assert [i for i, v in enumerate(verdicts) if not v.ok] == [2, 37, 64]
    for i, b in bad.items():
        alone = cd.verify(b)
        assert bytes(alone) == bytes(verdicts[i]) and alone.reason == REASON_OF_ORACLE[c.ref.verify(b)]
    assert (verdicts[37].reason, verdicts[37].query, verdicts[37].tree) == (TRACE_PATH, 11, 1)
    assert (verdicts[64].reason, verdicts[64].query) == (MALFORMED, 27)
    assert len({verdicts[i].reason for i in bad}) == 3
    assert cd.verify_many([]) == []


def test_64_random_bit_flips_in_one_batch(nlx, ctx, orc):
    c, cd = case(nlx, orc, "all-gates"), circuit(nlx, ctx, orc, "all-gates")
    proof = c.proof
    plb = path_length_bytes(nlx.plonk.proof_layout(cd))
    rng = np.random.default_rng(64)
    flips = [(int(rng.integers(0, len(proof))), int(rng.integers(0, 8))) for _ in range(64)]
    proofs = [flip(proof, off, bit) for off, bit in flips]
    verdicts = cd.verify_many(proofs)
    for (off, bit), bad, v in zip(flips, proofs, verdicts):
        rc = c.ref.verify(bad)
        assert (v.accepted == 1) == (rc == 1), (off, bit, rc, str(v))
        at = word_at(bad, off, plb)
        if rc != 1 and (at is None or at[1] < P):
            assert v.reason == REASON_OF_ORACLE[rc], (off, bit, rc, str(v))
        elif rc != 1:
            assert v.reason == MALFORMED


def test_bn128_circuits_are_unsupported(nlx, ctx):
    syn = nlx.SyntheticCircuit(5, seed=1)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher="poseidon_bn128")
    try:
        with pytest.raises(nlx.NlxError) as e:
            cd.verifier_data()
        assert e.value.code == -5 and "BN128" in str(e.value)
    finally:
        cd.close()


def test_map_reduce_levels(nlx, ctx, orc):
    """a tree of three map jobs: every (kind, level)'s proofs through one verify_many call each, and one flipped opening"""
    import torch
    mr = importlib.import_module("nlx_amd.mapreduce")
    plan = mr.TreePlan(3)
    prover = mr.GpuTreeProver(nlx, ctx, plan, 9, 9, torch=torch, workers=1)
    by_level = {}

    def record(kind, level, index, public_inputs):
        pr = prover(kind, level, index, public_inputs)
        by_level.setdefault((kind, level if kind == "reduce" else 0), []).append(pr)
        return pr
    mr.run_tree(plan, record)
    assert sorted(by_level) == [("map", 0), ("outer", 0), ("reduce", 0), ("reduce", 1)]
    assert [len(by_level[k]) for k in sorted(by_level)] == [3, 1, 1, 1]
    for (kind, level), proofs in by_level.items():
        assert all(v.ok for v in prover.verify_many(kind, level, proofs)), (kind, level)
    proofs = list(by_level[("map", 0)])
    lay = nlx.plonk.proof_layout(prover.workers[0]["circ"][("map", 0)][1])
    proofs[1] = flip(proofs[1], lay["zs"][0] + 2)
    assert [v.ok for v in prover.verify_many("map", 0, proofs)] == [True, False, True]
