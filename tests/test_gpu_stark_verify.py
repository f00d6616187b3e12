"""GPU tests of the STARK verifier (nlx_stark_verify, nlx_stark_verify_batch): honest proofs of every code path are accepted,
every named tamper is rejected for the reason the oracle's sequential verifier gives and at the place the tamper sits, unsatisfied
statements fail the constraint check, and a batch gives each proof the verdict it gets alone.  The proofs under test are the
ORACLE's provers' (orc.stark_prove / orc.stark_prove_rounds); the GPU prover's bytes are checked on top."""
import numpy as np
import pytest

from conftest import P
from stark_verify_cases import ALL_CASES, CONSTRAINTS, MALFORMED, PUBLIC_INPUTS, REASON_OF_ORACLE, case
from test_logup import make_trace, range_air, rounds_fn

pytestmark = pytest.mark.gpu

_provers = {}


def prover(nlx, ctx, orc, name):
    """the statement's resident STARK, built once a session"""
    if name not in _provers:
        _provers[name] = case(nlx, orc, name).st.build(ctx)
    return _provers[name]


@pytest.mark.parametrize("name", ALL_CASES)
def test_honest_proofs_are_accepted(nlx, ctx, orc, name):
    c, pr = case(nlx, orc, name), prover(nlx, ctx, orc, name)
    proof = c.oracle_proof(orc)
    assert orc.stark_verify(c.st.desc, proof) == 1
    assert len(proof) == pr.proof_bytes == nlx.stark.proof_layout(c.st)["total"]
    v = pr.verify(proof)
    assert v.ok and v.reason == 0 and v.reason_name == "accept", str(v)
    v.raise_if_rejected()
    # the prover the verifier ships with
    got = c.gpu_proof(pr)
    assert pr.verify(got).ok


def _flip(proof, off, bit=0):
    bad = bytearray(proof)
    bad[off] ^= 1 << bit
    return bytes(bad)


def _tampers(proof, lay, d):
    """[(name, tampered proof, query or None, tree or None, layer or None)] - one bit each, placed with the layout"""
    n_or = len(lay["oracle_cols"])
    q_last = len(lay["query"]) - 1
    out = [
        ("trace cap entry", _flip(proof, lay["cap"][0][0] + 40), None, None, None),
        ("quotient cap", _flip(proof, lay["cap"][n_or - 1][0] + 9), None, None, None),
        ("local opening", _flip(proof, lay["local"][0] + 16), None, None, None),
        ("next opening", _flip(proof, lay["next"][0] + 24), None, None, None),
        ("quotient opening", _flip(proof, lay["quotient"][0] + 8), None, None, None),
        ("final polynomial", _flip(proof, lay["final_poly"][0] + 16, 3), None, None, None),
        ("witness", _flip(proof, lay["pow_witness"][0], 5), None, None, None),
        ("public input", _flip(proof, lay["public_inputs"][0] + 8, 1), None, None, None),
        ("cut by 8", proof[:-8], None, None, None),
        ("extended by 8", proof + b"\0" * 8, None, None, None),
    ]
    # public input 0 as a word that is not canonical: itself + p, the same field element, where that fits 64 bits (it does for
    # values below 2^32 - 1: test_public_input_alias has such a statement; wide_air's are random), else p + its low bits
    at = lay["public_inputs"][0]
    pi0 = int.from_bytes(proof[at:at + 8], "little")
    alias = pi0 + P if pi0 + P < 1 << 64 else P + pi0 % 0xFFFFFFFF
    out.append(("public input 0 not canonical", proof[:at] + alias.to_bytes(8, "little") + proof[at + 8:], None, None, None))
    if lay["n_layers"]:
        out.append(("FRI commit cap", _flip(proof, lay["fri_cap"][0][0] + 3), None, None, None))
    for q in (0, q_last):
        Q = lay["query"][q]
        for o in (0, n_or - 2, n_or - 1):   # first and last trace tree, the quotient tree
            out.append(("query %d row of tree %d" % (q, o), _flip(proof, Q["row"][o][0] + 8 * (lay["oracle_cols"][o] - 1) + 2), q, o, None))
        out.append(("query %d sibling of tree 0" % q, _flip(proof, Q["path"][0][0] + 32 + 5, 7), q, 0, None))
        out.append(("query %d sibling of the quotient tree" % q, _flip(proof, Q["path"][n_or - 1][0] + Q["path"][n_or - 1][1] - 1), q, n_or - 1, None))
    out.append(("path-length byte of tree %d, query 1" % (n_or - 1), _flip(proof, lay["query"][1]["path_len"][n_or - 1][0]), 1, n_or - 1, None))
    if lay["n_layers"]:
        L0 = lay["query"][q_last]["layer"][0]
        out.append(("path-length byte of layer 0", _flip(proof, L0["path_len"][0], 1), q_last, None, 0))
        out.append(("layer sibling", _flip(proof, L0["path"][0] + 7), q_last, None, 0))
    return out


@pytest.fixture(scope="module", params=["wide16", "wide320-batch64"])
def tamper_target(request, nlx, ctx, orc):
    c = case(nlx, orc, request.param)
    pr = prover(nlx, ctx, orc, request.param)
    proof = c.oracle_proof(orc)
    honest = pr.verify(proof)
    assert honest.ok
    return c, pr, proof, nlx.stark.proof_layout(c.st)


def test_named_tampers(nlx, orc, tamper_target):
    c, pr, proof, lay = tamper_target
    d = c.st.desc
    tampers = _tampers(proof, lay, d)
    assert lay["n_layers"] >= 1
    verdicts = pr.verify_many([t[1] for t in tampers])
    seen = set()
    for (name, bad, q, tree, layer), v, alone in zip(tampers, verdicts, [pr.verify(t[1]) for t in tampers[:6]] + [None] * len(tampers)):
        rc = orc.stark_verify(d, bad)
        assert rc != 1 and not v.ok, name
        assert v.reason == REASON_OF_ORACLE[rc], (name, rc, str(v))
        seen.add(v.reason)
        if q is not None:
            assert v.query == q, (name, str(v))
        if tree is not None:
            assert v.tree == tree, (name, str(v))
        if layer is not None:
            assert v.layer == layer, (name, str(v))
        if alone is not None:   # the single call agrees with the batch
            assert bytes(alone) == bytes(v), name
    assert {MALFORMED, CONSTRAINTS, 5, 7} <= seen   # structure, constraints, trace paths and FRI paths were all reached
    with pytest.raises(ValueError):
        verdicts[0].raise_if_rejected()
    assert "query" in verdicts[0].message and "tree" in verdicts[0].message and "layer" in verdicts[0].message


def test_layer_evaluations(nlx, orc, tamper_target):
    """layer 0's evaluation at the query's own position (the fold check) and at another one (the layer's path), for query 0 and
    the last: the position within the coset is x_index mod arity, which the verdict of a path tamper on the same query gives"""
    c, pr, proof, lay = tamper_target
    d = c.st.desc
    for q in (0, len(lay["query"]) - 1):
        Q = lay["query"][q]
        x_index = pr.verify(_flip(proof, Q["path"][0][0])).x_index   # a trace-path tamper of query q names the query's index
        within = x_index % lay["arity"]
        own = _flip(proof, Q["layer"][0]["evals"][0] + 16 * within + 4)
        other = _flip(proof, Q["layer"][0]["evals"][0] + 16 * ((within + 1) % lay["arity"]) + 9)
        for bad, want in ((own, 6), (other, 7)):
            rc = orc.stark_verify(d, bad)
            v = pr.verify(bad)
            assert rc in (-7, -8) and REASON_OF_ORACLE[rc] == want == v.reason, (q, rc, str(v))
            assert (v.query, v.layer, v.x_index) == (q, 0, x_index)


def _plus_one(proof, off):
    """the word at `off` replaced by itself + 1 mod p"""
    word = (int.from_bytes(proof[off:off + 8], "little") + 1) % P
    return proof[:off] + word.to_bytes(8, "little") + proof[off + 8:]


@pytest.mark.parametrize("name", ["wide16-batch12", "fib7-nondefault"])
def test_opened_word_plus_one(nlx, ctx, orc, name):
    """An opened trace word of query 0 plus 1 mod p, in the first trace commitment and in the last (two runs of columns that enter
    both FRI batches for wide16-batch12, one for fib7-nondefault): the commitment's path fails, before anything of FRI is judged.
    Then a layer's evaluation at the query's own position, evals[x mod arity]: the fold check of that layer.  Reason, query, tree
    and layer are the oracle verifier's."""
    c, pr = case(nlx, orc, name), prover(nlx, ctx, orc, name)
    proof = c.oracle_proof(orc)
    lay = nlx.stark.proof_layout(c.st)
    d = c.st.desc
    Q = lay["query"][0]
    n_trace = len(lay["oracle_cols"]) - 1
    assert n_trace == (2 if name == "wide16-batch12" else 1) and lay["n_layers"] >= 1
    x_index = None
    for o in sorted({0, n_trace - 1}):
        bad = _plus_one(proof, Q["row"][o][0] + 8 * (lay["oracle_cols"][o] // 2))
        rc, v = orc.stark_verify(d, bad), pr.verify(bad)
        assert rc == -5 and v.reason == REASON_OF_ORACLE[rc] == 5, (o, rc, str(v))
        assert (v.query, v.tree, v.layer) == (0, o, 0), (o, str(v))
        x_index = v.x_index
    for k in range(lay["n_layers"]):
        within = (x_index >> (k * d.fri_arity_bits)) % lay["arity"]
        bad = _plus_one(proof, Q["layer"][k]["evals"][0] + 16 * within)
        rc, v = orc.stark_verify(d, bad), pr.verify(bad)
        assert rc == -7 and v.reason == REASON_OF_ORACLE[rc] == 6, (k, rc, str(v))
        assert (v.query, v.layer, v.x_index) == (0, k, x_index), (k, str(v))


def test_public_inputs_argument(nlx, orc, tamper_target):
    c, pr, proof, lay = tamper_target
    assert pr.verify(proof, c.pis).ok
    wrong = [int(v) for v in c.pis]
    wrong[-1] = (wrong[-1] + 1) % P
    v = pr.verify(proof, wrong)
    assert not v.ok and v.reason == PUBLIC_INPUTS and v.reason_name == "public inputs"
    with pytest.raises(nlx.NlxError):   # NLX_E_RANGE: not canonical
        pr.verify(proof, [P] + wrong[1:])
    vs = pr.verify_many([proof, proof], [c.pis, wrong])
    assert vs[0].ok and vs[1].reason == PUBLIC_INPUTS


def test_public_input_alias(nlx, ctx, orc):
    """public input 0 replaced by itself + p - the same field element, another word: malformed, as for the oracle"""
    c, pr = case(nlx, orc, "fib5"), prover(nlx, ctx, orc, "fib5")
    proof = c.oracle_proof(orc)
    at = nlx.stark.proof_layout(c.st)["public_inputs"][0]
    pi0 = int.from_bytes(proof[at:at + 8], "little")
    assert pi0 == int(c.pis[0]) and pi0 + P < 1 << 64
    bad = proof[:at] + (pi0 + P).to_bytes(8, "little") + proof[at + 8:]
    assert orc.stark_verify(c.st.desc, bad) == -1
    v = pr.verify(bad)
    assert not v.ok and v.reason == MALFORMED


def test_unsatisfied_statements(nlx, ctx, orc):
    S = nlx.stark
    c, pr = case(nlx, orc, "wide16"), prover(nlx, ctx, orc, "wide16")
    t2 = c.t.copy()
    t2[1, 3] = (int(t2[1, 3]) + 1) % P
    bad = orc.stark_prove(c.st.desc, t2, c.pis)
    assert orc.stark_verify(c.st.desc, bad) == -2
    v = pr.verify(bad)
    assert not v.ok and v.reason == CONSTRAINTS and v.challenge in (0, 1)
    # a LogUp witness with a wrong multiplicity
    air, _ = range_air(nlx, 5, 6)
    st = S.Stark(air, 7, S.StarkConfig(fri_num_queries=20))
    t0 = make_trace(orc, 5, 6, 7)
    t0[5, 2] = (int(t0[5, 2]) + 1) % P
    bad = orc.stark_prove_rounds(st.desc, rounds_fn(orc, t0, 5, 6), [])
    assert orc.stark_verify(st.desc, bad) == -2
    v = prover(nlx, ctx, orc, "range-check").verify(bad)   # the same statement
    assert not v.ok and v.reason == CONSTRAINTS


def test_batch_of_65(nlx, ctx, orc):
    """more than a wave of proofs, three of them tampered in three different ways"""
    c, pr = case(nlx, orc, "fib5"), prover(nlx, ctx, orc, "fib5")
    proof = c.oracle_proof(orc)
    lay = nlx.stark.proof_layout(c.st)
    bad = {2: _flip(proof, lay["local"][0] + 3),
           37: _flip(proof, lay["query"][11]["row"][1][0] + 1),
           64: _flip(proof, lay["query"][83]["path_len"][0][0])}
    proofs = [bad.get(i, proof) for i in range(65)]
    verdicts = pr.verify_many(proofs)
    assert [i for i, v in enumerate(verdicts) if not v.ok] == [2, 37, 64]
    for i, b in bad.items():
        alone = pr.verify(b)
        assert bytes(alone) == bytes(verdicts[i]) and alone.reason == REASON_OF_ORACLE[orc.stark_verify(c.st.desc, b)]
    assert (verdicts[37].reason, verdicts[37].query, verdicts[37].tree) == (5, 11, 1)
    assert (verdicts[64].reason, verdicts[64].query) == (MALFORMED, 83)
    assert len({verdicts[i].reason for i in bad}) == 3
    assert pr.verify_many([]) == []


def test_64_random_bit_flips_in_one_batch(nlx, ctx, orc):
    c, pr = case(nlx, orc, "wide16"), prover(nlx, ctx, orc, "wide16")
    proof = c.oracle_proof(orc)
    rng = np.random.default_rng(64)
    flips = [(int(rng.integers(0, len(proof))), int(rng.integers(0, 8))) for _ in range(64)]
    proofs = [_flip(proof, off, bit) for off, bit in flips]
    verdicts = pr.verify_many(proofs)
    for (off, bit), bad, v in zip(flips, proofs, verdicts):
        rc = orc.stark_verify(c.st.desc, bad)
        assert (v.accepted == 1) == (rc == 1), (off, bit, rc, str(v))
        if rc != 1:
            assert v.reason == REASON_OF_ORACLE[rc], (off, bit, rc, str(v))


def test_sha256_prover_verifies_its_proof(nlx, ctx):
    sp = nlx.sha256_air.Sha256Prover(ctx, 2)
    proof, _ = sp.prove([b"abc"])
    assert sp.verify(proof).ok
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 0x10
    v = sp.verify(bytes(bad))
    assert not v.ok and v.reason != 0
    sp.close()


def test_sha512_and_ed25519_provers_verify_their_proofs(nlx, ctx):
    """the two other AIRs of a Sync step (programs with 64-register segments: the constraint kernel's largest register file), at the
    smallest sizes their own tests use; and nlx_last_error after an accept no longer holds the line of the rejection before it"""
    sp = nlx.sha512_air.Sha512Prover(ctx, 2)
    proof, _ = sp.prove([b"abc"])
    assert sp.verify(proof).ok
    bad = bytearray(proof)
    bad[len(bad) // 3] ^= 0x04
    v = sp.verify(bytes(bad))
    assert not v.ok and v.reason != 0 and "does not verify" in nlx.lib.dll.nlx_last_error(ctx.handle).decode()
    assert sp.verify(proof).ok and nlx.lib.dll.nlx_last_error(ctx.handle) == b""
    sp.close()
    from test_ed25519_air import rfc_slots
    E = nlx.ed25519_air
    pr = E.Ed25519Prover(ctx, 4)
    proof = pr.prove((rfc_slots(nlx) + [E.inactive_slot()]) * 4)
    assert pr.verify(proof).ok
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 0x20
    assert not pr.verify(bytes(bad)).ok
    pr.close()
