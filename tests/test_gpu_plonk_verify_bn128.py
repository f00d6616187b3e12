"""GPU tests of the plonky2 verifier under plonky2x's PoseidonBN128GoldilocksConfig (nlx_verifier_create_hasher,
nlx_verifier_from_circuit_hasher).  The proofs are the device prover's; none of the references is the
code under test:
  paths, folds, final polynomial, proof of work, challenges, digest range - the pure Python model of the config
      (tools/bn128_config_model.py) behind tools/bn128_verify_model.py, which answers in the verdict's terms and puts the
      structural checks (length, count word, path-length bytes, field words < p, digests < r) in front;
  the vanishing identity - the Goldilocks twin: the two configs share the proof layout byte for byte, so the same change is applied
      to the ORACLE prover's Goldilocks proof of the same circuit and witness and the oracle's verifier is asked (orc_verify,
      REASON_OF_ORACLE).
The device accepts <=> the twin's return code is 1 and the model does not refuse.  tests/test_gpu_bn128_prove.py pins honest
proofs' openings to the oracle's polynomials, so "honest => valid" is not circular.  The model costs 1-2 ms per permutation:
every test stays below about 20 000 of them."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, P
from plonk_verify_cases import CASES, CONSTRAINTS, FRI_PATH, MALFORMED, POW, PUBLIC_INPUTS, REASON_OF_ORACLE, TRACE_PATH, flip

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn128_config_model as cm  # noqa: E402
import bn128_verify_model as vm  # noqa: E402

m = cm.m
R = cm.R
pytestmark = pytest.mark.gpu

BN, GOLD = "poseidon_bn128", "poseidon_goldilocks"
NLX_E_INVAL, NLX_E_RANGE, NLX_E_UNSUPPORTED = -1, -4, -5
HONEST = ["rows5", "rows6-one-selector", "all-gates", "wide-comparison", "one-challenge-cap0-arity4", "cap5-no-pow", "arity8",
          "layer-inside-cap", "rows5-one-query"]
# where the model replays the whole honest proof too: the cases below 2^9 rows, and of the 2^9-row cases the two cheapest
MODEL_TOO = ["rows5", "rows6-one-selector", "layer-inside-cap", "rows5-one-query", "one-challenge-cap0-arity4", "arity8"]
assert vm.MALFORMED == MALFORMED and vm.CONSTRAINTS == CONSTRAINTS and vm.FRI_PATH == FRI_PATH and vm.POW == POW


def _ints(words):
    return [m.from_words(w) for w in np.asarray(words).reshape(-1, 4)]


class BnCase:
    """a circuit of plonk_verify_cases.CASES under the BN128 config (`cd`, with the device prover's proof), what the model needs to
    replay it, and its Goldilocks twin: the oracle's circuit data (`ref`) and the oracle prover's proof of the same witness"""

    def __init__(self, nlx, ctx, orc, name, **cfg_over):
        log_n, kw, cfg = CASES[name]
        self.syn = nlx.SyntheticCircuit(log_n, config=nlx.CircuitConfig(**dict(cfg, **cfg_over)), **kw)
        self.cd = nlx.CircuitData.from_synthetic(ctx, self.syn, hasher=BN)
        self.proof = self.cd.prove(self.syn.wires, self.syn.public_inputs)
        self.sh = cm.Shape.from_synthetic(self.syn)
        self.digest = m.from_words(self.cd.circuit_digest)
        self.cs_cap = _ints(self.cd.constants_sigmas_cap)
        self.lay = nlx.plonk.proof_layout(self.cd)
        self.ref = orc.Circuit.from_synthetic(self.syn)
        self.twin = self.ref.prove(self.syn.wires, self.syn.public_inputs)
        assert len(self.twin) == len(self.proof) == self.lay["total"] and self.ref.verify(self.twin) == 1
        self.pis = [int(v) for v in self.syn.public_inputs]

    def answer(self, bad, twin_bad, public_inputs=None):
        """the references' answer for the changed proof `bad`, `twin_bad` being the twin with the same change"""
        return vm.classify(bad, self.lay, self.sh, self.digest, self.cs_cap, self.ref.verify(twin_bad), public_inputs)


_cases = {}


def bn_case(nlx, ctx, orc, name, **cfg_over):
    key = (name, tuple(sorted(cfg_over.items())))
    if key not in _cases:
        _cases[key] = BnCase(nlx, ctx, orc, name, **cfg_over)
    return _cases[key]


def _held_to(v, a, what):
    """the device's verdict `v` against the references' answer `a`"""
    assert (v.accepted == 1) == a.accepted and v.reason == a.reason, (what, str(v), a)
    for field in ("query", "tree", "layer", "x_index"):
        if getattr(a, field) is not None:
            assert getattr(v, field) == getattr(a, field), (what, field, str(v), a)


# ---- 1. honest proofs ----
@pytest.mark.parametrize("name", HONEST)
def test_honest_proofs_are_accepted(nlx, ctx, orc, name):
    c = bn_case(nlx, ctx, orc, name)
    cd = c.cd
    assert cd.hasher == BN
    vd = cd.verifier_data(BN)
    assert vd.hasher == BN and vd.proof_bytes == len(c.proof)
    v = cd.verify(c.proof)
    assert v.ok and v.reason == 0 and v.reason_name == "accept", str(v)
    v.raise_if_rejected()
    assert cd.verify(cd.prove(c.syn.wires, c.syn.public_inputs)).ok
    if name in MODEL_TOO:
        cm.verify(c.proof, c.sh, c.digest, c.cs_cap)
    # a verifier made from descriptor, cap and digest alone gives byte-equal verdicts
    key = nlx.VerifierData(ctx, c.syn.desc(), cd.constants_sigmas_cap, cd.circuit_digest, hasher=BN)
    try:
        assert key.hasher == BN and key.proof_bytes == len(c.proof)
        bad = flip(c.proof, c.lay["wires"][0] + 5)
        assert bytes(key.verify(c.proof)) == bytes(v)
        assert bytes(key.verify(bad)) == bytes(cd.verify(bad)) and not key.verify(bad).ok
    finally:
        key.close()


def test_honest_shapes_cover_the_chunk_remainders(nlx, ctx, orc):
    """the leaves of the honest cases - the opened rows and the commit-phase cosets of 8, 16 and 32 words - leave last chunks of
    1, 2, 5, 7, 8 and 9 (a whole one) words"""
    rem, fri = set(), set()
    for name in HONEST:
        lay = bn_case(nlx, ctx, orc, name).lay
        rem |= {(w - 1) % 9 + 1 for w in lay["tree_cols"]}
        if lay["n_layers"]:
            fri.add(2 * lay["arity"])
    rem |= {(w - 1) % 9 + 1 for w in fri}
    assert {1, 2, 5, 7, 8, 9} <= rem and fri == {8, 16, 32}


# ---- 2. refusals, and hasher 0 through the new entries ----
def _raw_verdict(nlx, handle, proof):
    v = nlx.stark.Verdict()
    assert nlx.lib.dll.nlx_verify(handle, proof, len(proof), None, ctypes.byref(v)) == 0
    return bytes(v)


def test_refusals(nlx, ctx, orc):
    dll = nlx.lib.dll
    zero4 = np.zeros(4, np.uint64)
    lk = nlx.SyntheticCircuit(9, seed=5, num_luts=1, lut_bits=6, num_lookups=100)
    narrow = nlx.SyntheticCircuit(6, seed=6, config=nlx.CircuitConfig(num_challenges=1, rate_bits=2, quotient_degree_factor=4),
                                  pct_poseidon=20, pct_arithmetic=30, pct_base_sum=5, pct_constant=5)
    for syn in (lk, narrow):
        d = syn.desc()
        cap = np.zeros(4 << d.cap_height, np.uint64)
        with pytest.raises(nlx.NlxError) as e:
            nlx.VerifierData(ctx, d, cap, zero4, hasher=BN)
        assert e.value.code == NLX_E_UNSUPPORTED
    d = lk.desc()
    nlx.VerifierData(ctx, d, np.zeros(4 << d.cap_height, np.uint64), zero4).close()   # the Goldilocks config takes lookup tables
    # cap and digest are digests of the hasher
    c = bn_case(nlx, ctx, orc, "rows5")
    d = c.syn.desc()
    cap, dig = c.cd.constants_sigmas_cap, c.cd.circuit_digest
    over = np.array(m.to_words(R), dtype=np.uint64)
    bad_cap = cap.copy()
    bad_cap[1] = over
    for args in ((bad_cap, dig), (cap, over)):
        with pytest.raises(nlx.NlxError) as e:
            nlx.VerifierData(ctx, d, args[0], args[1], hasher=BN)
        assert e.value.code == NLX_E_RANGE
    h = ctypes.c_void_p()
    assert dll.nlx_verifier_create_hasher(ctx.handle, ctypes.byref(d), cap.ctypes.data, dig.ctypes.data, 7, ctypes.byref(h)) == NLX_E_RANGE
    assert dll.nlx_verifier_create_hasher(None, None, None, None, 1, ctypes.byref(h)) == NLX_E_INVAL and not h.value
    assert dll.nlx_verifier_from_circuit_hasher(None, 1, ctypes.byref(h)) == NLX_E_INVAL
    assert dll.nlx_verifier_hasher(None) == NLX_E_INVAL
    # the config the caller expects against the circuit's
    gold = nlx.CircuitData.from_synthetic(ctx, c.syn)
    try:
        with pytest.raises(nlx.NlxError) as e:
            gold.verifier_data(hasher=BN)
        assert e.value.code == NLX_E_INVAL
        assert dll.nlx_verifier_from_circuit_hasher(c.cd.handle, 0, ctypes.byref(h)) == NLX_E_INVAL and not h.value
        assert dll.nlx_verifier_from_circuit_hasher(c.cd.handle, 7, ctypes.byref(h)) == NLX_E_RANGE
        with pytest.raises(nlx.NlxError) as e:                   # the old entry keeps its refusal
            c.cd.verifier_data()
        assert e.value.code == NLX_E_UNSUPPORTED and "BN128" in str(e.value)
        # hasher 0 through the new entries: the old entries' verdicts, byte for byte
        gd = c.syn.desc()
        proofs = [c.twin, flip(c.twin, c.lay["wires"][0] + 5), flip(c.twin, c.lay["query"][3]["row"][1][0] + 1), c.twin[:-8]]
        old = [bytes(v) for v in gold.verify_many(proofs)]
        assert gold.verifier_data().hasher == GOLD
        assert dll.nlx_verifier_from_circuit_hasher(gold.handle, 0, ctypes.byref(h)) == 0
        assert dll.nlx_verifier_hasher(h) == 0
        assert [_raw_verdict(nlx, h, p) for p in proofs] == old
        dll.nlx_verifier_destroy(h)
        gcap, gdig = gold.constants_sigmas_cap, gold.circuit_digest
        assert dll.nlx_verifier_create_hasher(ctx.handle, ctypes.byref(gd), gcap.ctypes.data, gdig.ctypes.data, 0, ctypes.byref(h)) == 0
        assert [_raw_verdict(nlx, h, p) for p in proofs] == old
        dll.nlx_verifier_destroy(h)
        assert len({o for o in old}) == 4
    finally:
        gold.close()


# ---- 3. cross-config ----
def test_cross_config(nlx, ctx, orc):
    c = bn_case(nlx, ctx, orc, "rows5")
    cd = c.cd
    assert not cd.verify(c.twin).ok                              # a Goldilocks proof of the same circuit
    gold = nlx.CircuitData.from_synthetic(ctx, c.syn)
    try:
        assert gold.verify(c.twin).ok
        assert not gold.verify(c.proof).ok                       # no reason asserted: digest words may or may not exceed p
    finally:
        gold.close()
    wrong = (c.digest + 1) % R
    key = nlx.VerifierData(ctx, c.syn.desc(), cd.constants_sigmas_cap, np.array(m.to_words(wrong), dtype=np.uint64), hasher=BN)
    try:
        v = key.verify(c.proof)
        assert not v.ok and v.reason == CONSTRAINTS
    finally:
        key.close()
    assert cd.verify(c.proof, c.pis).ok
    other = list(c.pis)
    other[-1] = (other[-1] + 1) % P
    v = cd.verify(c.proof, other)
    assert not v.ok and v.reason == PUBLIC_INPUTS
    _held_to(v, c.answer(c.proof, c.twin, other), "other public inputs")
    vs = cd.verify_many([c.proof, c.proof], [c.pis, other])
    assert vs[0].ok and vs[1].reason == PUBLIC_INPUTS


# ---- 4. named tampers ----
def _set_word(proof, at, value):
    return proof[:at] + int(value).to_bytes(8, "little") + proof[at + 8:]


def _tampers(lay):
    """[(name, change: proof -> proof, twin's change or None for the same, query or None, tree or None, layer or None)] - the
    list of tests/test_gpu_plonk_verify.py::_tampers, one bit each and placed with the layout, as changes that apply to the proof
    and to its twin alike; then the digest-specific ones, whose twin gets a flipped bit at the same place"""
    q_last = len(lay["query"]) - 1

    def bit(off, b=0):
        return lambda p: flip(p, off, b)

    out = [("%s cap" % n, bit(lay["cap"][i][0] + 9 + 32 * i), None, None, None, None) for i, n in enumerate(("wires", "zs", "quotient"))]
    for k, name in enumerate(["constants", "sigmas", "wires", "zs", "zs_next", "partial_products", "quotient"]):
        assert lay[name][1] >= 16
        out.append(("%s opening" % name, bit(lay[name][0] + lay[name][1] - 16 + k % 8, k % 5), None, None, None, None))
    out += [
        ("FRI commit cap", bit(lay["fri_cap"][0][0] + 3), None, None, None, None),
        ("final polynomial", bit(lay["final_poly"][0] + 16, 3), None, None, None, None),
        ("witness", bit(lay["pow_witness"][0], 5), None, None, None, None),
        ("public input", bit(lay["public_inputs"][0] + 8, 1), None, None, None, None),
        ("count word", bit(lay["num_public_inputs"][0], 2), None, None, None, None),
        ("cut by 8", lambda p: p[:-8], None, None, None, None),
        ("extended by 8", lambda p: p + b"\0" * 8, None, None, None, None),
    ]
    for q in (0, q_last):
        Q = lay["query"][q]
        for t in range(4):
            out.append(("query %d row of tree %d" % (q, t), bit(Q["row"][t][0] + 8 * (lay["tree_cols"][t] - 1) + 2), None, q, t, None))
        out.append(("query %d sibling of tree 0" % q, bit(Q["path"][0][0] + 32 + 5, 7), None, q, 0, None))
        out.append(("query %d sibling of tree 3" % q, bit(Q["path"][3][0] + Q["path"][3][1] - 1), None, q, 3, None))
        out.append(("query %d path-length byte of tree 2" % q, bit(Q["path_len"][2][0]), None, q, 2, None))
        out.append(("query %d path-length byte of layer 0" % q, bit(Q["layer"][0]["path_len"][0], 1), None, q, None, 0))
        out.append(("query %d layer sibling" % q, bit(Q["layer"][0]["path"][0] + 7), None, q, None, 0))
    # digests are not field words.  r's top word is below p, so a top word one above it makes a digest >= r of words below p;
    # the highest word that can be >= p in a digest below r is the third
    top = (R >> 192) + 1
    assert top < P
    Q = lay["query"][1]
    sib, lsib = Q["path"][1][0] + 64, Q["layer"][0]["path"][0] + 32
    out += [
        ("a cap digest >= r", lambda p: _set_word(p, lay["cap"][1][0] + 24, top), bit(lay["cap"][1][0] + 24), None, None, None),
        ("a sibling word >= p, digest < r", lambda p: _set_word(p, sib + 16, 2 ** 64 - 1), bit(sib + 16), 1, 1, None),
        ("a layer sibling word >= p, digest < r", lambda p: _set_word(p, lsib + 16, P), bit(lsib + 16), 1, None, 0),
        ("a sibling >= r", lambda p: _set_word(p, sib + 24, top), bit(sib + 24), None, None, None),
        ("a FRI cap digest >= r", lambda p: _set_word(p, lay["fri_cap"][0][0] + 24, 2 ** 64 - 1), bit(lay["fri_cap"][0][0] + 24), None, None, None),
    ]
    return out


def test_named_tampers(nlx, ctx, orc):
    c = bn_case(nlx, ctx, orc, "all-gates", fri_num_queries=5)
    cd, lay = c.cd, c.lay
    assert cd.verify(c.proof).ok and len(lay["query"]) == 5
    tampers = _tampers(lay)
    bads = [t[1](c.proof) for t in tampers]
    verdicts = cd.verify_many(bads)
    alone = {i: cd.verify(bads[i]) for i in (0, 5, 12, len(tampers) - 1, len(tampers) - 3)}
    seen, by_name = set(), {}
    for i, ((name, change, twin_change, q, tree, layer), bad, v) in enumerate(zip(tampers, bads, verdicts)):
        a = c.answer(bad, (twin_change or change)(c.twin))
        print("%-45s device %-16s references %r" % (name, v.reason_name, a))
        assert not a.accepted and not v.ok, name
        _held_to(v, a, name)
        seen.add(v.reason)
        by_name[name] = v
        # query, tree and layer are those of the tamper's position
        if q is not None:
            assert v.query == q, (name, str(v))
        if tree is not None:
            assert v.tree == tree, (name, str(v))
        if layer is not None:
            assert v.layer == layer, (name, str(v))
        if v.reason in (TRACE_PATH, FRI_PATH):
            assert v.x_index == cm.replay(bad, c.sh, c.digest)["query_indices"][v.query], name
        if i in alone:
            assert bytes(alone[i]) == bytes(v), name
    assert {MALFORMED, CONSTRAINTS, POW, TRACE_PATH, FRI_PATH} <= seen
    assert by_name["a cap digest >= r"].reason == MALFORMED and by_name["a sibling >= r"].reason == MALFORMED
    assert by_name["a FRI cap digest >= r"].reason == MALFORMED
    assert by_name["a sibling word >= p, digest < r"].reason == TRACE_PATH
    assert by_name["a layer sibling word >= p, digest < r"].reason == FRI_PATH
    with pytest.raises(ValueError):
        verdicts[0].raise_if_rejected()
    assert "query" in verdicts[0].message and "tree" in verdicts[0].message and "layer" in verdicts[0].message


# ---- 5. seeded bit flips ----
def test_32_seeded_bit_flips_in_one_batch(nlx, ctx, orc):
    """32 flips of default_rng(64) on "one-challenge-cap0-arity4" in one verify_many call: acceptance and reason are the
    references'.  The seed's check is part of the run: vm.classify raises where the twin's code and the model contradict each
    other (twin code 1 <=> the model accepts), and it did not for any of the 32 flips of this seed on the MI355X run that
    this test was written on - the BN128 proof is the device prover's, so the check cannot be made without a device."""
    c = bn_case(nlx, ctx, orc, "one-challenge-cap0-arity4")
    rng = np.random.default_rng(64)
    flips = [(int(rng.integers(0, len(c.proof))), int(rng.integers(0, 8))) for _ in range(32)]
    bads = [flip(c.proof, off, b) for off, b in flips]
    verdicts = c.cd.verify_many(bads)
    reasons = {}
    for (off, b), bad, v in zip(flips, bads, verdicts):
        a = c.answer(bad, flip(c.twin, off, b))
        print("flip %6d.%d  device %-16s references %r" % (off, b, v.reason_name, a))
        _held_to(v, a, (off, b))
        reasons[v.reason] = reasons.get(v.reason, 0) + 1
    print("reasons:", reasons)
    assert len(reasons) >= 2


# ---- 6. batch = alone ----
def test_batch_gives_each_proof_its_own_verdict(nlx, ctx, orc):
    c = bn_case(nlx, ctx, orc, "rows6-one-selector")
    lay, proof = c.lay, c.proof
    other = c.cd.prove(c.syn.wires, c.syn.public_inputs)
    proofs = [proof,
              flip(proof, lay["query"][2]["path_len"][1][0]),                      # MALFORMED
              flip(proof, lay["zs"][0] + 2),                                       # CONSTRAINTS
              other,
              flip(proof, lay["query"][4]["layer"][0]["path"][0] + 7),             # FRI_PATH
              flip(proof, lay["query"][1]["row"][3][0] + 1)]                       # TRACE_PATH
    alone = [bytes(c.cd.verify(p)) for p in proofs]
    reasons = [c.cd.verify(p).reason for p in proofs]
    assert reasons == [0, MALFORMED, CONSTRAINTS, 0, FRI_PATH, TRACE_PATH]
    for perm in ([0, 1, 2, 3, 4, 5], [4, 2, 0, 5, 1, 3], [5, 4, 3, 2, 1, 0]):
        got = c.cd.verify_many([proofs[i] for i in perm])
        assert [bytes(v) for v in got] == [alone[i] for i in perm], perm
