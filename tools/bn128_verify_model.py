#!/usr/bin/env python3
"""The reference the device verifier of PoseidonBN128-config proofs is tested against (nlx_verifier_create_hasher with
NLX_HASHER_POSEIDON_BN128): tools/bn128_config_model.py's replay verifier, used as it is, behind an answer
in the device verdict's terms - a reason code in the order of a sequential verifier with the query, tree
and layer of the failing check - and with the structural checks the device's parser makes put in front of it.

What each part decides:
  structure()   length, public-input count word, path-length bytes, field words below p, digests below r  -> MALFORMED
  the caller    the vanishing identity: the model does not evaluate gates, so the caller passes what the frozen oracle's
                verifier says of the SAME change applied to the Goldilocks proof of the same circuit and witness (`twin_rc`) -
                the two configs share the proof layout byte for byte (rule 7), so which check a changed word reaches depends only
                on where it sits                                                                           -> CONSTRAINTS
  cm.verify     proof of work, every Merkle path, every fold, the final polynomial, with the challenges of its own replay
                                                                     -> POW, TRACE_PATH, FRI_FOLD, FRI_PATH, FINAL_POLY, accept
Test infrastructure: pure Python, 1-2 ms per BN128 permutation."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn128_config_model as cm  # noqa: E402

ACCEPT, MALFORMED, PUBLIC_INPUTS, CONSTRAINTS, POW, TRACE_PATH, FRI_FOLD, FRI_PATH, FINAL_POLY = range(9)
P, R = cm.P, cm.R
ORACLE_CONSTRAINTS = -2   # oracle/plonk.c orc_verify: the vanishing identity fails


class Answer:
    """what the device's verdict must say: accepted, reason, and where a reason has a place, query / tree / layer / x_index
    (None: not determined by the reason)"""

    def __init__(self, reason, query=None, tree=None, layer=None, x_index=None):
        self.accepted = reason == ACCEPT
        self.reason, self.query, self.tree, self.layer, self.x_index = reason, query, tree, layer, x_index

    def __repr__(self):
        return "Answer(reason=%d, query=%r, tree=%r, layer=%r, x_index=%r)" % (self.reason, self.query, self.tree, self.layer, self.x_index)


def structure(proof, lay, num_public_inputs):
    """The parser's findings in its order (csrc/fri_proof_layout.hpp): length, the count word, the first wrong path-length byte,
    the first field word not below p or digest not below r.  lay: plonk.proof_layout's dict.  None: sound."""
    if len(proof) != lay["total"]:
        return Answer(MALFORMED)
    at = lay["num_public_inputs"][0]
    if int.from_bytes(proof[at:at + 8], "little") != num_public_inputs:
        return Answer(MALFORMED)
    skip = []
    for q, Q in enumerate(lay["query"]):
        for t, (ln, path) in enumerate(zip(Q["path_len"], Q["path"])):
            skip.append((ln[0], 1))
            if proof[ln[0]] != path[1] // 32:
                return Answer(MALFORMED, query=q, tree=t)
        for k, ly in enumerate(Q["layer"]):
            skip.append((ly["path_len"][0], 1))
            if proof[ly["path_len"][0]] != ly["path"][1] // 32:
                return Answer(MALFORMED, query=q, layer=k)
    at = 0
    for start, length in sorted(skip + [tuple(sp) for sp in lay["digests"]]) + [(lay["total"], 0)]:
        assert (start - at) % 8 == 0 and start >= at
        if start > at and bool((np.frombuffer(proof, dtype="<u8", count=(start - at) // 8, offset=at) >= np.uint64(P)).any()):
            return Answer(MALFORMED)
        if length > 1:
            assert length % 32 == 0
            for o in range(start, start + length, 32):
                if int.from_bytes(proof[o:o + 32], "little") >= R:
                    return Answer(MALFORMED)
        at = start + length
    return None


_PLACES = [
    (re.compile(r"^proof of work$"), lambda g: Answer(POW)),
    (re.compile(r"^query (\d+) oracle (\d+): Merkle path"), lambda g: Answer(TRACE_PATH, query=int(g[0]), tree=int(g[1]))),
    (re.compile(r"^query (\d+) round (\d+): the coset does not hold"), lambda g: Answer(FRI_FOLD, query=int(g[0]), layer=int(g[1]))),
    (re.compile(r"^query (\d+) round (\d+): Merkle path"), lambda g: Answer(FRI_PATH, query=int(g[0]), layer=int(g[1]))),
    (re.compile(r"^query (\d+): final polynomial$"), lambda g: Answer(FINAL_POLY, query=int(g[0]))),
]


def fri_answer(proof, sh, circuit_digest, constants_sigmas_cap):
    """cm.verify's answer as a reason: ACCEPT, or the first of POW, TRACE_PATH, FRI_FOLD, FRI_PATH, FINAL_POLY it meets (its order
    is the sequential verifier's).  Any other refusal of cm.verify is structural, and structure() comes before this call."""
    try:
        t = cm.verify(proof, sh, circuit_digest, constants_sigmas_cap)
    except cm.Reject as e:
        for rx, make in _PLACES:
            mt = rx.match(str(e))
            if mt:
                a = make(mt.groups())
                if a.query is not None:
                    a.x_index = cm.replay(proof, sh, circuit_digest)["query_indices"][a.query]
                return a
        return Answer(MALFORMED)
    a = Answer(ACCEPT)
    a.replay = t
    return a


def classify(proof, lay, sh, circuit_digest, constants_sigmas_cap, twin_rc, public_inputs=None):
    """The whole answer, in the device's order: structure, the caller's public inputs, the vanishing identity (twin_rc: the
    frozen oracle's return code for the Goldilocks twin of this proof), then cm.verify.  Raises AssertionError where the
    references contradict each other: the twin accepts exactly what the model accepts once both are past the identity."""
    n_pis = lay["public_inputs"][1] // 8
    bad = structure(proof, lay, n_pis)
    if bad is not None:
        return bad
    if public_inputs is not None:
        at = lay["public_inputs"][0]
        if [int.from_bytes(proof[at + 8 * i:at + 8 * i + 8], "little") for i in range(n_pis)] != [int(v) for v in public_inputs]:
            return Answer(PUBLIC_INPUTS)
    if twin_rc == ORACLE_CONSTRAINTS:
        return Answer(CONSTRAINTS)
    a = fri_answer(proof, sh, circuit_digest, constants_sigmas_cap)
    assert a.reason != MALFORMED, "the model refuses a proof the structural checks pass"
    assert (twin_rc == 1) == a.accepted, "the references disagree: the twin's code is %d, the model says %r" % (twin_rc, a)
    return a
