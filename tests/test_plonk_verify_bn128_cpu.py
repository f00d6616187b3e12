"""CPU tests of the host side of the plonky2 verifier under the PoseidonBN128 config: which bytes of a
proof Python's proof_layout calls digests, the wrapper model (tools/bn128_verify_model.py) against the replay verifier it wraps
on a stored proof, and the parser's digest-word rule under a sanitizer (a stand-alone program: nothing loaded into Python runs
under one).  The stored proof (tests/golden/bn128_rows5_one_query.*) is the device prover's proof of plonk_verify_cases'
"rows5-one-query" under the BN128 config, with the circuit digest and constants_sigmas_cap it was made under."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import P, ROOT
from plonk_verify_cases import CASES, case, flip, path_length_bytes, shape_args

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn128_config_model as cm  # noqa: E402
import bn128_verify_model as vm  # noqa: E402

R = cm.R
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def stored(nlx, orc):
    c = case(nlx, orc, "rows5-one-query")                    # the same circuit: its oracle proof is the Goldilocks twin
    key = json.load(open(os.path.join(GOLDEN, "bn128_rows5_one_query.json")))
    proof = open(os.path.join(GOLDEN, "bn128_rows5_one_query.proof"), "rb").read()
    lay = nlx.plonk.proof_layout(c.syn)
    assert key["case"] == "rows5-one-query" and len(proof) == lay["total"] == len(c.proof)
    return dict(c=c, proof=proof, lay=lay, sh=cm.Shape.from_synthetic(c.syn), digest=int(key["circuit_digest"], 16),
                cap=[int(x, 16) for x in key["constants_sigmas_cap"]])


@pytest.mark.parametrize("name", ["rows5", "one-challenge-cap0-arity4", "layer-inside-cap", "lookup-1-table"])
def test_digest_ranges_are_the_caps_and_the_siblings(nlx, name):
    log_n, kw, cfg = CASES[name]
    syn = nlx.SyntheticCircuit(log_n, config=nlx.CircuitConfig(**cfg), **kw)
    lay = nlx.plonk.proof_layout(syn)
    d = syn.desc()
    want = [tuple(sp) for sp in lay["cap"]] + [tuple(sp) for sp in lay["fri_cap"]]
    for q in lay["query"]:
        want += [tuple(sp) for sp in q["path"]] + [tuple(ly["path"]) for ly in q["layer"]]
    want = [sp for sp in want if sp[1]]
    got = [tuple(sp) for sp in lay["digests"]]
    assert got == want and got == sorted(got)                 # in proof order
    assert all(ln % 32 == 0 and ln > 0 for _, ln in got)
    assert all(a + la <= b for (a, la), (b, _) in zip(got, got[1:]))   # disjoint
    log_l = d.degree_bits + d.rate_bits
    n_sib = 4 * (log_l - d.cap_height) + sum(max(log_l - (k + 1) * d.fri_arity_bits - d.cap_height, 0) for k in range(lay["n_layers"]))
    assert sum(ln for _, ln in got) == 32 * ((3 + lay["n_layers"]) * (1 << d.cap_height) + d.fri_num_queries * n_sib)
    # nothing else is a digest: the openings, the rows, the cosets, the final polynomial, the tail
    covered = np.zeros(lay["total"], dtype=bool)
    for a, ln in got:
        covered[a:a + ln] = True
    for name_ in ("openings", "final_poly", "pow_witness", "num_public_inputs", "public_inputs"):
        a, ln = lay[name_]
        assert not covered[a:a + ln].any(), name_
    for q in lay["query"]:
        for sp in q["row"] + q["path_len"] + [ly["evals"] for ly in q["layer"]] + [ly["path_len"] for ly in q["layer"]]:
            assert not covered[sp[0]:sp[0] + sp[1]].any()
    if name == "layer-inside-cap":
        assert lay["query"][0]["layer"][1]["path"][1] == 0     # a layer without siblings adds no range


def test_wrapper_model_follows_the_replay_verifier(stored):
    """on the stored proof and on changes of it: the wrapper says ACCEPT exactly where cm.verify returns, names the reason of
    cm.verify's refusal where it refuses, and calls MALFORMED what the structural rules refuse before the replay"""
    s = stored
    proof, lay, sh, c = s["proof"], s["lay"], s["sh"], s["c"]
    cm.verify(proof, sh, s["digest"], s["cap"])
    a = vm.classify(proof, lay, sh, s["digest"], s["cap"], c.ref.verify(c.proof))
    assert a.accepted and a.reason == vm.ACCEPT
    assert vm.classify(proof, lay, sh, s["digest"], s["cap"], 1, c.pis).accepted
    assert vm.classify(proof, lay, sh, s["digest"], s["cap"], 1, c.pis[:-1] + [(c.pis[-1] + 1) % P]).reason == vm.PUBLIC_INPUTS
    Q = lay["query"][0]
    top = (R >> 192) + 1
    changes = {
        "row": (flip(proof, Q["row"][1][0] + 3), vm.TRACE_PATH, dict(query=0, tree=1)),
        "sibling": (flip(proof, Q["path"][2][0] + 40), vm.TRACE_PATH, dict(query=0, tree=2)),
        "sibling word >= p": (proof[:Q["path"][3][0] + 16] + b"\xff" * 8 + proof[Q["path"][3][0] + 24:], vm.TRACE_PATH, dict(query=0, tree=3)),
        "sibling >= r": (proof[:Q["path"][0][0] + 24] + top.to_bytes(8, "little") + proof[Q["path"][0][0] + 32:], vm.MALFORMED, {}),
        "cap >= r": (proof[:lay["cap"][2][0] + 56] + top.to_bytes(8, "little") + proof[lay["cap"][2][0] + 64:], vm.MALFORMED, {}),
        "row word >= p": (proof[:Q["row"][0][0]] + b"\xff" * 8 + proof[Q["row"][0][0] + 8:], vm.MALFORMED, {}),
        "path-length byte": (flip(proof, Q["path_len"][3][0], 2), vm.MALFORMED, dict(query=0, tree=3)),
        "count word": (flip(proof, lay["num_public_inputs"][0]), vm.MALFORMED, {}),
        "cut": (proof[:-1], vm.MALFORMED, {}),
    }
    for name, (bad, want, place) in changes.items():
        a = vm.classify(bad, lay, sh, s["digest"], s["cap"], 0)   # a twin code that is neither "accepts" nor "constraints"
        assert not a.accepted and a.reason == want, (name, a)
        for k, v in place.items():
            assert getattr(a, k) == v, (name, a)
        with pytest.raises(cm.Reject):
            cm.verify(bad, sh, s["digest"], s["cap"])
        if want == vm.TRACE_PATH:
            assert a.x_index == cm.replay(bad, sh, s["digest"])["query_indices"][0]
    # one query and no proof of work: a flipped final-polynomial coefficient that keeps the query index reaches its own check
    at = lay["final_poly"][0]
    index = cm.replay(proof, sh, s["digest"])["query_indices"][0]
    found = None
    for byte in range(64):
        bad = flip(proof, at + byte, 1)
        if cm.replay(bad, sh, s["digest"])["query_indices"][0] == index:
            found = bad
            break
    if found is not None:
        assert vm.classify(found, lay, sh, s["digest"], s["cap"], 0).reason == vm.FINAL_POLY
    # the vanishing identity is the twin's to decide, and comes before the replay
    assert vm.classify(flip(proof, lay["wires"][0] + 1), lay, sh, s["digest"], s["cap"], vm.ORACLE_CONSTRAINTS).reason == vm.CONSTRAINTS
    with pytest.raises(AssertionError):
        vm.classify(flip(proof, Q["row"][1][0] + 3), lay, sh, s["digest"], s["cap"], 1)   # the references would contradict


@pytest.fixture(scope="module")
def digest_words_check(tmp_path_factory):
    """tests/tools/digest_words_check.cpp built with -fsanitize=address,undefined; skipped where a trivial program does not link
    that way"""
    tmp = tmp_path_factory.mktemp("digest_words_check")
    trivial = tmp / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    san = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    try:
        r = subprocess.run(san + [str(trivial), "-o", str(tmp / "trivial")], capture_output=True)
        ok = r.returncode == 0 and subprocess.run([str(tmp / "trivial")], capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip("no g++ with AddressSanitizer here")
    exe = tmp / "digest_words_check"
    r = subprocess.run(san + [os.path.join(ROOT, "tests", "tools", "digest_words_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _findings(proof, lay, plb, digest_spans):
    """(finding, staging word) of the parser in Goldilocks mode - the rule of the code before the hasher existed: every word a
    field word - and in BN128 mode, for a proof of the right length, from Python's layout alone"""
    n_pis = lay["public_inputs"][1] // 8
    at = lay["num_public_inputs"][0]
    if int.from_bytes(proof[at:at + 8], "little") != n_pis:
        return (2, 0), (2, 0)
    for q in lay["query"]:
        for ln, path in list(zip(q["path_len"], q["path"])) + [(ly["path_len"], ly["path"]) for ly in q["layer"]]:
            if proof[ln[0]] != path[1] // 32:
                return (3, 0), (3, 0)
    # the staging buffer: the proof without its path-length bytes
    keep = np.ones(len(proof), dtype=bool)
    keep[sorted(plb)] = False
    raw = np.frombuffer(proof, dtype=np.uint8)[keep]
    words = np.frombuffer(raw.tobytes(), dtype="<u8")
    big = np.nonzero(words >= np.uint64(P))[0]
    gold = (4, int(big[0])) if big.size else (0, 0)
    first = None
    staged_at = np.cumsum(keep) - 1                           # byte offset in the proof -> byte offset in the staging buffer
    is_digest = np.zeros(words.size, dtype=bool)
    for a, ln in digest_spans:
        w0 = int(staged_at[a]) // 8
        is_digest[w0:w0 + ln // 8] = True
        for k in range(ln // 32):
            v = sum(int(words[w0 + 4 * k + j]) << (64 * j) for j in range(4))
            if v >= R and (first is None or w0 + 4 * k < first):
                first = w0 + 4 * k
    big_field = [int(i) for i in big if not is_digest[i]]
    if big_field and (first is None or big_field[0] < first):
        first = big_field[0]
    return gold, ((4, first) if first is not None else (0, 0))


def test_digest_word_rule_under_sanitizers(nlx, stored, digest_words_check, tmp_path):
    """The parser in both modes on the stored BN128 proof, on every truncation of it to a multiple of 8 bytes and to one byte
    either side, and on 4 000 seeded mutations - three byte flips, then a whole word set to all ones -: exit 0, nothing reported,
    only the untouched length is called sound, and every finding with its word index is the one Python's layout gives - in
    Goldilocks mode by the rule of the parser before it knew of hashers (the first word >= p, wherever it lies)."""
    s = stored
    proof, lay, c = s["proof"], s["lay"], s["c"]
    path = tmp_path / "proof.bin"
    path.write_bytes(proof)
    seed, n_mut = 33033, 4000
    r = subprocess.run([digest_words_check, str(path), str(seed), str(n_mut)] + shape_args(c.syn, lay), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    plb = path_length_bytes(lay)
    spans = [tuple(sp) for sp in lay["digests"]]
    gold0, bn0 = _findings(proof, lay, plb, spans)
    assert bn0 == (0, 0)                                       # the stored proof is sound under its own config
    assert lines[0] == "total %d" % len(proof) and lines[1] == "file %d %d" % (gold0[0], bn0[0])
    tried = sum(1 for t in range(len(proof)) if t % 8 in (0, 1, 7))
    assert lines[2] == "truncations %d sound 0 0" % tried
    muts = [ln.split() for ln in lines[3:] if ln]
    assert len(muts) == n_mut
    seen = set()
    for k, (_, off, kind, g_what, g_word, b_what, b_word) in enumerate(muts):
        seed = (seed * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        off, kind = int(off), int(kind)
        want_off = (seed >> 16) % len(proof)
        bad = bytearray(proof)
        if k % 4 == 3:
            want_off = min(want_off, len(proof) - 8)
            assert kind == 256
            bad[want_off:want_off + 8] = b"\xff" * 8
        else:
            assert kind == 1 + (seed >> 56) % 255
            bad[want_off] ^= kind
        assert off == want_off
        gold, bn = _findings(bytes(bad), lay, plb, spans)
        got_g = (int(g_what), int(g_word) if int(g_what) == 4 else 0)
        got_b = (int(b_what), int(b_word) if int(b_what) == 4 else 0)
        assert got_g == gold and got_b == bn, (k, off, kind, got_g, gold, got_b, bn)
        seen.add((gold[0], bn[0]))
    # sound in both; structure in both; a word both refuse; a digest word >= p that only the Goldilocks rule refuses; and a
    # digest >= r of words below p, or a word of ones that only ..., that only the BN128 rule refuses
    assert {(0, 0), (3, 3), (4, 4), (4, 0)} <= seen, seen
