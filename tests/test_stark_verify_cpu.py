"""CPU tests of the STARK verifier's host side: argument checks that run before any device call, the verdict's Python mirror, the
proof layout computed from the descriptor, and the layout header's parser under a sanitizer (a stand-alone program: nothing
loaded into Python runs under one)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import P, ROOT
from stark_verify_cases import ALL_CASES, case


def test_verify_abi_rejects_null(nlx):
    """NULL arguments come back as NLX_E_INVAL before any device call, and the verdict is zero-filled first"""
    d = nlx.lib.dll
    v = nlx.stark.Verdict(1, 2, 3, 4, 5, 6, 7)
    buf = ctypes.create_string_buffer(64)
    assert d.nlx_stark_verify(None, buf, 64, None, ctypes.byref(v)) == -1
    assert (v.accepted, v.reason, v.challenge, v.query, v.tree, v.layer, v.x_index) == (0,) * 7
    assert d.nlx_stark_verify(None, None, 0, None, None) == -1
    vs = (nlx.stark.Verdict * 2)()
    vs[1].reason = 9
    assert d.nlx_stark_verify_batch(None, None, None, 2, None, vs) == -1
    assert vs[1].reason == 0
    assert d.nlx_stark_proof_bytes(None) == 0


def test_verdict_mirror(nlx):
    S = nlx.stark
    assert ctypes.sizeof(S.Verdict) == 32 and S.Verdict.x_index.offset == 24
    assert len(S.VERIFY_REASON_NAMES) == 9
    names = [S.Verdict(0, r).reason_name for r in range(9)]
    assert len(set(names)) == 9 and "?" not in names and S.Verdict(0, 9).reason_name == "?"
    assert (S.VERIFY_ACCEPT, S.VERIFY_MALFORMED, S.VERIFY_PUBLIC_INPUTS, S.VERIFY_CONSTRAINTS, S.VERIFY_POW, S.VERIFY_TRACE_PATH,
            S.VERIFY_FRI_FOLD, S.VERIFY_FRI_PATH, S.VERIFY_FINAL_POLY) == tuple(range(9))
    # the header's numbers
    text = open(os.path.join(ROOT, "include", "nlx.h")).read()
    for code, macro in enumerate(("ACCEPT", "MALFORMED", "PUBLIC_INPUTS", "CONSTRAINTS", "POW", "TRACE_PATH", "FRI_FOLD", "FRI_PATH",
                                  "FINAL_POLY")):
        assert "#define NLX_VERIFY_%s" % macro in text
        assert int(text.split("#define NLX_VERIFY_%s" % macro)[1].split()[0]) == code
    ok = S.Verdict(1, 0)
    assert ok.ok and ok.raise_if_rejected() is ok and "verifies" in str(ok)
    bad = S.Verdict(0, S.VERIFY_FRI_PATH, 0, 17, 0, 2, 99)
    assert not bad.ok and "FRI path" in str(bad) and "17" in str(bad)
    with pytest.raises(ValueError):
        bad.raise_if_rejected()


@pytest.mark.parametrize("name", ALL_CASES)
def test_layout_total_is_the_oracle_proofs_length(nlx, orc, name):
    c = case(nlx, orc, name)
    proof = c.oracle_proof(orc)
    assert orc.stark_verify(c.st.desc, proof) == 1
    lay = nlx.stark.proof_layout(c.st)
    assert lay["total"] == len(proof)
    # the parts tile the proof, and the words the layout names are where the oracle put them
    d = c.st.desc
    assert lay["caps"] == (0, (32 << d.cap_height) * len(lay["oracle_cols"]))
    assert lay["query"][0]["row"][0][0] == lay["fri_caps"][0] + lay["fri_caps"][1]
    last = lay["query"][-1]["layer"][-1]["path"] if lay["n_layers"] else lay["query"][-1]["path"][-1]
    assert last[0] + last[1] == lay["final_poly"][0]
    assert lay["round_values"][0] + lay["round_values"][1] == lay["total"]
    at = lay["num_public_inputs"][0]
    assert int.from_bytes(proof[at:at + 8], "little") == d.num_public_inputs
    at = lay["public_inputs"][0]
    assert [int.from_bytes(proof[at + 8 * i:at + 8 * i + 8], "little") for i in range(d.num_public_inputs)] == [int(v) for v in c.pis]
    for q in (lay["query"][0], lay["query"][-1]):
        for o in range(len(lay["oracle_cols"])):
            assert proof[q["path_len"][o][0]] == d.degree_bits + d.rate_bits - d.cap_height
        for k in range(lay["n_layers"]):
            assert proof[q["layer"][k]["path_len"][0]] == q["layer"][k]["path"][1] // 32


def _shape_args(st, lay):
    d = st.desc
    return [str(int(x)) for x in (d.degree_bits, d.rate_bits, d.cap_height, d.fri_arity_bits, d.fri_final_poly_bits, d.fri_num_queries,
                                  d.n_cols, d.num_challenges * d.quotient_degree_factor, d.num_public_inputs,
                                  lay["round_values"][1] // 8)] + [str(w) for w in lay["oracle_cols"]]


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    """tests/tools/layout_check.cpp built with -fsanitize=address,undefined; skipped where a trivial program does not link
    that way"""
    tmp = tmp_path_factory.mktemp("layout_check")
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
    exe = tmp / "layout_check"
    r = subprocess.run(san + [os.path.join(ROOT, "tests", "tools", "layout_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("name", ["fib7-nondefault", "fingerprint", "wide16-batch12"])
def test_layout_parser_under_sanitizers(nlx, orc, layout_check, tmp_path, name):
    """The parser on an oracle proof, on every truncation of it to a multiple of 8 bytes and to one byte either side, and on
    1 000 seeded byte mutations: exit 0, nothing reported, only the untouched length called sound, and every mutation judged as
    the Python layout says - a path-length byte and the public-input count are structure, a field word is structure only once
    it is >= p."""
    c = case(nlx, orc, name)
    proof = c.oracle_proof(orc)
    lay = nlx.stark.proof_layout(c.st)
    path = tmp_path / "proof.bin"
    path.write_bytes(proof)
    seed, n_mut = 20240 + len(name), 1000
    r = subprocess.run([layout_check, "stark", str(path), str(seed), str(n_mut)] + _shape_args(c.st, lay), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[0] == "total %d" % len(proof) and lines[1] == "file 0"
    tried = sum(1 for t in range(len(proof)) if t % 8 in (0, 1, 7))
    assert lines[2] == "truncations %d sound 0" % tried
    # what a mutation at `off` must be called
    path_len_at = {}
    for q in lay["query"]:
        for sp in q["path_len"] + [ly["path_len"] for ly in q["layer"]]:
            path_len_at[sp[0]] = True
    muts = [ln.split() for ln in lines[3:] if ln]
    assert len(muts) == n_mut
    kinds = set()
    for _, off, x, got in muts:
        seed = (seed * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        off, x, got = int(off), int(x), int(got)
        assert off == (seed >> 16) % len(proof) and x == 1 + (seed >> 56) % 255
        if lay["num_public_inputs"][0] <= off < lay["num_public_inputs"][0] + 8:
            want = 2
        elif off in path_len_at:
            want = 3
        else:
            # the word the byte is part of: words start right after a path-length byte, or at the start of the proof
            start = max([0] + [b + 1 for b in path_len_at if b < off])
            w0 = off - (off - start) % 8
            word = int.from_bytes(proof[w0:w0 + 8], "little") ^ (x << (8 * (off - w0)))
            want = 4 if word >= P else 0
        assert got == want, (off, x, got, want)
        kinds.add(want)
    assert 0 in kinds and 3 in kinds
