"""CPU tests of the plonky2 verifier's host side: argument checks that run before any device call, the verdict's Python mirror,
the proof layout computed from the descriptor, and the layout header's parser under a sanitizer (a stand-alone program: nothing
loaded into Python runs under one).  nlx_verifier_proof_bytes needs a verifier, which needs a device: tests/test_gpu_plonk_verify.py
compares it with the same lengths; here the stand-alone program prints the header's own total."""
import ctypes
import os
import subprocess

import pytest

from conftest import P, ROOT
from plonk_verify_cases import ALL_CASES, SANITIZER_CASES, case, path_length_bytes, shape_args, word_at


def test_verify_abi_rejects_null(nlx):
    """NULL arguments come back as NLX_E_INVAL before any device call, and the verdict is zero-filled first"""
    d = nlx.lib.dll
    v = nlx.stark.Verdict(1, 2, 3, 4, 5, 6, 7)
    buf = ctypes.create_string_buffer(64)
    assert d.nlx_verify(None, buf, 64, None, ctypes.byref(v)) == -1
    assert (v.accepted, v.reason, v.challenge, v.query, v.tree, v.layer, v.x_index) == (0,) * 7
    assert d.nlx_verify(None, None, 0, None, None) == -1
    vs = (nlx.stark.Verdict * 2)()
    vs[1].reason = 9
    assert d.nlx_verify_batch(None, None, None, 2, None, vs) == -1
    assert vs[1].reason == 0
    assert d.nlx_verifier_proof_bytes(None) == 0
    h = ctypes.c_void_p()
    assert d.nlx_verifier_from_circuit(None, ctypes.byref(h)) == -1 and not h.value
    assert d.nlx_verifier_create(None, None, None, None, ctypes.byref(h)) == -1 and not h.value
    d.nlx_verifier_destroy(None)


def test_verdict_mirror(nlx):
    """nlx_proof_verdict is nlx_stark_verdict: one Python Verdict serves both verifiers"""
    text = open(os.path.join(ROOT, "include", "nlx.h")).read()
    assert "typedef nlx_stark_verdict nlx_proof_verdict;" in text
    V = nlx.stark.Verdict
    assert ctypes.sizeof(V) == 32 and V.x_index.offset == 24
    assert [f[0] for f in V._fields_] == ["accepted", "reason", "challenge", "query", "tree", "layer", "x_index"]
    bad = V(0, nlx.stark.VERIFY_CONSTRAINTS, 1)
    assert not bad.ok and bad.reason_name == "constraints"
    with pytest.raises(ValueError):
        bad.raise_if_rejected()
    assert nlx.VerifierData is nlx.plonk.VerifierData and callable(nlx.plonk.proof_layout)
    assert hasattr(nlx.CircuitData, "verify") and hasattr(nlx.CircuitData, "verify_many") and hasattr(nlx.CircuitData, "verifier_data")


@pytest.mark.parametrize("name", ALL_CASES)
def test_layout_total_is_the_oracle_proofs_length(nlx, orc, name):
    c = case(nlx, orc, name)
    proof = c.proof
    assert c.ref.verify(proof) == 1
    lay = nlx.plonk.proof_layout(c.syn)
    assert lay["total"] == len(proof)
    d = c.syn.desc()
    # the parts tile the proof, and the words the layout names are where the oracle put them
    assert lay["caps"] == (0, 3 * (32 << d.cap_height))
    assert lay["openings"][0] == lay["caps"][1] and lay["constants"][0] == lay["openings"][0]
    assert lay["quotient"][0] + lay["quotient"][1] == lay["fri_caps"][0]
    assert lay["query"][0]["row"][0][0] == lay["fri_caps"][0] + lay["fri_caps"][1]
    last = lay["query"][-1]["layer"][-1]["path"] if lay["n_layers"] else lay["query"][-1]["path"][-1]
    assert last[0] + last[1] == lay["final_poly"][0]
    assert lay["public_inputs"][0] + lay["public_inputs"][1] == lay["total"]
    at = lay["num_public_inputs"][0]
    assert int.from_bytes(proof[at:at + 8], "little") == d.num_public_inputs
    at = lay["public_inputs"][0]
    assert [int.from_bytes(proof[at + 8 * i:at + 8 * i + 8], "little") for i in range(d.num_public_inputs)] == c.pis
    for q in (lay["query"][0], lay["query"][-1]):
        for t in range(4):
            assert proof[q["path_len"][t][0]] == d.degree_bits + d.rate_bits - d.cap_height
        for k in range(lay["n_layers"]):
            assert proof[q["layer"][k]["path_len"][0]] == q["layer"][k]["path"][1] // 32
    if name == "layer-inside-cap":
        assert [ly["path"][1] for ly in lay["query"][0]["layer"]] == [64, 0]
    if name == "rows5":
        assert lay["n_layers"] == 0 and lay["final_poly"][1] == 16 * 32
    if name.startswith("lookup"):
        assert lay["lookup_zs"][1] > 0 and lay["lookup_zs"][1] == lay["lookup_zs_next"][1]
    else:
        assert lay["lookup_zs"][1] == 0
    # the constants' openings are observed first: the wires cap, then the openings, as the descriptor counts them
    assert lay["wires"][1] == 16 * d.num_wires and lay["sigmas"][1] == 16 * d.num_routed_wires


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    """tests/tools/layout_check.cpp built with -fsanitize=address,undefined; skipped where a trivial program does not link
    that way"""
    tmp = tmp_path_factory.mktemp("plonk_layout_check")
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


@pytest.mark.parametrize("name", SANITIZER_CASES)
def test_layout_parser_under_sanitizers(nlx, orc, layout_check, tmp_path, name):
    """The parser on an oracle proof, on every truncation of it to a multiple of 8 bytes and to one byte either side, and on
    4 000 seeded byte mutations (enough to land on the few path-length bytes): exit 0, nothing reported, the header's total is the
    proof's length, only the untouched length is called sound, and every mutation is judged as the Python layout says - a
    path-length byte and the public-input count are structure, a field word is structure only once it is >= p."""
    c = case(nlx, orc, name)
    proof = c.proof
    lay = nlx.plonk.proof_layout(c.syn)
    path = tmp_path / "proof.bin"
    path.write_bytes(proof)
    seed, n_mut = 29000 + len(name), 4000
    r = subprocess.run([layout_check, "plonk", str(path), str(seed), str(n_mut)] + shape_args(c.syn, lay), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[0] == "total %d" % len(proof) and lines[1] == "file 0"
    tried = sum(1 for t in range(len(proof)) if t % 8 in (0, 1, 7))
    assert lines[2] == "truncations %d sound 0" % tried
    plb = path_length_bytes(lay)
    muts = [ln.split() for ln in lines[3:] if ln]
    assert len(muts) == n_mut
    kinds = set()
    for _, off, x, got in muts:
        seed = (seed * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        off, x, got = int(off), int(x), int(got)
        assert off == (seed >> 16) % len(proof) and x == 1 + (seed >> 56) % 255
        if lay["num_public_inputs"][0] <= off < lay["num_public_inputs"][0] + 8:
            want = 2
        elif off in plb:
            want = 3
        else:
            w0, word = word_at(proof, off, plb)
            want = 4 if word ^ (x << (8 * (off - w0))) >= P else 0
        assert got == want, (off, x, got, want)
        kinds.add(want)
    assert 0 in kinds and 3 in kinds
