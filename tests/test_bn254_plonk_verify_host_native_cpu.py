"""CPU tests: the PLONK verifier's host half, csrc/bn254_plonk_verify_host.hpp, built with plain g++
(tests/native/bn254_plonk_verify_host_check.cpp) against vectors the big-integer model writes (tools/gnark_plonk_verify_model.py):
the verdict and index of honest and tampered proofs, the four challenges, the scalars of the device's combinations, gamma' and
lambda.  The lambda rule is restated here from include/nlx.h with hashlib.  The program is built twice: plainly, and with
-fsanitize=address,undefined (that stand-alone binary is run; skipped where a trivial sanitized program does not link)."""
import os
import subprocess

import pytest

from bn254_plonk_verify_cases import MALFORMED, R, bn, case, gm, vm
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "bn254_plonk_verify_host_check.cpp")
INCLUDE = os.path.join(ROOT, "near-light-client_amd", "csrc")
FOLD_DST = b"nlx-plonk-kzg-fold"


def hx(x):
    return "%064x" % (x % R)


def fold_lambda(zeta, gp, z, hb, hz, v_f, zw):
    msg = bn.fr_bytes(zeta) + bn.fr_bytes(gp) + bn.g1_marshal(z) + bn.g1_marshal(hb) + bn.g1_marshal(hz) + bn.fr_bytes(v_f) + bn.fr_bytes(zw)
    return gm.hash_to_field(msg, FOLD_DST) or 1


def lines_of(c):
    k = c.k
    out = ["key %d %d %d %s %s %s %s" % (c.log_n, len(c.public), k, hx(c.inst.k1), hx(c.inst.k2), " ".join(str(i) for i in c.vk["commit_rows"]),
                                        " ".join(bn.g1_compress(p).hex() for p in c.key_commitments() + [bn.G1]))]
    out[0] = " ".join(out[0].split())
    w = bn.root_of_unity(c.log_n)
    for label, data, public in [("honest", c.proof, c.public)] + [t[:3] for t in c.tampers()]:
        accepted, reason, index = c.model_verdict(data, public)
        head = "proof %s %s =" % (data.hex(), " ".join(hx(x) for x in public))
        head = " ".join(head.split())
        if reason == MALFORMED:
            out.append("%s %d %d" % (head, reason, index))
            continue
        proof = gm.proof_from_bytes(data)
        t = vm.derive(proof, c.vk, c.n, c.inst.k1, c.inst.k2, public)
        if not t["relation"]:
            out.append("%s %d 0" % (head, vm.ALGEBRAIC))
            continue
        out.append("%s 0 0 %s" % (head, " ".join(hx(t[x]) for x in ("gamma", "beta", "alpha", "zeta", "zn2")) + " " + hx(t["sc"]["z"]) + " " + hx(t["sc"]["s3"])))
        zw = proof["z_shifted"]["value"]
        lam = fold_lambda(t["zeta"], t["gp"], proof["z"], proof["batched"]["h"], proof["z_shifted"]["h"], t["v_f"], zw)
        out.append("fold %s %s = %s %s %s %s %s %d" % (bn.g1_compress(t["folded_h_digest"]).hex(), bn.g1_compress(t["lin_digest"]).hex(), hx(t["gp"]), hx(lam),
                                                      hx(t["v_f"]), hx(-(t["v_f"] + lam * zw)), hx(lam * t["zeta"] * w), 20 + 2 * k))
    return out


@pytest.fixture(scope="module")
def cases():
    lines = []
    for log_n, k, n_pi in ((3, 0, 2), (3, 1, 2), (4, 2, 0), (5, 4, 2)):
        lines += lines_of(case(log_n, k, n_pi))
    assert sum(1 for x in lines if x.startswith("fold")) >= 4 * 3      # the honest proof and the two PAIRING tampers of every case
    return "\n".join(lines) + "\n"


def _build(tmp, name, extra):
    exe = tmp / name
    r = subprocess.run(["g++", "-std=c++17", "-I", INCLUDE] + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(exe, cases, tmp):
    path = tmp / "cases.txt"
    path.write_text(cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("%d cases, 0 bad" % cases.count("\n"))


def test_host_half_against_the_model(cases, tmp_path):
    _run(_build(tmp_path, "bn254_plonk_verify_host_check", ["-O2"]), cases, tmp_path)


def test_host_half_under_sanitizers(cases, tmp_path):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    try:
        r = subprocess.run(["g++", "-std=c++17"] + san + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True)
        ok = r.returncode == 0 and subprocess.run([str(tmp_path / "trivial")], capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip("a trivial program does not link with -fsanitize=address,undefined here")
    _run(_build(tmp_path, "bn254_plonk_verify_host_check_san", san), cases, tmp_path)
