"""CPU tests: csrc/bn254_plonk_solve.hpp - the witness solver's schedule and per-item arithmetic, the text the kernels compile -
built with plain g++ (tests/native/bn254_plonk_solve_check.cpp) against the big-integer model tools/gnark_plonk_solve_model.py
on every circuit of tests/bn254_plonk_solve_cases.py: the schedule (level, form and assigned variable per constraint, the level
per hint), the solved vector word for word, ragged's failing inputs (kind, constraint, value, failures, poisoned variables and
which variables are poisoned) and every refusal with its index.  The program is built twice: plainly, and with
-fsanitize=address,undefined (that stand-alone binary is run; skipped where a trivial sanitized program does not link)."""
import os
import subprocess

import pytest

from conftest import ROOT

import bn254_plonk_solve_cases as cases

pm, R = cases.pm, cases.R
MONT = 1 << 256
SRC = os.path.join(ROOT, "tests", "native", "bn254_plonk_solve_check.cpp")
INCLUDE = os.path.join(ROOT, "near-light-client_amd", "csrc")


def hx(x):
    return "%064x" % x


def mont(x):
    return hx(x % R * MONT % R)


def circuit_lines(m, n_given, commit_values=()):
    """a model solver as the program reads it; the hints in running order"""
    skipped = [int(f == pm.SKIPPED) for f in m.form]
    order = sorted(range(len(m.hints)), key=lambda h: m.hints[h][1])          # stable: a commitment's hint after the listed ones
    lines = ["circuit %d %d %d %d" % (m.n_variables, n_given, len(m.constraints), len(order))]
    for con, q, sk in zip(m.constraints, m.q, skipped):
        lines.append("con %d %d %d %d %s" % (con[0], con[1], con[2], sk, " ".join(mont(v) for v in q)))
    for h in order:
        kind, before, ins, outs, param = m.hints[h]
        value = commit_values[param] if kind == pm.COMMIT else 0
        lines.append("hint %d %d %d %016x %s %d %s %d %s" % (h, kind, before, param, mont(value), len(ins), " ".join(map(str, ins)), len(outs),
                                                             " ".join(map(str, outs))))
    return lines, order


def sched_line(m, order):
    per = " ".join("%d %d %d" % t for t in zip(m.level, m.form, m.assigns))
    return "sched %s %s" % (per, " ".join(str(m.hint_level[h]) for h in order))


def run_line(inputs, values, first, failures, poisoned):
    kind, constraint, value = first if first else (0, pm.NONE, 0)
    return "run %s = %d %d %s %d %d %s" % (" ".join(mont(x) for x in inputs), kind, constraint, hx(value), failures, poisoned,
                                           " ".join("P" if v is None else mont(v) for v in values))


@pytest.fixture(scope="module")
def records():
    lines = []
    for name in cases.ALL:
        c, m = cases.case(name), cases.model(name)
        values, _, cs = cases.solved(name)
        head, order = circuit_lines(m, c.n_public + c.n_secret, cs)
        lines += head + [sched_line(m, order), run_line(c.inputs, values, None, 0, 0)]
        if name == "ragged":
            for inputs, _, _, _ in cases.failing(c).values():
                vals, first, failures, poisoned = m.solve(inputs, stop=False)
                lines.append(run_line(inputs, vals, first, failures, poisoned))
    for what, constraints, hints, where in cases.refusals():
        lines.append("circuit %d 2 %d %d" % (cases.REFUSAL_VARIABLES, len(constraints), len(hints)))
        for con in constraints:
            lines.append("con %d %d %d 0 %s" % (con[0], con[1], con[2], " ".join(mont(cases.REFUSAL_COEFFS[i]) for i in con[3:8])))
        for h, t in enumerate(hints):
            outs = [t[3]] if t[0] == "inv_zero" else list(t[3]) if t[0] == "n_bits" else [t[4], t[5]]
            lines.append("hint %d %d %d %016x %s 1 %d %d %s" % (h, pm.HINT_KINDS[t[0]], t[1], t[3] if t[0] == "quo_rem64" else 0, hx(0), t[2], len(outs),
                                                                " ".join(map(str, outs))))
        lines.append("refuse %d %d" % (where[0] == "hint", where[1]))
    text = "\n".join(lines) + "\n"
    return text, sum(line.startswith(("sched", "run", "refuse")) for line in lines)


def _build(tmp, name, extra):
    exe = tmp / name
    r = subprocess.run(["g++", "-std=c++17", "-I", INCLUDE] + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(exe, records, tmp):
    text, count = records
    path = tmp / "cases.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("%d cases, 0 bad" % count)


def test_the_records_reach_every_part(records):
    text, count = records
    assert count == 2 * len(cases.ALL) + 3 + len(cases.refusals())
    kinds = {int(line.split()[2]) for line in text.splitlines() if line.startswith("hint")}
    assert kinds == {pm.INV_ZERO, pm.N_BITS, pm.QUO_REM64, pm.COMMIT}
    assert any(" P " in line for line in text.splitlines() if line.startswith("run"))


def test_header_against_the_model(records, tmp_path):
    _run(_build(tmp_path, "bn254_plonk_solve_check", ["-O2"]), records, tmp_path)


def test_header_under_sanitizers(records, tmp_path):
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
    _run(_build(tmp_path, "bn254_plonk_solve_check_san", san), records, tmp_path)
