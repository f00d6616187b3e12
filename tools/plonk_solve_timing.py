#!/usr/bin/env python3
"""Times nlx_bn254_plonk_solver_solve and writes profiles/plonk_solve_timing.json.

    python tools/plonk_solve_timing.py 14 18 20

Per log2 size, three solvable circuits of about 2^log_n constraints, all O-form unless said:
  wide    depth 20, constant divisors (qo = -1)
  deep    a chain of depth n / 4, width 4 - run fused and with one launch per level (NO_FUSE) in the same session
  mixed   wide with 5 % value-dependent divisors (L-form, qm != 0)
One process; per figure the median of 3 solves after a warm-up, wall clock around the call with device inputs and outputs, plus
the library's event timing per kernel name from one more solve.  Against: the native check program's sequential loop over the
same header (g++ -O2, one core of this host; up to 2^18, the records are text) and the Python model at 2^14.  At 2^18 and 2^20 also
the solve's share of solve + wires + prove on the wide circuit.  First values: no thresholds."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_py as bn  # noqa: E402
import gnark_plonk_solve_model as pm  # noqa: E402

R = bn.R
N_INPUTS, N_PUBLIC = 16, 2
ZERO, ONE, MINUS_ONE, POOL0, N_POOL = 0, 1, 2, 3, 12


def circuit(kind, log_n, seed=39):
    """-> (constraints (m, 8) int64, coeffs, n_variables)"""
    rng = np.random.default_rng(seed + log_n)
    coeffs = [0, 1, R - 1] + [int.from_bytes(rng.bytes(31), "little") + 1 for _ in range(N_POOL)]
    m = (1 << log_n) - N_PUBLIC - 2
    width = 4 if kind == "deep" else -(-m // 20)
    cons = np.zeros((m, 8), dtype=np.int64)
    new = N_INPUTS + np.arange(m)
    level_start = np.arange(m) // width * width                      # the first constraint of this one's level
    prev_lo = np.where(level_start == 0, 0, N_INPUTS + level_start - width)
    prev_n = np.where(level_start == 0, N_INPUTS, width)
    a = prev_lo + rng.integers(0, 1 << 30, m) % prev_n               # an operand of the previous level
    if kind == "deep":
        a = np.where(level_start == 0, np.arange(m) % N_INPUTS, new - width)
    b = rng.integers(0, N_INPUTS, m)
    cons[:, 0], cons[:, 1], cons[:, 2] = a, b, new
    cons[:, 3:6] = POOL0 + rng.integers(0, N_POOL, (m, 3))
    cons[:, 6], cons[:, 7] = MINUS_ONE, POOL0 + rng.integers(0, N_POOL, m)
    if kind == "mixed":
        lform = rng.random(m) < 0.05                                  # l = new from r = a, o = b: the divisor is ql + qm a
        cons[lform, 0], cons[lform, 1], cons[lform, 2] = new[lform], a[lform], b[lform]
        cons[lform, 6] = POOL0 + rng.integers(0, N_POOL, int(lform.sum()))
    return cons, coeffs, N_INPUTS + m


def median_seconds(fn, sync, reps=3):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def native_seconds(exe, cons, coeffs, n_variables, inputs):
    hexes = ["%064x" % (c % R * (1 << 256) % R) for c in coeffs]
    lines = ["circuit %d %d %d 0" % (n_variables, N_INPUTS, len(cons))]
    lines += ["con %d %d %d 0 %s %s %s %s %s" % (c[0], c[1], c[2], hexes[c[3]], hexes[c[4]], hexes[c[5]], hexes[c[6]], hexes[c[7]]) for c in cons.tolist()]
    lines.append("run " + " ".join("%064x" % (x % R * (1 << 256) % R) for x in inputs))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        r = subprocess.run([exe, "--time", f.name], capture_output=True, text=True, check=True)
    finally:
        os.unlink(f.name)
    return float(r.stdout.split()[0])


def main(sizes):
    import torch
    import nlxpkg
    nlx = nlxpkg.load()
    P = nlx.bn254_plonk
    ctx = nlx.Context(0)
    sync = torch.cuda.synchronize
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "bn254_plonk_solve_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "bn254_plonk_solve_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(1)
    inputs = [int.from_bytes(rng.bytes(31), "little") for _ in range(N_INPUTS)]
    words = torch.from_numpy(nlx.bn254_pack([[bn.to_montgomery(x) for x in inputs]])[0].view(np.int64)).to("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "fuse": P.SOLVER_FUSE, "conditions": "one process; medians of 3 after a warm-up; wall clock around "
              "Solver.solve with device inputs and outputs; kernel_ms: the library's event timing of one further solve", "rows": []}
    out = os.path.join(ROOT, "profiles", "plonk_solve_timing.json")
    for log_n in sizes:
        for kind in ("wide", "deep", "mixed"):
            cons, coeffs, nv = circuit(kind, log_n)
            setup = P.Setup(ctx, nv, N_PUBLIC, cons, coeffs, log_n=log_n)
            row = {"log_n": log_n, "circuit": kind, "constraints": len(cons)}
            for fuse in ((True, False) if kind == "deep" else (True,)):
                solver = setup.solver(N_INPUTS - N_PUBLIC, fuse=fuse)
                info = solver.info()
                values, rep = solver.solve(words)
                rep.raise_if_unsolved()
                tag = "fused" if fuse else "no_fuse"
                row[tag + "_ms"] = 1e3 * median_seconds(lambda: solver.solve(words), sync)
                row[tag + "_launches"], row["levels"], row["value_divisors"] = info["launches"], info["levels"], info["value_divisors"]
                if fuse or info["launches"] <= 1 << 12:            # an event pair per launch: not for 2^16 launches and more
                    ctx.kernel_timing(True)
                    solver.solve(words)
                    row[tag + "_kernel_ms"] = {name: round(ctx.kernel_stats("bn254_plonk_solve_" + name)[1], 4) for name in ("levels", "fused", "commit")}
                    ctx.kernel_timing(False)
                if fuse and log_n <= 18:
                    row["native_one_core_ms"] = 1e3 * native_seconds(exe, cons, coeffs, nv, inputs)
                if fuse and log_n == 14:
                    t0 = time.perf_counter()
                    model = pm.Solver(nv, N_PUBLIC, N_INPUTS - N_PUBLIC, cons.tolist(), coeffs)
                    got, failure = model.solve(inputs)
                    row["python_model_ms"] = 1e3 * (time.perf_counter() - t0)
                    assert failure is None and np.array_equal(values.cpu().numpy().view(np.uint64), nlx.bn254_pack([[bn.to_montgomery(v) for v in got]])[0])
                if fuse and kind == "wide" and log_n >= 18:
                    g1, _, _ = P.kzg_srs(ctx, 12345, (1 << log_n) + 3, device="cuda:0")
                    key = setup.key(g1)
                    l, r, o = setup.wires(values)
                    pubs = inputs[:N_PUBLIC]
                    blind = list(range(1, 10))
                    row["wires_ms"] = 1e3 * median_seconds(lambda: setup.wires(values), sync)
                    row["prove_ms"] = 1e3 * median_seconds(lambda: P.prove_resident(key, l, r, o, pubs, blind), sync)
                    row["solve_share"] = row["fused_ms"] / (row["fused_ms"] + row["wires_ms"] + row["prove_ms"])
                    key.close()
                    del g1
                solver.close()
            setup.close()
            ctx.trim()
            print(json.dumps(row), flush=True)
            result["rows"].append(row)
            with open(out, "w") as f:                                # after every row: a run cut short keeps what it measured
                json.dump(result, f, indent=1)
                f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or [14, 18, 20])
