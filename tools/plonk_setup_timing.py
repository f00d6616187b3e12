"""Wall and kernel time of gnark's plonk.Setup on the device (near-light-client_amd/bn254_plonk.py Setup, kzg_srs) at 2^k gates of
the structured circuit (constraint c uses variables c, c + 1 and 7 c mod V; tests/bn254_plonk_setup_cases.py `structured`), beside
the same key made the old way: the trace on the host with numpy and Python integers, handed to ResidentKey.
  python3 tools/plonk_setup_timing.py 14 18 20 --json profiles/plonk_setup_timing.json
Per size: the setup call (rows, sort, permutation and sigma from the library's kernel timing; the rest of the wall time is the
host's validation of every id), nlx_bn254_plonk_setup_key, nlx_bn254_kzg_srs of n + 3 points, the host's trace and the
ResidentKey made from it, and the FIRST copy check of a setup-built key against that of a key_create key (which decodes s1 s2
s3 first).  --runs N --warmup W: medians over N runs after W unrecorded ones; first checks are single shots by nature."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import nlxpkg

ap = argparse.ArgumentParser()
ap.add_argument("log_n", nargs="*", type=int)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--old-way-max", type=int, default=20, help="largest log_n at which the host builds the trace too")
ap.add_argument("--json", default=None)
opt = ap.parse_args()

nlx = nlxpkg.load()
import torch

P = nlx.bn254_plonk
R = P.R
ctx = nlx.Context(0)
SETUP_KERNELS = ("bn254_plonk_setup_rows", "bn254_plonk_setup_sort", "bn254_plonk_setup_perm", "bn254_plonk_setup_sigma")
SRS_KERNELS = ("bn254_kzg_srs_powers", "bn254_fixed_base_table", "bn254_fixed_base_g1", "bn254_fixed_base_g2")
CHECK_KERNELS = ("bn254_plonk_sigma_decode", "bn254_plonk_check_copies")
MONT = (1 << 256) % R


def circuit(log_n):
    m = (1 << log_n) - 16
    v = m + 1
    c = np.arange(m, dtype=np.int64)
    cons = np.stack([c, c + 1, 7 * c % v, 3 + c % 8, 3 + (c >> 3) % 8, np.zeros(m, dtype=np.int64), 3 + (c >> 6) % 8, np.ones(m, dtype=np.int64)], axis=1)
    rng = np.random.default_rng(log_n)
    coeffs = [0, 1, R - 1] + [int(x) for x in rng.integers(2, 1 << 62, 8)]
    return v, 2, cons, coeffs


def words_of(ints):
    """Montgomery words of a list of integers: one to_bytes per element, one frombuffer for all"""
    return np.frombuffer(b"".join((x * MONT % R).to_bytes(32, "little") for x in ints), dtype=np.uint64).reshape(-1, 4)


def host_trace(log_n, n_public, cons, coeffs, k1=5, k2=25):
    """the rules of tools/gnark_plonk_setup_model.py with numpy where numpy reaches and Python integers for the field"""
    n, m = 1 << log_n, len(cons)
    cw = words_of(coeffs)
    values = {}
    for at, name in enumerate(("ql", "qr", "qm", "qo", "qk")):
        col = np.zeros((n, 4), dtype=np.uint64)
        col[n_public:n_public + m] = cw[cons[:, 3 + at]]
        values[name] = col
    values["ql"][:n_public] = cw[2]
    cells = np.zeros((3, n), dtype=np.int64)
    cells[0, :n_public] = np.arange(n_public)
    cells[:, n_public:n_public + m] = cons[:, :3].T
    flat = cells.reshape(-1)
    order = np.argsort(flat, kind="stable")
    keys = flat[order]
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    last = np.concatenate([first[1:], [True]])
    source = np.roll(order, 1)
    source[first] = order[last]            # classes appear in the same order among the firsts and the lasts
    perm = np.empty(3 * n, dtype=np.int64)
    perm[order] = source
    w = pow(pow(5, (R - 1) >> 28, R), 1 << (28 - log_n), R)
    ident, x = [], 1
    for _ in range(n):
        ident.append(x)
        x = x * w % R
    ident = words_of(ident + [k1 * t % R for t in ident] + [k2 * t % R for t in ident])
    sigma = ident[perm]
    values["s1"], values["s2"], values["s3"] = sigma[:n], sigma[n:2 * n], sigma[2 * n:]
    return values, perm


def median_ms(fn, cleanup=None):
    times = []
    for i in range(opt.warmup + opt.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= opt.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
        if cleanup:
            cleanup(out)
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def kernel_ms(fn, names):
    """per-kernel device time and call count of ONE call"""
    ctx.kernel_timing(True)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ms = {name: round(ctx.kernel_stats(name)[1], 3) for name in names}
    calls = {name: ctx.kernel_stats(name)[0] for name in names}
    ctx.kernel_timing(False)
    return ms, calls, round(wall, 3), out


records = []
for log_n in opt.log_n or [14]:
    n = 1 << log_n
    n_variables, n_public, cons, coeffs = circuit(log_n)
    tau = 0x1234567 + log_n
    srs_ms, srs_runs = median_ms(lambda: P.kzg_srs(ctx, tau, n + 3, device="cuda:0"))
    srs_kernels, _, _, (g1, _, _) = kernel_ms(lambda: P.kzg_srs(ctx, tau, n + 3, device="cuda:0"), SRS_KERNELS)
    make = lambda: P.Setup(ctx, n_variables, n_public, cons, coeffs, log_n=log_n)
    setup_ms, setup_runs = median_ms(make, cleanup=lambda s: s.close())
    kernels, _, _, s = kernel_ms(make, SETUP_KERNELS)
    info = s.info()
    key_ms, key_runs = median_ms(lambda: s.key(g1), cleanup=lambda k: k.close())
    rec = {"log_n": log_n, "n_constraints": len(cons), "n_variables": n_variables, "info": info, "kzg_srs_ms": srs_ms, "kzg_srs_ms_runs": srs_runs,
           "kzg_srs_kernels_ms": srs_kernels, "setup_ms": setup_ms, "setup_ms_runs": setup_runs, "setup_kernels_ms": kernels,
           "setup_key_ms": key_ms, "setup_key_ms_runs": key_runs, "runs": opt.runs, "warmup": opt.warmup}
    # the first copy check: wires gathered from random variable values satisfy every copy
    rng = np.random.default_rng(1)
    vals = rng.integers(0, 1 << 62, (n_variables, 4))
    vals[:, 3] >>= 2
    l, r, o = s.wires(torch.from_numpy(vals.astype(np.int64)).cuda())
    key = s.key(g1)
    ms, calls, wall, rep = kernel_ms(lambda: P.check_resident(key, l, r, o, what=P.CHECK_COPIES), CHECK_KERNELS)
    assert rep.satisfied == 1 and calls["bn254_plonk_sigma_decode"] == 0 and rep.cache_bytes == 12 * n
    rec["first_copy_check_setup_key"] = {"wall_ms": wall, "kernels_ms": ms, "decode_calls": calls["bn254_plonk_sigma_decode"]}
    later, _ = median_ms(lambda: P.check_resident(key, l, r, o, what=P.CHECK_COPIES))
    rec["later_copy_check_ms"] = later
    key.close()
    if log_n <= opt.old_way_max:
        t0 = time.perf_counter()
        values, perm = host_trace(log_n, n_public, cons, coeffs)
        rec["host_trace_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert np.array_equal(perm, s.read("permutation").astype(np.int64)) and np.array_equal(values["s3"], s.read("s3")) \
            and np.array_equal(values["qo"], s.read("qo"))
        old_ms, old_runs = median_ms(lambda: P.ResidentKey(ctx, values, g1, 5, 25), cleanup=lambda k: k.close())
        rec["resident_key_from_host_values_ms"], rec["resident_key_from_host_values_ms_runs"] = old_ms, old_runs
        old = P.ResidentKey(ctx, values, g1, 5, 25)
        ms, calls, wall, rep = kernel_ms(lambda: P.check_resident(old, l, r, o, what=P.CHECK_COPIES), CHECK_KERNELS)
        assert rep.satisfied == 1 and calls["bn254_plonk_sigma_decode"] == 1
        rec["first_copy_check_key_create_key"] = {"wall_ms": wall, "kernels_ms": ms, "decode_calls": calls["bn254_plonk_sigma_decode"]}
        old.close()
    s.close()
    records.append(rec)
    print(json.dumps(rec), flush=True)

print("| gates | kzg_srs (n + 3) | setup call | rows | sort | perm | sigma | setup_key | host trace | ResidentKey (host values) | first copy check, setup key | first copy check, key_create key |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for rec in records:
    k = rec["setup_kernels_ms"]
    old = rec.get("first_copy_check_key_create_key", {}).get("wall_ms", "-")
    print("| 2^%d | %.1f | %.1f | %.2f | %.2f | %.2f | %.2f | %.1f | %s | %s | %.2f | %s |" % (
        rec["log_n"], rec["kzg_srs_ms"], rec["setup_ms"], k[SETUP_KERNELS[0]], k[SETUP_KERNELS[1]], k[SETUP_KERNELS[2]], k[SETUP_KERNELS[3]],
        rec["setup_key_ms"], rec.get("host_trace_ms", "-"), rec.get("resident_key_from_host_values_ms", "-"),
        rec["first_copy_check_setup_key"]["wall_ms"], old))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "unit": "ms", "records": records}, f, indent=1)
        f.write("\n")
