"""Wall and kernel time of gnark's groth16.Setup from a trapdoor on the device (near-light-client_amd/bn254_groth16.py Setup) at 2^k
constraints, and the rate of the two fixed-base kernels on their own.  The R1CS is synthetic (a setup needs no witness): every
row of A carries ONE and one other wire, B one or two wires, C the row's own new wire - ONE's column has 2^k terms (the
wave-per-wire path), every other wire a few.
  python3 tools/groth16_setup_timing.py 14 18 20 --json profiles/groth16_setup_timing.json
Per size: the setup call (scalar side, the G1 and G2 launches and the tables from the library's kernel timing; the rest of the
wall time is the host's validation and index lists), the key build (nlx_bn254_groth16_setup_key), and for comparison the
big-integer model's fixed-base rate on this host (tools/groth16_model.py g1_gen_mul / g2_gen_mul over --model-points scalars).
--runs N --warmup W: medians over N runs after W unrecorded ones."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import nlxpkg
import groth16_model as gm

ap = argparse.ArgumentParser()
ap.add_argument("log_n", nargs="*", type=int)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--model-points", type=int, default=200)
ap.add_argument("--json", default=None)
opt = ap.parse_args()

nlx = nlxpkg.load()
import torch

G = nlx.bn254_groth16
R = G.R
ctx = nlx.Context(0)
KERNELS = ("bn254_groth16_setup_scalars", "bn254_fixed_base_table", "bn254_fixed_base_g1", "bn254_fixed_base_g2")


def r1cs(log_n, rng):
    n = 1 << log_n
    n_free = 4
    other = rng.integers(1, n_free + np.arange(n), dtype=np.int64)             # a wire that exists when the row is reached
    a_wire = np.stack([np.zeros(n, dtype=np.int64), other], axis=1).reshape(-1)
    b_count = rng.integers(1, 3, n)
    b_ptr = np.concatenate([[0], np.cumsum(b_count)])
    b_wire = rng.integers(1, n_free + np.repeat(np.arange(n), b_count), dtype=np.int64)
    c_wire = n_free + np.arange(n)
    coeffs = G.fr_pack([1, R - 1] + [int(x) for x in rng.integers(2, 1 << 62, 10)])
    ids = lambda count: rng.integers(0, len(coeffs), count).astype(np.uint32)
    return n_free + n, {"A": (np.arange(0, 2 * n + 1, 2, dtype=np.uint64), a_wire.astype(np.uint32), ids(2 * n)),
                        "B": (b_ptr.astype(np.uint64), b_wire.astype(np.uint32), ids(len(b_wire))),
                        "C": (np.arange(n + 1, dtype=np.uint64), c_wire.astype(np.uint32), ids(n)), "coeffs": coeffs}


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


def kernel_ms(fn):
    """per-kernel device time of ONE call"""
    ctx.kernel_timing(True)
    out = fn()
    torch.cuda.synchronize()
    ms = {name: round(ctx.kernel_stats(name)[1], 3) for name in KERNELS}
    ctx.kernel_timing(False)
    return ms, out


def model_rate():
    rng = np.random.default_rng(1)
    ks = [int(a) | (int(b) << 64) | (int(c) << 128) | (int(d) << 190) for a, b, c, d in rng.integers(0, 1 << 62, (opt.model_points, 4))]
    gm.g1_gen_mul(1), gm.g2_gen_mul(1)                                          # the model's own tables
    out = {}
    for name, fn in (("g1", gm.g1_gen_mul), ("g2", gm.g2_gen_mul)):
        t0 = time.perf_counter()
        for k in ks:
            fn(k)
        out[name + "_points_per_s"] = round(len(ks) / (time.perf_counter() - t0), 1)
    return out


records = []
model = model_rate()
print("model on this host: %.0f G1 and %.0f G2 fixed-base multiples per second" % (model["g1_points_per_s"], model["g2_points_per_s"]), flush=True)
for log_n in opt.log_n or [14]:
    rng = np.random.default_rng(log_n)
    n_wires, mats = r1cs(log_n, rng)
    td = G.Trapdoor.random()
    make = lambda: G.Setup(ctx, log_n, n_wires, 3, 1 << log_n, mats, td)
    setup_ms, setup_all = median_ms(make, cleanup=lambda s: s.close())
    kernels, s = kernel_ms(make)
    info = s.info()
    key_ms, key_all = median_ms(s.key, cleanup=lambda k: k.close())
    s.close()
    # the two kernels on their own: n scalars resident on the device, the result left there
    n = 1 << log_n
    words = rng.integers(0, 1 << 62, (n, 4))
    words[:, 3] >>= 2                                                           # canonical integers below 2^252 < r
    scalars = torch.from_numpy(words.astype(np.int64)).cuda()
    rate = {}
    for name, fn, base in (("g1", nlx.bn254_g1_scalar_muls, gm.bn.G1), ("g2", nlx.bn254_g2_scalar_muls, gm.bn.G2)):
        call = lambda: fn(ctx, base, scalars, device="cuda:0")
        wall, _ = median_ms(call)
        k_ms, _ = kernel_ms(call)
        rate[name] = {"call_ms": wall, "table_ms": k_ms["bn254_fixed_base_table"], "kernel_ms": k_ms["bn254_fixed_base_" + name],
                      "points_per_s": round(n / (k_ms["bn254_fixed_base_" + name] * 1e-3), 0)}
    g1_points = info["g1_a"] + info["g1_b"] + info["g1_k"] + info["g1_z"] + 3 + info["ic"]
    rec = {"log_n": log_n, "n_wires": n_wires, "g1_points": g1_points, "g2_points": info["g1_b"] + 3, "wave_wires": info["wave_wires"],
           "setup_ms": setup_ms, "setup_ms_runs": setup_all, "setup_kernels_ms": kernels, "key_build_ms": key_ms, "key_build_ms_runs": key_all,
           "fixed_base": rate, "model": model, "runs": opt.runs, "warmup": opt.warmup}
    records.append(rec)
    print("2^%d constraints: setup %.1f ms (scalars %.1f, tables %.1f, G1 %.1f for %d points, G2 %.1f for %d points), key build %.1f ms; "
          "fixed base alone: G1 %.2e points/s, G2 %.2e points/s" % (
              log_n, setup_ms, kernels[KERNELS[0]], kernels[KERNELS[1]], kernels[KERNELS[2]], g1_points, kernels[KERNELS[3]], rec["g2_points"],
              key_ms, rate["g1"]["points_per_s"], rate["g2"]["points_per_s"]), flush=True)
if opt.json:
    with open(opt.json, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)
        f.write("\n")
