"""Wall and kernel time of the BN254 point codec (near-light-client_amd/bn254_codec.py: nlx_bn254_g1_decode / g2_decode / g1_encode /
g2_encode) and of the two containers that stand on it, in one process, medians of --runs after --warmup unrecorded calls:
  python3 tools/bn254_codec_timing.py --keys 14 20 --json profiles/bn254_codec_timing.json
  - decode and encode of 2^--log-g1 G1 and 2^--log-g2 G2 points (fixed-base multiples of the generators, resident on the device,
    the result left there), compressed and raw; G2 decode with and without the subgroup test
  - per key size 2^k constraints (the synthetic R1CS of tools/groth16_setup_timing.py): nlx_bn254_groth16_setup's time, then
    Setup.proving_key_bytes (the whole key written, bytes on the host) and ProvingKey.from_bytes (the whole key read and made
    resident), compressed and raw
  - the big-integer model's decode rate on this host (tools/gnark_bytes_model.py over --model-points points)
No test gates on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import nlxpkg
import bn254_py as bn
import gnark_bytes_model as gb

ap = argparse.ArgumentParser()
ap.add_argument("--log-g1", type=int, default=20)
ap.add_argument("--log-g2", type=int, default=18)
ap.add_argument("--keys", nargs="*", type=int, default=[14, 20])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--model-points", type=int, default=64)
ap.add_argument("--json", default=None)
opt = ap.parse_args()

nlx = nlxpkg.load()
import torch

G = nlx.bn254_groth16
R = G.R
ctx = nlx.Context(0)


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


def kernel_ms(fn, name):
    ctx.kernel_timing(True)
    fn()
    torch.cuda.synchronize()
    ms = round(ctx.kernel_stats(name)[1], 3)
    ctx.kernel_timing(False)
    return ms


def points_record(g2, log_n):
    n = 1 << log_n
    words = np.random.default_rng(log_n).integers(0, 1 << 62, (n, 4))
    words[:, 3] >>= 2                                                           # canonical integers below 2^252 < r
    scalars = torch.from_numpy(words.astype(np.int64)).cuda()
    points = (nlx.bn254_g2_scalar_muls if g2 else nlx.bn254_g1_scalar_muls)(ctx, bn.G2 if g2 else bn.G1, scalars, device="cuda:0")
    enc, dec = (nlx.bn254_g2_encode, nlx.bn254_g2_decode) if g2 else (nlx.bn254_g1_encode, nlx.bn254_g1_decode)
    name = "g2" if g2 else "g1"
    rec = {"group": name, "log_n": log_n}
    for raw in (False, True):
        mode = "raw" if raw else "compressed"
        data = enc(ctx, points, raw=raw)
        variants = [("decode", lambda: dec(ctx, data, raw=raw), "bn254_%s_decode" % name), ("encode", lambda: enc(ctx, points, raw=raw), "bn254_%s_encode" % name)]
        if g2:
            variants.append(("decode_no_subgroup", lambda: dec(ctx, data, raw=raw, subgroup=False), "bn254_g2_decode"))
        for what, call, kernel in variants:
            wall, runs = median_ms(call)
            k_ms = kernel_ms(call, kernel)
            rec["%s_%s" % (what, mode)] = {"call_ms": wall, "call_ms_runs": runs, "kernel_ms": k_ms, "points_per_s": round(n / (k_ms * 1e-3), 0)}
        back = dec(ctx, data, raw=raw)
        assert torch.equal(back, points), "decode(encode(points)) differs from the points"
    return rec


def r1cs(log_n, rng):
    """the synthetic R1CS of tools/groth16_setup_timing.py"""
    n = 1 << log_n
    n_free = 4
    other = rng.integers(1, n_free + np.arange(n), dtype=np.int64)
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


def key_record(log_n):
    n_wires, mats = r1cs(log_n, np.random.default_rng(log_n))
    td = G.Trapdoor.random()
    make = lambda: G.Setup(ctx, log_n, n_wires, 3, 1 << log_n, mats, td)
    setup_ms, setup_runs = median_ms(make, cleanup=lambda s: s.close())
    s = make()
    info = s.info()
    rec = {"log_n": log_n, "g1_points": info["g1_a"] + info["g1_b"] + info["g1_k"] + info["g1_z"] + 3, "g2_points": info["g1_b"] + 2,
           "setup_ms": setup_ms, "setup_ms_runs": setup_runs}
    for raw in (False, True):
        mode = "raw" if raw else "compressed"
        write_ms, write_runs = median_ms(lambda: s.proving_key_bytes(raw=raw))
        data = s.proving_key_bytes(raw=raw)
        read_ms, read_runs = median_ms(lambda: G.ProvingKey.from_bytes(ctx, data, r1cs=mats), cleanup=lambda k: k.close())
        ctx.kernel_timing(True)
        G.ProvingKey.from_bytes(ctx, data, r1cs=mats).close()
        torch.cuda.synchronize()
        decode_kernels = round(ctx.kernel_stats("bn254_g1_decode")[1] + ctx.kernel_stats("bn254_g2_decode")[1], 3)
        ctx.kernel_timing(False)
        rec[mode] = {"bytes": len(data), "write_ms": write_ms, "write_ms_runs": write_runs, "read_ms": read_ms, "read_ms_runs": read_runs,
                     "read_decode_kernels_ms": decode_kernels}
        del data
    s.close()
    return rec


def model_rate():
    rng = np.random.default_rng(1)
    ks = [int(x) for x in rng.integers(1, 1 << 62, opt.model_points)]
    out = {}
    for name, pts, dec, enc in (("g1", [bn.g1_mul(k, bn.G1) for k in ks], gb.g1_decode, gb.g1_encode),
                                ("g2", [bn.g2_mul(k, bn.G2) for k in ks], gb.g2_decode, gb.g2_encode)):
        for raw in (False, True):
            data = [enc(p, raw) for p in pts]
            t0 = time.perf_counter()
            for d in data:
                assert dec(d, raw)[0] == gb.OK
            out["%s_decode_%s_points_per_s" % (name, "raw" if raw else "compressed")] = round(len(data) / (time.perf_counter() - t0), 1)
    return out


model = model_rate()
print("model on this host:", model, flush=True)
points = [points_record(False, opt.log_g1), points_record(True, opt.log_g2)]
for rec in points:
    print(json.dumps(rec), flush=True)
keys = []
for log_n in opt.keys:
    keys.append(key_record(log_n))
    print(json.dumps(keys[-1]), flush=True)
if opt.json:
    with open(opt.json, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "runs": opt.runs, "warmup": opt.warmup, "points": points, "keys": keys, "model": model},
                  f, indent=1)
        f.write("\n")
