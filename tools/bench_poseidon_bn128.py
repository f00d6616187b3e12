#!/usr/bin/env python3
"""Throughput of PoseidonBN128 on the GPU (csrc/poseidon_bn128.hip): prints ONE JSON line.

  * perms_per_s: nlx_poseidon_bn128_permute_batch on 2^22 device-resident random states (in place; the call synchronises);
  * per commitment shape (135 columns x 2^16 rows and 20 columns x 2^18 rows, rate_bits 3, cap_height 4): the BN128 commitment
    and the Goldilocks commitment of the same device-resident random input, measured in the same run: the median over --reps of
    the device-event time of the library's kernels (nlx_ctx_kernel_timing: intt + lde + leaf hashing + Merkle levels) and of the
    wall time of the whole call.

Warm-up calls (--warmup) precede every measured series.  Kernel-level statistics come from a separate run under
rocprofv3 --kernel-trace --stats (profiles/README.md).

Usage: python tools/bench_poseidon_bn128.py [--reps 5] [--warmup 2] [--log-states 22]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import nlxpkg  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GL_P = 0xFFFFFFFF00000001
KERNELS = {"poseidon_goldilocks": ("intt", "lde", "hash_lde_leaves", "merkle_levels"),
           "poseidon_bn128": ("intt", "lde", "hash_lde_leaves_bn128", "merkle_levels_bn128")}


def random_states(rng, n):
    """n random canonical states as (n, 4, 4) words: top word below r's (every element < r)"""
    w = rng.integers(0, 2**63, size=(n, 4, 4), dtype=np.uint64) * np.uint64(2)
    w[:, :, 3] %= np.uint64(R >> 192)
    return w


def bench_permute(nlx, ctx, log_states, reps, warmup):
    import torch
    rng = np.random.default_rng(1)
    n = 1 << log_states
    dev = torch.from_numpy(random_states(rng, n).view(np.int64)).to("cuda")
    dll = nlx.lib.dll
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        ctx.check(dll.nlx_poseidon_bn128_permute_batch(ctx.handle, dev.data_ptr(), n))
        t = time.perf_counter() - t0
        if i >= warmup:
            times.append(t)
    return n / statistics.median(times), statistics.median(times) * 1e3


def bench_commit(nlx, ctx, n_cols, log_n, rate_bits, cap_height, reps, warmup):
    import torch
    rng = np.random.default_rng(2)
    vals = rng.integers(0, GL_P, size=(n_cols, 1 << log_n), dtype=np.uint64)
    dev = torch.from_numpy(vals.view(np.int64)).to("cuda")
    out = {}
    for hasher, names in KERNELS.items():
        dev_ms, wall_ms = [], []
        for i in range(warmup + reps):
            ctx.kernel_timing(True)   # clears the samples
            t0 = time.perf_counter()
            pb = nlx.PolynomialBatch.from_values(ctx, dev, rate_bits, cap_height, hasher=hasher)
            wall = time.perf_counter() - t0
            per = {k: ctx.kernel_stats(k)[1] for k in names}
            pb.close()
            if i >= warmup:
                dev_ms.append(sum(per.values()))
                wall_ms.append(wall * 1e3)
                last = per
        ctx.kernel_timing(False)
        out[hasher] = {"device_ms": round(statistics.median(dev_ms), 3), "wall_ms": round(statistics.median(wall_ms), 3),
                       "kernels_ms": {k: round(v, 3) for k, v in last.items()}}
    L = (1 << (log_n + rate_bits))
    bn = out["poseidon_bn128"]
    leaf_perms = L * ((n_cols + 8) // 9)
    bn["leaf_perms_per_s"] = round(leaf_perms / (bn["kernels_ms"]["hash_lde_leaves_bn128"] * 1e-3))
    out["bn128_over_goldilocks"] = round(bn["device_ms"] / out["poseidon_goldilocks"]["device_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-states", type=int, default=22)
    a = ap.parse_args()
    nlx = nlxpkg.load()
    ctx = nlx.Context(0)
    pps, ms = bench_permute(nlx, ctx, a.log_states, a.reps, a.warmup)
    res = {"tool": "bench_poseidon_bn128", "states": 1 << a.log_states, "perms_per_s": round(pps), "permute_ms": round(ms, 3),
           "reps": a.reps, "warmup": a.warmup, "commit": {}}
    for n_cols, log_n in ((135, 16), (20, 18)):
        res["commit"]["%dx2^%d_rate3" % (n_cols, log_n)] = bench_commit(nlx, ctx, n_cols, log_n, 3, 4, a.reps, a.warmup)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
