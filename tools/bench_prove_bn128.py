#!/usr/bin/env python3
"""Latency of the PoseidonBN128 Merkle levels and stage times of whole proofs under the BN128 config: prints ONE JSON line.

  * "levels": one Merkle level of 2^0 .. 2^18 parents (nlx_poseidon_bn128_merkle_build on 2 n device-resident four-word leaves -
    a four-word leaf is its own digest - with the cap at the parents, so exactly one level kernel runs), through the one-lane
    kernel (k_pbn_merkle_level, a context created with NLX_PBN_QUAD_MAX_PARENTS=0) and the lane-split kernel
    (k_pbn_merkle_level_quad, a context created with the variable at 2^30), interleaved in ONE process: per size the median and
    the minimum over --reps of the device-event time (nlx_ctx_kernel_timing, "merkle_levels_bn128") after --warmup calls.
  * "proofs": nlx_prove at degree_bits 13, 16 and 18 (standard config, the outer workload's gate mix), one stream: the device-event
    stage times (nlx_prove_stage_times, median over --reps after --warmup) under the BN128 config with the library's dispatch
    threshold, under the BN128 config with NLX_PBN_QUAD_MAX_PARENTS=0, and under the Goldilocks config on the same build; and
    the BN128 proof's hashing kernels (leaf and level times of the three proof commitments, the FRI commit phase).
  * --verify: the replay verifier (tools/bn128_config_model.py) checks the degree-13 BN128 proof.

Kernel-level statistics come from a separate run under rocprofv3 --kernel-trace --stats (profiles/README.md).

Usage: python tools/bench_prove_bn128.py [--reps 5] [--warmup 2] [--max-level-bits 18] [--degrees 13,16,18] [--verify]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import nlxpkg  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN, GOLD = "poseidon_bn128", "poseidon_goldilocks"
OUTER = dict(pct_poseidon=25, pct_arithmetic=20, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=10, pct_u32=15)
HASH_KERNELS = ("hash_lde_leaves_bn128", "merkle_levels_bn128", "fri_leaves_bn128", "fri_merkle_levels_bn128")


def context_with(nlx, quad_max):
    """a context whose dispatch threshold is `quad_max` (None: the library's constant); the variable is read at creation"""
    old = os.environ.pop("NLX_PBN_QUAD_MAX_PARENTS", None)
    if quad_max is not None:
        os.environ["NLX_PBN_QUAD_MAX_PARENTS"] = str(quad_max)
    try:
        return nlx.Context(0)
    finally:
        os.environ.pop("NLX_PBN_QUAD_MAX_PARENTS", None)
        if old is not None:
            os.environ["NLX_PBN_QUAD_MAX_PARENTS"] = old


def bench_levels(nlx, ctxs, max_bits, reps, warmup):
    import torch
    dll = nlx.lib.dll
    rng = np.random.default_rng(3)
    rows = []
    for bits in range(max_bits + 1):
        n = 1 << bits
        leaves = rng.integers(0, 2**63, size=(2 * n, 4), dtype=np.uint64)
        leaves[:, 3] %= np.uint64(R >> 192)
        dev = torch.from_numpy(leaves.view(np.int64)).to("cuda")
        cap = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        samples = {k: [] for k in ctxs}
        caps = {}
        for i in range(warmup + reps):
            for name, ctx in ctxs.items():   # interleaved: both kernels see the same clock and cache state
                ctx.kernel_timing(True)
                ctx.check(dll.nlx_poseidon_bn128_merkle_build(ctx.handle, dev.data_ptr(), 2 * n, 4, bits, None, cap.data_ptr()))
                ms = ctx.kernel_stats("merkle_levels_bn128")[1]
                ctx.kernel_timing(False)
                if i >= warmup:
                    samples[name].append(ms * 1e3)
                if i == 0:
                    caps[name] = cap.cpu().numpy().copy()
        assert all(np.array_equal(c, caps["one_lane"]) for c in caps.values()), "the two kernels disagree at 2^%d parents" % bits
        rows.append({"parents_log2": bits,
                     **{"%s_us" % k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                        for k, v in samples.items()}})
    return rows


def bench_proof(nlx, ctx, syn, hasher, reps, warmup):
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=hasher)
    stages, kernels, proof = [], None, None
    for i in range(warmup + reps):
        if i == warmup + reps - 1:
            ctx.kernel_timing(True)
        proof = cd.prove(syn.wires, syn.public_inputs)
        if i >= warmup:
            stages.append(dict(cd.stage_times()))
    if hasher == BN:
        kernels = {k: {"calls": ctx.kernel_stats(k)[0], "ms": round(ctx.kernel_stats(k)[1], 3), "perms": ctx.kernel_units(k)} for k in HASH_KERNELS}
    ctx.kernel_timing(False)
    med = {k: round(statistics.median(s[k] for s in stages), 3) for k in stages[0]}
    out = {"stage_ms": med, "total_ms": round(sum(med.values()), 3), "proof_bytes": len(proof)}
    if kernels:
        out["hash_kernels_last_proof"] = kernels
    cs_cap, digest = cd.constants_sigmas_cap, cd.circuit_digest
    cd.close()
    return out, proof, cs_cap, digest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-level-bits", type=int, default=18)
    ap.add_argument("--degrees", default="13,16,18")
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    nlx = nlxpkg.load()
    ctxs = {"default": context_with(nlx, None), "one_lane": context_with(nlx, 0), "quad": context_with(nlx, 1 << 30)}
    res = {"tool": "bench_prove_bn128", "reps": a.reps, "warmup": a.warmup,
           "levels": bench_levels(nlx, {k: ctxs[k] for k in ("one_lane", "quad")}, a.max_level_bits, a.reps, a.warmup), "proofs": {}}
    for log_n in [int(x) for x in a.degrees.split(",") if x]:
        syn = nlx.SyntheticCircuit(log_n, seed=1000, num_public_inputs=64, **OUTER)
        row = {}
        row["bn128"], proof, cs_cap, digest = bench_proof(nlx, ctxs["default"], syn, BN, a.reps, a.warmup)
        row["bn128_quad_off"], proof_off, _, _ = bench_proof(nlx, ctxs["one_lane"], syn, BN, a.reps, a.warmup)
        row["goldilocks"], _, _, _ = bench_proof(nlx, ctxs["default"], syn, GOLD, a.reps, a.warmup)
        row["proofs_byte_equal_between_dispatch_settings"] = proof == proof_off
        if a.verify and log_n == 13:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bn128_config_model as cm
            cap = [cm.m.from_words(w) for w in cs_cap]
            cm.verify(proof, cm.Shape.from_synthetic(syn), cm.m.from_words(digest), cap)
            row["replay_verifier_accepts"] = True
        res["proofs"]["2^%d" % log_n] = row
    for c in ctxs.values():
        c.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
