"""Time of the PLONK verifier over BN254 for 1 and 256 proofs in one call, k = 0 and k = 1 Bsb22 commitments, at log_n = 5, and of
the segmented G1 combination against the Groth16 verifier's public sum on the same number of segments and terms:
  python3 tools/bn254_plonk_verify_timing.py [--reps 5] [--warmup 2]
The protocol is tools/groth16_verify_timing.py's: the median call of --reps after --warmup, all in one process, each launch's
device time by HIP events.  Per k and batch size:
  * lincomb_a_ms, lincomb_b_ms, miller_ms, final_exp_ms, their sum device_ms, and wall_ms: the whole call, host side included
    (decoding, square roots, SHA-256, the scalars, two round trips);
  * model_ms: for scale only, the big-integer model's verifier (tools/gnark_plonk_verify_model.py) on one proof.
The kernel's parent figure: the Groth16 verifier's "bn254_groth16_ksum" sample (k_bn254_g16_ksum and its one-lane-per-segment
reduction) on a key whose n_public is combination B's left segment, 18 + 2 k terms, for 1 and 256 proofs; against one
"bn254_g1_lincomb" launch over as many segments of as many terms (random scalars, as the public inputs are).
The batch is the same proof n times - the verifier has no cache that could tell.  Writes profiles/bn254_plonk_verify_timing.json."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("bn254_plonk_verify_lincomb_a", "bn254_plonk_verify_lincomb_b", "bn254_pairing_miller", "bn254_pairing_final_exp")
BATCHES = (1, 256)


def median_call(ctx, call, names, warmup, reps):
    dev, wall = [], []
    for rep in range(warmup + reps):
        ctx.kernel_timing(True)
        t0 = time.perf_counter()
        call()
        w = (time.perf_counter() - t0) * 1e3
        parts = [ctx.kernel_stats(name)[1] for name in names]
        if rep >= warmup:
            dev.append(parts)
            wall.append(w)
    ctx.kernel_timing(False)
    totals = [sum(p) for p in dev]
    return dev[totals.index(statistics.median_low(totals))], totals, statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn254_plonk_verify_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nlxpkg
    from bn254_plonk_verify_cases import R, bn, case
    import groth16_model as g16m
    nlx = nlxpkg.load()
    ctx = nlx.Context(0)
    out = {"protocol": "median call of %d after %d warm-up calls, one process; device times by HIP events per launch" % (args.reps, args.warmup),
           "shape": "log_n = 5, n_public = 2", "parent": "none for the verifier: the capability is new (profiles/groth16_verify_timing.json for scale)",
           "results": [], "kernel": []}
    for k in (0, 1):
        c = case(5, k)
        t0 = time.perf_counter()
        assert c.model_verdict(c.proof)[0]
        model_ms = (time.perf_counter() - t0) * 1e3
        vk = c.verifying_key(nlx, ctx)
        res = {"k": k, "proof_bytes": len(c.proof), "model_ms": round(model_ms, 1)}
        for n in BATCHES:
            proofs, publics = [c.proof] * n, [c.public] * n

            def call():
                assert all(v.accepted for v in vk.verify_many(proofs, publics))
            mid, totals, wall = median_call(ctx, call, KERNELS, args.warmup, args.reps)
            res["n%d" % n] = {"device_ms": round(sum(mid), 3), "lincomb_a_ms": round(mid[0], 3), "lincomb_b_ms": round(mid[1], 3),
                              "miller_ms": round(mid[2], 3), "final_exp_ms": round(mid[3], 3), "device_ms_per_proof": round(sum(mid) / n, 3),
                              "device_ms_min_max": [round(min(totals), 3), round(max(totals), 3)], "wall_ms": round(wall, 3),
                              "wall_ms_per_proof": round(wall / n, 3)}
            print("k=%d n=%d %s" % (k, n, json.dumps(res["n%d" % n])), flush=True)
        vk.close()
        out["results"].append(res)
    # the kernel against its parent
    rng = random.Random(32)
    for k in (0, 1):
        terms = 18 + 2 * k
        inst = g16m.Instance(8, rng, n_public=terms)
        td = g16m.Trapdoor.random(rng)
        pk, gvk = g16m.setup(inst, td)
        pts = g16m.prove_by_logs(inst, td, inst.witness, rng.randrange(R), rng.randrange(R))
        data = g16m.proof_bytes(*pts)
        g2 = lambda p: nlx.bn254_g2_pack([p])[0]
        key = nlx.bn254_groth16.VerifyingKey(ctx, n_public=inst.n_public, g1_alpha=nlx.bn254_g1_pack([pk["g1_alpha"]])[0], g2_beta=g2(pk["g2_beta"]),
                                             g2_gamma=g2(gvk["g2_gamma"]), g2_delta=g2(pk["g2_delta"]), ic=nlx.bn254_g1_pack(gvk["ic"]))
        public = list(inst.witness[1:inst.n_public])
        base = nlx.bn254_g1_pack([bn.g1_mul(rng.randrange(1, R), bn.G1) for _ in range(terms)])
        row = {"k": k, "terms_per_segment": terms}
        for n in BATCHES:
            def parent():
                assert all(v.accepted for v in key.verify_many([data] * n, [public] * n))
            mid, totals, _ = median_call(ctx, parent, ("bn254_groth16_ksum",), args.warmup, args.reps)
            points = np.tile(base, (n, 1))
            scalars = nlx.bn254_pack([[rng.randrange(R) for _ in range(n * terms)]])[0]
            first = [terms * i for i in range(n + 1)]

            def new():
                nlx.bn254_g1_lincomb(ctx, points, scalars, first)
            mid2, totals2, _ = median_call(ctx, new, ("bn254_g1_lincomb",), args.warmup, args.reps)
            row["n%d" % n] = {"groth16_ksum_ms": round(mid[0], 3), "groth16_ksum_ms_min_max": [round(min(totals), 3), round(max(totals), 3)],
                              "g1_lincomb_ms": round(mid2[0], 3), "g1_lincomb_ms_min_max": [round(min(totals2), 3), round(max(totals2), 3)]}
            print("kernel k=%d n=%d %s" % (k, n, json.dumps(row["n%d" % n])), flush=True)
        key.close()
        out["kernel"].append(row)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
