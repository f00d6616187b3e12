"""Time of the Groth16 verifier for 1, 16, 64 and 256 proofs in one call, on a key without commitments and on one with one:
  python3 tools/groth16_verify_timing.py [--reps 5] [--warmup 2]
The key is the model's "public3" shape at 2^3 constraints (tools/groth16_model.py / groth16_commit_model.py; the verifier's work
depends on n_public and k only).  Per k and batch size:
  * each launch's device time by HIP events (ksum_ms: k_bn254_g16_ksum and its reduction; points_ms: the subgroup test of Bs;
    miller_ms; final_exp_ms), their sum device_ms, per call, the median call of --reps after --warmup, all in one process;
  * wall_ms: the whole call, host side included (decoding, the square roots, the hashes, the copies), median likewise;
  * model_ms: for scale only, the big-integer model's verifier (tools/bn254_pairing_model.py) on one proof.
The batch is the same proof n times - the verifier has no cache that could tell.  Writes profiles/groth16_verify_timing.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("bn254_groth16_ksum", "bn254_pairing_points", "bn254_pairing_miller", "bn254_pairing_final_exp")
BATCHES = (1, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nlxpkg
    from groth16_verify_cases import case
    nlx = nlxpkg.load()
    ctx = nlx.Context(0)
    out = {"protocol": "median call of %d after %d warm-up calls, one process; device times by HIP events per launch" % (args.reps, args.warmup),
           "shape": "public3, 2^3 constraints, n_public = 3", "results": []}
    for k in (0, 1):
        c = case("public3", 8, k)
        t0 = time.perf_counter()
        assert c.model_accepts(c.proof)
        model_ms = (time.perf_counter() - t0) * 1e3
        vk = c.verifying_key(nlx, ctx)
        res = {"k": k, "proof_bytes": len(c.proof), "model_ms": round(model_ms, 1)}
        for n in BATCHES:
            proofs, publics = [c.proof] * n, [c.public] * n
            dev, wall = [], []
            for rep in range(args.warmup + args.reps):
                ctx.kernel_timing(True)
                t0 = time.perf_counter()
                vs = vk.verify_many(proofs, publics)
                w = (time.perf_counter() - t0) * 1e3
                parts = [ctx.kernel_stats(name)[1] for name in KERNELS]
                assert all(v.accepted for v in vs)
                if rep >= args.warmup:
                    dev.append(parts)
                    wall.append(w)
            ctx.kernel_timing(False)
            totals = [sum(p) for p in dev]
            mid = dev[totals.index(statistics.median_low(totals))]
            res["n%d" % n] = {"device_ms": round(sum(mid), 3), "ksum_ms": round(mid[0], 3), "points_ms": round(mid[1], 3),
                              "miller_ms": round(mid[2], 3), "final_exp_ms": round(mid[3], 3),
                              "device_ms_per_proof": round(sum(mid) / n, 3), "device_ms_min_max": [round(min(totals), 3), round(max(totals), 3)],
                              "wall_ms": round(statistics.median(wall), 3), "wall_ms_per_proof": round(statistics.median(wall) / n, 3)}
            print("k=%d n=%d %s" % (k, n, json.dumps(res["n%d" % n])), flush=True)
        vk.close()
        out["results"].append(res)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
