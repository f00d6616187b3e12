"""Time of the plonky2 verifier for 1, 16 and 64 proofs of one circuit in one call:
  python3 tools/plonk_verify_timing.py [--reps 5] [--warmup 2] [--log-n 12,16,18] [--timeout 600] [--hasher poseidon_bn128]
The nearx gate mix (bench.py GATE_MIXES["nearx"], 64 public inputs) at 2^12, 2^16 and 2^18 rows.  Per shape and batch size:
  * device_ms: the three launches' device time (HIP events around k_fri_paths, k_fri_queries and k_plonk_constraints), summed per
    call, median of --reps calls after --warmup; paths_ms / fri_ms / constraints_ms are its parts;
  * wall_ms: the whole call, host side included (parsing, the transcript, the copies), median likewise;
  * oracle_ms: for scale only, the oracle's one-thread host verifier (test infrastructure) on the same proof.
The proofs are the GPU prover's; the batch is the same proof n times - the verifier has no cache that could tell.
Every shape runs in a child process of its own under --timeout seconds, and the first one that fails ends the run.
Writes profiles/plonk_verify_timing.json.
--hasher poseidon_bn128: the same circuits under plonky2x's PoseidonBN128GoldilocksConfig at 2^12 and 2^16
rows; the path launch is then k_fri_paths_bn128 (timing name plonk_verify_paths_bn128), and per shape "paths_chain_perms" is the
longest tree's dependent chain of lane-split permutations, ceil(width / 9) + path_len.  There is no oracle_ms: the oracle's
verifier is the Goldilocks config's.  Writes profiles/plonk_verify_bn128_timing.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("plonk_verify_paths", "plonk_verify_fri", "plonk_verify_constraints")
BN128 = "poseidon_bn128"
BATCHES = (1, 16, 64)


def measure(log_n, args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import bench
    import nlxpkg
    import oracle_py as orc
    nlx = nlxpkg.load()
    ctx = nlx.Context(0)
    syn = nlx.SyntheticCircuit(log_n, seed=1000, num_public_inputs=64, **bench.GATE_MIXES["nearx"])
    bn128 = args.hasher == BN128
    kernels = ("plonk_verify_paths_bn128",) + KERNELS[1:] if bn128 else KERNELS
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=args.hasher)
    proof = cd.prove(syn.wires, syn.public_inputs)
    res = {"degree_bits": log_n, "gates": int(syn.num_gates), "proof_bytes": len(proof), "queries": int(syn.config.fri_num_queries)}
    if bn128:
        lay = nlx.plonk.proof_layout(cd)
        q0 = lay["query"][0]
        res["paths_chain_perms"] = max([-(-w // 9) + sp[1] // 32 for w, sp in zip(lay["tree_cols"], q0["path"])] +
                                       [-(-2 * lay["arity"] // 9) + ly["path"][1] // 32 for ly in q0["layer"]])
        res["paths_perms_per_query"] = (sum(-(-w // 9) + sp[1] // 32 for w, sp in zip(lay["tree_cols"], q0["path"])) +
                                        sum(-(-2 * lay["arity"] // 9) + ly["path"][1] // 32 for ly in q0["layer"]))
    t0 = time.perf_counter()
    first = cd.verify(proof)
    res["first_verify_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)   # with the verifier's construction
    assert first.ok, str(first)
    for n in BATCHES:
        proofs = [proof] * n
        dev, wall = [], []
        for rep in range(args.warmup + args.reps):
            ctx.kernel_timing(True)
            t0 = time.perf_counter()
            vs = cd.verify_many(proofs)
            w = (time.perf_counter() - t0) * 1e3
            parts = [ctx.kernel_stats(k)[1] for k in kernels]
            assert all(v.ok for v in vs)
            if rep >= args.warmup:
                dev.append(parts)
                wall.append(w)
        ctx.kernel_timing(False)
        totals = [sum(p) for p in dev]
        mid = dev[totals.index(statistics.median_low(totals))]
        res["n%d" % n] = {"device_ms": round(sum(mid), 4), "paths_ms": round(mid[0], 4), "fri_ms": round(mid[1], 4),
                          "constraints_ms": round(mid[2], 4), "device_ms_per_proof": round(sum(mid) / n, 4),
                          "device_ms_min_max": [round(min(totals), 4), round(max(totals), 4)],
                          "wall_ms": round(statistics.median(wall), 3), "wall_ms_per_proof": round(statistics.median(wall) / n, 3)}
    cd.close()
    ctx.close()
    if bn128:
        return res
    ref = orc.Circuit.from_synthetic(syn)    # the oracle commits the constants on one host thread first: not part of the figure
    t0 = time.perf_counter()
    assert ref.verify(proof) == 1
    res["oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    ref.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", default=None)
    ap.add_argument("--hasher", default="poseidon_goldilocks", choices=["poseidon_goldilocks", BN128])
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bn128 = args.hasher == BN128
    args.log_n = args.log_n or ("12,16" if bn128 else "12,16,18")
    args.out = args.out or os.path.join(ROOT, "profiles", "plonk_verify_bn128_timing.json" if bn128 else "plonk_verify_timing.json")
    if args.child:
        print("RESULT " + json.dumps(measure(args.child, args)), flush=True)
        return 0
    out = {"reps": args.reps, "warmup": args.warmup, "batches": list(BATCHES), "gate_mix": "nearx, 64 public inputs", "hasher": args.hasher,
           "unit": "ms; device = HIP events around the verifier's launches, wall = the whole call", "circuits": {}}
    for log_n in (int(x) for x in args.log_n.split(",")):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(log_n), "--reps", str(args.reps),
                            "--warmup", str(args.warmup), "--hasher", args.hasher], capture_output=True, text=True, timeout=args.timeout)
        line = next((ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            print("2^%d rows: the measuring process ended with status %d; stopping" % (log_n, r.returncode), file=sys.stderr)
            return 1
        out["circuits"]["nearx_2p%d" % log_n] = json.loads(line[7:])
        print("nearx_2p%d" % log_n, line[7:], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
