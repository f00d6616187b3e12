"""Wall time of a whole gnark-shaped PLONK proof over BN254: prove_gnark (the Python orchestration over a ProvingKey, wires as
host integers - the only form it takes) against prove_resident (one library call on a ResidentKey, wires as device tensors)
without and with the fixed polynomials' coset values resident.  The key is the structured one of tools/plonk_prove_timing.py
(all selectors zero but the commitments' rows, random wires, the identity permutation, an SRS of distinct points): no
big-integer model at these sizes.
  python3 tools/plonk_resident_timing.py [--sizes 18 20] [--commitments 0 1] [--groups 3] [--per-group 4] [--limit 900]
Every configuration (size, k) runs in a child process of its own under its own time limit; a configuration that fails or runs
out of time ends the run.  Per prover: the median of groups x per-group proofs after one warm-up, and the medians of the groups -
their max - min is the run-to-run spread the comparison is read against.  Writes profiles/plonk_resident_timing.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = ("commit", "wires", "z", "quotient", "evals", "open")


def child(log_n, K, groups, per_group):
    import numpy as np
    sys.path.insert(0, ROOT)
    import nlxpkg
    nlx = nlxpkg.load()
    import torch
    P = nlx.bn254_plonk
    R = P.R
    ctx = nlx.Context(0)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    w = P.root_of_unity(log_n)
    ident, x = [], 1
    for _ in range(n):
        ident.append(x)
        x = x * w % R
    vals = {k: [0] * n for k in ("ql", "qr", "qm", "qo", "qk")}
    vals.update(s1=ident, s2=[5 * v % R for v in ident], s3=[25 * v % R for v in ident])
    info = [{"committed": list(range(j * n // 8, (j + 1) * n // 8)), "row": n // 2 + j, "last_row": n - 1} for j in range(K)]
    for j, c in enumerate(info):
        vals["qcp%d" % j] = [0] * n
        for i in c["committed"] + [c["row"]]:
            vals["ql"][i] = R - 1
        for i in c["committed"]:
            vals["qcp%d" % j][i] = 1
    srs = nlx.bn254_g1_multiples(ctx, (1, 2), n + 3, device="cuda:0")
    pk = P.ProvingKey(ctx, vals, srs, 5, 25, commitments=info)
    on_dev = {name: pk.value(name) for name in pk.NAMES}
    on_dev.update({"qcp%d" % j: pk.qcp_values[j] for j in range(K)})
    keys = {coset: P.ResidentKey(ctx, on_dev, srs, 5, 25, commitments=info, coset=coset) for coset in (False, True)}
    l, r, o = ([int(v) for v in rng.integers(0, 2 ** 62, n)] for _ in range(3))
    cb = [int(v) for v in rng.integers(1, 2 ** 62, 2 * K)]
    to_dev = lambda col: torch.from_numpy(nlx.bn254_pack([[P._to_mont(v) for v in col]])[0].view(np.int64)).cuda()
    dev = [to_dev(c) for c in (l, r, o)]
    for j in range(K):   # the hint once: the resident prover then takes finished wires, as a solver hands them over
        c = P.commit_resident(keys[False], j, dev[0], cb[2 * j:2 * j + 2])[1]
        dev[0][info[j]["row"]] = to_dev([c])[0]

    def witness(cs):
        for j, c in enumerate(cs):
            l[info[j]["row"]] = c
        return l, r, o
    provers = {
        "prove_gnark": (lambda: P.prove_gnark(pk, public_inputs=(), commit_blinding=cb, witness=witness)) if K else (lambda: P.prove_gnark(pk, l, r, o)),
        "prove_resident": lambda: P.prove_resident(keys[False], dev[0], dev[1], dev[2], commit_blinding=cb if K else None),
        "prove_resident_coset": lambda: P.prove_resident(keys[True], dev[0], dev[1], dev[2], commit_blinding=cb if K else None),
    }
    blind = [int(v) for v in rng.integers(1, 2 ** 62, 9)]
    fixed = [P.prove_resident(keys[c], dev[0], dev[1], dev[2], blinding=blind, commit_blinding=cb if K else None) for c in (False, True)]
    record = {"log_n": log_n, "commitments": K, "groups": groups, "per_group": per_group, "same_bytes_with_and_without_coset": fixed[0] == fixed[1],
              "resident_bytes": {str(c): keys[c].info()["resident_bytes"] for c in (False, True)}}
    for name, fn in provers.items():
        proof = fn()   # warm-up
        torch.cuda.synchronize()
        medians, every = [], []
        for _ in range(groups):
            times = []
            for _ in range(per_group):
                t0 = time.perf_counter()
                proof = fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            medians.append(statistics.median(times))
            every += times
        record[name] = {"median_ms": round(statistics.median(every), 3), "group_medians_ms": [round(m, 3) for m in medians],
                        "spread_ms": round(max(medians) - min(medians), 3), "min_ms": round(min(every), 3), "max_ms": round(max(every), 3),
                        "proof_bytes": len(proof)}
        if name != "prove_gnark":   # the rounds' device time, from two more proofs outside the timed ones
            ctx.kernel_timing(True)
            fn(), fn()
            rounds = {}
            for rd in ROUNDS:
                calls, ms, _ = ctx.kernel_stats("bn254_plonk_prove_" + rd)
                rounds[rd] = round(ms / calls, 3) if calls else None
            record[name]["round_ms"] = rounds
            ctx.kernel_timing(False)
    print("RECORD " + json.dumps(record), flush=True)
    for key in keys.values():
        key.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[18, 20])
    ap.add_argument("--commitments", nargs="*", type=int, default=[0, 1])
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--per-group", type=int, default=4)
    ap.add_argument("--limit", type=float, default=900.0, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_resident_timing.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args()
    if opt.child:
        return child(opt.child[0], opt.child[1], opt.groups, opt.per_group)
    if opt.groups * opt.per_group < 10:
        sys.exit("at least ten proofs per prover")
    records = []
    for log_n in opt.sizes:
        for K in opt.commitments:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(log_n), str(K), "--groups", str(opt.groups), "--per-group", str(opt.per_group)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=opt.limit)
            except subprocess.TimeoutExpired:
                sys.exit("2^%d gates, %d commitments: no result within %.0f s - stopping here" % (log_n, K, opt.limit))
            line = [x for x in res.stdout.splitlines() if x.startswith("RECORD ")]
            if res.returncode or not line:
                sys.exit("2^%d gates, %d commitments: the child ended with status %d - stopping here\n%s" % (log_n, K, res.returncode, res.stderr[-2000:]))
            rec = json.loads(line[0][7:])
            records.append(rec)
            print("2^%d gates, k = %d: prove_gnark %.1f ms (spread %.1f), prove_resident %.1f ms (spread %.1f), with coset values %.1f ms (spread %.1f)" % (
                log_n, K, rec["prove_gnark"]["median_ms"], rec["prove_gnark"]["spread_ms"], rec["prove_resident"]["median_ms"],
                rec["prove_resident"]["spread_ms"], rec["prove_resident_coset"]["median_ms"], rec["prove_resident_coset"]["spread_ms"]), flush=True)
            with open(opt.out, "w") as f:
                json.dump({"tool": "tools/plonk_resident_timing.py", "unit": "ms of wall time per proof", "records": records}, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
