"""Wall time of a whole PLONK proof over BN254 on the device (near-light-client_amd/bn254_plonk.py) at 2^k gates.  The instance is the
cheapest satisfying one that still exercises every kernel at full size: all selectors zero, random wires, the identity
permutation (z = 1), an SRS of distinct points (i G: the pipeline does not care that it is not a power series).
  python3 tools/plonk_prove_timing.py 16 18
--gnark times prove_gnark (gnark's proof shape: blinding, batched opening, bytes; wires as host integers) instead of prove();
--commitments K (implies --gnark) gives the key K Bsb22 commitments: each covers 2^k / 8 rows, whose gates read - l + pi2_j = 0, and
has its commitment row, where the L wire takes the hash of the commitment (the witness is completed between commitments);
--runs N --warmup W report the median and min .. max of N runs after W unrecorded ones; --json PATH appends one record per size."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import nlxpkg

ap = argparse.ArgumentParser()
ap.add_argument("log_n", nargs="*", type=int)
ap.add_argument("--commitments", type=int, default=0)
ap.add_argument("--gnark", action="store_true")
ap.add_argument("--runs", type=int, default=0)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--json", default=None)
opt = ap.parse_args()

nlx = nlxpkg.load()
import torch

P = nlx.bn254_plonk
R = P.R
ctx = nlx.Context(0)


def report(label, log_n, times):
    """the legacy line for the default run (mean of three), median and spread when --runs is given"""
    if not opt.runs:
        return "2^%d gates: %.1f ms per proof (%s)" % (log_n, sum(times) / len(times) * 1e3, label)
    ms = sorted(t * 1e3 for t in times)
    return "2^%d gates: median %.1f ms, min %.1f .. max %.1f ms over %d runs after %d warm-ups (%s)" % (
        log_n, statistics.median(ms), ms[0], ms[-1], len(ms), opt.warmup, label)


def timed(fn):
    for _ in range(opt.warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(opt.runs or 3):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, out


for log_n in opt.log_n or [16]:
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    w = P.root_of_unity(log_n)
    ident, x = [], 1
    for _ in range(n):
        ident.append(x)
        x = x * w % R
    vals = {k: [0] * n for k in ("ql", "qr", "qm", "qo", "qk")}
    vals.update(s1=ident, s2=[5 * v % R for v in ident], s3=[25 * v % R for v in ident])
    if not (opt.gnark or opt.commitments):
        # the default run, kept word for word with its own warm-up and loop so that its output line stays what it was
        srs = nlx.bn254_g1_multiples(ctx, (1, 2), n, device="cuda:0")
        pk = P.ProvingKey(ctx, vals, srs, 5, 25)
        # witness as fr.Element words resident in HBM (any words below r are Montgomery forms of some field elements)
        wires = [torch.from_numpy(np.stack([rng.integers(0, 2 ** 62, n), rng.integers(0, 2 ** 62, n), rng.integers(0, 2 ** 62, n),
                                            rng.integers(0, 2 ** 60, n)], axis=1).astype(np.int64)).cuda() for _ in range(3)]
        P.prove(pk, *wires)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            proof = P.prove(pk, *wires)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        print("2^%d gates: %.1f ms per proof (witness resident in HBM; 9 MSMs of n points, 5 + 12 + 1 transforms of n / 4n, the grand product, "
              "two openings; proof = 9 points + 6 scalars)" % (log_n, dt * 1e3), flush=True)
        continue
    # gnark's proof shape.  With K commitments: commitment j covers the rows [j n / 8, (j + 1) n / 8) of the lower half, its
    # commitment row is n / 2 + j, last_row is n - 1; those rows' gates are - l + (pi2_j | c_j) = 0, every other row's are empty
    K = opt.commitments
    srs = nlx.bn254_g1_multiples(ctx, (1, 2), n + 3, device="cuda:0")
    info = [{"committed": list(range(j * n // 8, (j + 1) * n // 8)), "row": n // 2 + j, "last_row": n - 1} for j in range(K)]
    for j, c in enumerate(info):
        vals["qcp%d" % j] = [0] * n
        for i in c["committed"] + [c["row"]]:
            vals["ql"][i] = R - 1
        for i in c["committed"]:
            vals["qcp%d" % j][i] = 1
    pk = P.ProvingKey(ctx, vals, srs, 5, 25, commitments=info) if K else P.ProvingKey(ctx, vals, srs, 5, 25)
    l, r, o = ([int(v) for v in rng.integers(0, 2 ** 62, n)] for _ in range(3))

    def witness(cs):
        for j, c in enumerate(cs):
            l[info[j]["row"]] = c
        return l, r, o
    if K:
        fn = lambda: P.prove_gnark(pk, public_inputs=(), witness=witness)
    else:
        fn = lambda: P.prove_gnark(pk, l, r, o)
    times, proof = timed(fn)
    label = "prove_gnark, %d Bsb22 commitments, wires as host integers; proof = %d bytes" % (K, len(proof))
    print(report(label, log_n, times), flush=True)
    if opt.json:
        with open(opt.json, "a") as f:
            f.write(json.dumps({"log_n": log_n, "commitments": K, "runs": len(times), "warmup": opt.warmup, "ms": [round(t * 1e3, 3) for t in times],
                                "median_ms": round(statistics.median(times) * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
                                "max_ms": round(max(times) * 1e3, 3)}) + "\n")
