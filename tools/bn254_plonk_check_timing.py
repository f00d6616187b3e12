"""Wall time of nlx_bn254_plonk_check_witness against nlx_bn254_plonk_prove on the same resident key, in one process (DESIGN.md
section 35).  The key is the structured one of tools/plonk_resident_timing.py (all selectors zero but the commitments' rows,
random wires, an SRS of distinct points) with one change: sigma swaps the rows 2 i and 2 i + 1 of every wire, which hold equal
values, so that - as in a real gnark circuit - almost no cell is routed to itself and the first COPIES check pays the whole
decode (the pair that holds a commitment row stays on the identity).  Wires on the device.
  python3 tools/bn254_plonk_check_timing.py [--sizes 18 20] [--commitments 0 1] [--limit 900]
Per configuration, in a child process under its own time limit: the synchronous call's wall time, the median of 5 after 2
warm-ups, for GATES, COPIES, GATES | COPIES and ALL on a key checked before ("later"), the first call of each on a key never
checked ("first": for COPIES and ALL it includes the sigma decode), one proof on the same key, and the three kernels' device
times.  The one condition: a later GATES | COPIES check takes less time than one proof - the tool ends with a non-zero status
when it does not hold at some size (tests/test_gpu_bn254_plonk_check.py asserts the same at 2^10 gates).  Writes
profiles/bn254_plonk_check_timing.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("bn254_plonk_sigma_decode", "bn254_plonk_check_gates", "bn254_plonk_check_copies")
WARMUPS, RUNS = 2, 5


def child(log_n, K):
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
    info = [{"committed": list(range(j * n // 8, (j + 1) * n // 8)), "row": n // 2 + 2 * j, "last_row": n - 1} for j in range(K)]
    fixed_pairs = {c["row"] >> 1 for c in info}
    partner = [i if (i >> 1) in fixed_pairs else i ^ 1 for i in range(n)]
    swapped = [ident[partner[i]] for i in range(n)]
    vals = {k: [0] * n for k in ("ql", "qr", "qm", "qo", "qk")}
    vals.update(s1=swapped, s2=[5 * v % R for v in swapped], s3=[25 * v % R for v in swapped])
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
    new_key = lambda: P.ResidentKey(ctx, on_dev, srs, 5, 25, commitments=info)
    cols = [[int(v) for v in rng.integers(0, 2 ** 62, n)] for _ in range(3)]
    for col in cols:
        for i in range(0, n, 2):
            col[i + 1] = col[i]
    cb = [int(v) for v in rng.integers(1, 2 ** 62, 2 * K)]
    to_dev = lambda col: torch.from_numpy(nlx.bn254_pack([[P._to_mont(v) for v in col]])[0].view(np.int64)).cuda()
    dev = [to_dev(c) for c in cols]
    key = new_key()
    for j in range(K):   # the hint once: finished wires, as a solver hands them over
        c = P.commit_resident(key, j, dev[0], cb[2 * j:2 * j + 2])[1]
        dev[0][info[j]["row"]] = to_dev([c])[0]
    blind = [int(v) for v in rng.integers(1, 2 ** 62, 9)]
    cbk = cb if K else None
    whats = {"gates": P.CHECK_GATES, "copies": P.CHECK_COPIES, "gates_copies": P.CHECK_GATES | P.CHECK_COPIES, "all": P.CHECK_ALL}

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def median_of(fn):
        for _ in range(WARMUPS):
            fn()
        times = [timed(fn)[0] for _ in range(RUNS)]
        return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}

    check = lambda k_, what: P.check_resident(k_, dev[0], dev[1], dev[2], (), cbk, what)
    record = {"log_n": log_n, "commitments": K, "warmups": WARMUPS, "runs": RUNS, "later": {}, "first": {}}
    rep = check(key, P.CHECK_ALL)        # also warms the process: modules, twiddle tables, the allocator
    assert rep.satisfied == 1 and rep.cache_bytes == 12 * n, str(rep)
    record["cache_bytes"] = int(rep.cache_bytes)
    for name, what in whats.items():
        record["later"][name] = median_of(lambda: check(key, what))
    record["prove"] = median_of(lambda: P.prove_resident(key, dev[0], dev[1], dev[2], (), blind, cbk))
    for name, what in whats.items():     # a key never checked: once
        fresh = new_key()
        ms, rep = timed(lambda: check(fresh, what))
        assert rep.satisfied == 1
        record["first"][name] = round(ms, 3)
        fresh.close()
    # a witness with one wrong cell: the failing path's second launch and reads
    bad = dev[2].clone()
    bad[n // 3] = to_dev([12345])[0]
    record["later"]["gates_copies_unsatisfied"] = median_of(lambda: P.check_resident(key, dev[0], dev[1], bad, (), cbk, 3))
    ctx.kernel_timing(True)
    fresh = new_key()
    check(fresh, P.CHECK_ALL), check(fresh, P.CHECK_ALL)
    record["kernel_ms"] = {}
    for name in KERNELS:
        calls, ms, _ = ctx.kernel_stats(name)
        record["kernel_ms"][name] = {"calls": calls, "mean_ms": round(ms / calls, 4) if calls else None}
    ctx.kernel_timing(False)
    fresh.close()
    record["later_gates_copies_below_one_proof"] = record["later"]["gates_copies"]["median_ms"] < record["prove"]["median_ms"]
    print("RECORD " + json.dumps(record), flush=True)
    key.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[18, 20])
    ap.add_argument("--commitments", nargs="*", type=int, default=[0, 1])
    ap.add_argument("--limit", type=float, default=900.0, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn254_plonk_check_timing.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args()
    if opt.child:
        return child(opt.child[0], opt.child[1])
    records = []
    for log_n in opt.sizes:
        for K in opt.commitments:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(log_n), str(K)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=opt.limit)
            except subprocess.TimeoutExpired:
                sys.exit("2^%d gates, %d commitments: no result within %.0f s - stopping here" % (log_n, K, opt.limit))
            line = [x for x in res.stdout.splitlines() if x.startswith("RECORD ")]
            if res.returncode or not line:
                sys.exit("2^%d gates, %d commitments: the child ended with status %d - stopping here\n%s" % (log_n, K, res.returncode, res.stderr[-2000:]))
            rec = json.loads(line[0][7:])
            records.append(rec)
            print("2^%d gates, k = %d: later gates %.2f, copies %.2f, gates | copies %.2f, all %.2f ms; first copies %.2f ms; one proof %.2f ms; condition %s" % (
                log_n, K, rec["later"]["gates"]["median_ms"], rec["later"]["copies"]["median_ms"], rec["later"]["gates_copies"]["median_ms"],
                rec["later"]["all"]["median_ms"], rec["first"]["copies"], rec["prove"]["median_ms"],
                "holds" if rec["later_gates_copies_below_one_proof"] else "DOES NOT HOLD"), flush=True)
            with open(opt.out, "w") as f:
                json.dump({"tool": "tools/bn254_plonk_check_timing.py", "unit": "ms of wall time per synchronous call", "records": records}, f, indent=1)
                f.write("\n")
    failed = [(r["log_n"], r["commitments"]) for r in records if not r["later_gates_copies_below_one_proof"]]
    if failed:
        sys.exit("a later GATES | COPIES check does not take less time than one proof at (log_n, k) = %s" % failed)


if __name__ == "__main__":
    main()
