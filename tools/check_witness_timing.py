"""Wall time of nlx_circuit_check_witness beside nlx_prove of the same circuit, in one process: the outer proof's gate mix
(bench.py --workload outer: GATE_MIXES["nearx"], seed 1000, 64 public inputs), the witness resident on the device.
  python3 tools/check_witness_timing.py [--sizes 16 18] [--reps 5] [--warmup 2]
Per size, on a fresh circuit per what-bit: the FIRST check (for gates it includes the constants' transform onto H, for copies
the sigma decode), then the median of --reps later checks after --warmup more; the same for a full check (what = 7) and for
nlx_prove.  Both calls return synchronised, so wall time is what a caller waits.  Writes profiles/check_witness_timing.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_MIX = dict(pct_poseidon=25, pct_arithmetic=20, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=10, pct_u32=15)
WHATS = (("gates", 1), ("copies", 2), ("all", 7))


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 18])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import nlxpkg
    nlx = nlxpkg.load()
    import torch
    ctx = nlx.Context(0)
    out = {"gate_mix": GATE_MIX, "reps": args.reps, "warmup": args.warmup, "unit": "ms, wall, witness on the device", "sizes": {}}
    for log_n in args.sizes:
        syn = nlx.SyntheticCircuit(log_n, seed=1000, num_public_inputs=64, **GATE_MIX)
        wires = torch.from_numpy(syn.wires.view(np.int64)).cuda()
        res = {}
        for name, bits in WHATS:
            cd = nlx.CircuitData.from_synthetic(ctx, syn)      # fresh: nothing cached for the first check
            ctx.synchronize()

            def check():
                rep = cd.check_witness(wires, syn.public_inputs, bits)
                assert rep.ok and rep.checked == bits & 3, str(rep)   # no tables in this circuit: LOOKUPS is dropped
            first = ms(check)
            for _ in range(args.warmup):
                check()
            later = [ms(check) for _ in range(args.reps)]
            res[name] = {"first_ms": round(first, 3), "later_median_ms": round(statistics.median(later), 3),
                         "later_ms": [round(v, 3) for v in later]}
            if bits == 7:
                prove = lambda: cd.prove_into(wires, syn.public_inputs.ctypes.data)   # noqa: E731
                for _ in range(args.warmup):
                    prove()
                pv = [ms(prove) for _ in range(args.reps)]
                res["prove"] = {"median_ms": round(statistics.median(pv), 3), "ms": [round(v, 3) for v in pv]}
            cd.close()
        res["later_full_check_over_prove"] = round(res["all"]["later_median_ms"] / res["prove"]["median_ms"], 4)
        out["sizes"]["2^%d" % log_n] = res
        print(log_n, json.dumps(res), flush=True)
    ctx.close()
    path = os.path.join(ROOT, "profiles", "check_witness_timing.json")
    if os.path.exists(path):   # keep what other tools recorded there (the k_quotient comparison)
        with open(path) as f:
            prev = json.load(f)
        out = dict(prev, **out)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
