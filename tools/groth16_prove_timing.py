"""Wall time of one Groth16 proof over BN254 at 2^k constraints on a structured key (queries tiled from 64 G1 / 16 G2 points: the
pipeline does not care that it is not a setup's output), the R1CS built so that a o b = c holds.
  python3 tools/groth16_prove_timing.py 18 20 --json profiles/groth16_prove_timing.json
Default mode: nlx_bn254_groth16_prove on a resident key, the witness and a, b, c resident in HBM - first with a, b, c supplied
(like for like with the baseline), then with a, b, c computed from the key's matrices (the difference is the SpMV's cost; the
kernel's own time is reported from the library's kernel timing).
--separate-calls: the baseline - only entry points that exist without the resident key: nlx_bn254_groth16_quotient (h left on the
device), the witness filtered by the infinity masks on the host, five nlx_bn254_msm_g1 / _g2 calls with the (device-resident) points
passed per call, a, b, c supplied.  The blinding tail (a few scalar multiplications a caller would write for itself) is NOT in the
baseline's time: it is in the resident-key figure only.  This mode imports nothing the resident key brought, so it runs on a build
of the commit before it.
--runs N --warmup W: median and min .. max of N runs after W unrecorded ones; --json PATH appends one record per size and mode.
--one-proof: build the key, run ONE proof (a, b, c computed) and stop - the process to put under a kernel trace:
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/groth16_prove_timing.py 18 --one-proof
--commitments K --committed M: the same instance on a key with K Bsb22 / Pedersen commitments over M committed wires in all (split
evenly; the bases tiled from the same 64 points), proved by nlx_bn254_groth16_prove_committed - what a commitment costs is the
difference to the run without.  The commitment wires hold the instance's own values: the library does not
hash, and the binding's challenge check is not part of the proof's time, so the library entry is timed directly.
The A/B of the shared sort: a tuning build of the library that sorts the wire vector's digits once per query,
  NLX_BUILD_VARIANT=g16sort NLX_EXTRA_FLAGS=-DNLX_GROTH16_INDEPENDENT_SORT python near-light-client_amd/build.py
and this tool run with NLX_BUILD_VARIANT=g16sort in the environment (its records are labelled independent-sort)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "oracle")
import bn254_py as bn
import nlxpkg

ap = argparse.ArgumentParser()
ap.add_argument("log_n", nargs="*", type=int)
ap.add_argument("--separate-calls", action="store_true")
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--json", default=None)
ap.add_argument("--one-proof", action="store_true")
ap.add_argument("--commitments", type=int, default=0)
ap.add_argument("--committed", type=int, default=0)
opt = ap.parse_args()

nlx = nlxpkg.load()
import torch

R = bn.R
MONT = (1 << 256) % R
MONT_INV = pow(MONT, R - 2, R)
ctx = nlx.Context(0)
DEV = "cuda:0"


def words(values):
    """integers -> (n, 4) uint64 little-endian words"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def timed(fn):
    for _ in range(opt.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(opt.runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def record(log_n, mode, times, **extra):
    ms = sorted(times)
    rec = dict(log_n=log_n, mode=mode, runs=len(ms), warmup=opt.warmup, median_ms=round(statistics.median(ms), 3), min_ms=round(ms[0], 3),
               max_ms=round(ms[-1], 3), spread_ms=round(ms[-1] - ms[0], 3), ms=[round(t, 3) for t in times], **extra)
    print("2^%d constraints, %s: median %.1f ms, min %.1f .. max %.1f ms over %d runs after %d warm-ups %s" % (
        log_n, mode, rec["median_ms"], rec["min_ms"], rec["max_ms"], len(ms), opt.warmup, extra or ""), flush=True)
    if opt.json:
        with open(opt.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


def instance(log_n, rng):
    """n constraints (w_i1 + k w_i2) (w_i3 - w_i4) = the constraint's own new wire: CSR matrices over a table of 8 coefficients,
    the witness and a, b, c as Montgomery integers"""
    n = 1 << log_n
    free = 64
    table = [1, R - 1] + [int(x) for x in rng.integers(2, 1 << 62, 6)]
    w = [1] + [int(x) for x in rng.integers(1, 1 << 62, free - 1)]
    pick = rng.integers(0, 1 << 62, (n, 4))
    kid = rng.integers(0, 8, n)
    wire_a, wire_b = np.zeros((n, 2), dtype=np.uint32), np.zeros((n, 2), dtype=np.uint32)
    a, b, c = [], [], []
    for j in range(n):
        have = free + j
        i1, i2, i3, i4 = (int(v) % have for v in pick[j])
        x = (w[i1] + table[kid[j]] * w[i2]) % R
        y = (w[i3] - w[i4]) % R
        z = x * y % R
        wire_a[j], wire_b[j] = (i1, i2), (i3, i4)
        a.append(x)
        b.append(y)
        c.append(z)
        w.append(z)
    n_wires = len(w)
    two = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    r1cs = {"A": (two, wire_a.reshape(-1), np.stack([np.zeros(n, dtype=np.uint32), kid.astype(np.uint32)], axis=1).reshape(-1)),
            "B": (two, wire_b.reshape(-1), np.tile(np.array([0, 1], dtype=np.uint32), n)),
            "C": (np.arange(n + 1, dtype=np.uint64), np.arange(free, free + n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)),
            "coeffs": words([v * MONT % R for v in table])}
    mont = lambda vals: words([v * MONT % R for v in vals])
    return n_wires, r1cs, mont(w), mont(a), mont(b), mont(c)


g1 = [bn.g1_mul(7 + 11 * i, bn.G1) for i in range(64)]
g2 = [bn.g2_mul(5 + 3 * i, bn.G2) for i in range(16)]
p1, p2 = nlx.bn254_g1_pack(g1), nlx.bn254_g2_pack(g2)

for log_n in opt.log_n or [18]:
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    t0 = time.perf_counter()
    n_wires, r1cs, w, a, b, c = instance(log_n, rng)
    mask_a = np.bincount(r1cs["A"][1], minlength=n_wires) == 0
    mask_b = np.bincount(r1cs["B"][1], minlength=n_wires) == 0
    wires = np.arange(n_wires)
    keep_a, keep_b = wires[~mask_a], wires[~mask_b]
    q = dict(g1_a=p1[keep_a % 64], g1_b=p1[(keep_b + 7) % 64], g2_b=p2[keep_b % 16], g1_k=p1[(3 * wires[1:] + 1) % 64],
             g1_z=p1[(5 * np.arange(n - 1) + 2) % 64])
    print("2^%d constraints, %d wires (%d in A, %d in B): instance built in %.1f s" % (log_n, n_wires, len(keep_a), len(keep_b),
                                                                                        time.perf_counter() - t0), flush=True)
    d_w, d_a, d_b, d_c = dev(w), dev(a), dev(b), dev(c)
    if opt.separate_calls:
        d_q = {k: dev(v) for k, v in q.items()}
        d_h = torch.empty((n, 4), dtype=torch.int64, device=DEV)
        shift = words([5 * MONT % R])
        dll = nlx.lib.dll

        def separate():
            ctx.check(dll.nlx_bn254_groth16_quotient(ctx.handle, log_n, d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), shift.ctypes.data, d_h.data_ptr()))
            wa, wb = w[~mask_a], w[~mask_b]                      # the host filters the wire vector by the key's masks
            out = [nlx.bn254_msm_g1(ctx, d_q["g1_a"], wa, montgomery=True), nlx.bn254_msm_g1(ctx, d_q["g1_b"], wb, montgomery=True),
                   nlx.bn254_msm_g2(ctx, d_q["g2_b"], wb, montgomery=True), nlx.bn254_msm_g1(ctx, d_q["g1_k"], d_w[1:], montgomery=True),
                   nlx.bn254_msm_g1(ctx, d_q["g1_z"], d_h[:n - 1], montgomery=True)]
            return out
        record(log_n, "separate-calls", timed(separate))
        continue
    G = nlx.bn254_groth16
    t0 = time.perf_counter()
    commitments = None
    if opt.commitments:
        # the commitment wires are the last K wires, the committed ones M wires spread over the private wires before them
        K, M = opt.commitments, opt.committed
        cwires = list(range(n_wires - K, n_wires))
        ids = np.unique(np.linspace(1, n_wires - K - 1, M).astype(np.int64))
        assert len(ids) == M, "too many committed wires for this size"
        sets = np.array_split(ids, K)
        commitments = [dict(private=[int(i) for i in sets[j]], public=[0] + cwires[:j], wire=cwires[j], basis=p1[(7 * sets[j] + j) % 64],
                            basis_exp_sigma=p1[(11 * sets[j] + 5 + j) % 64]) for j in range(K)]
        left = np.ones(n_wires, dtype=bool)
        left[0], left[ids], left[cwires] = False, False, False
        q["g1_k"] = p1[(3 * wires[left] + 1) % 64]
    key = G.ProvingKey(ctx, log_n, n_wires, 1, n, q["g1_a"], q["g1_b"], q["g2_b"], q["g1_k"], q["g1_z"], mask_a.astype(np.uint8),
                       mask_b.astype(np.uint8), p1[1], p1[2], p1[3], p2[1], p2[2], r1cs=r1cs, commitments=commitments)
    info = key.info()
    print("key resident: %.1f MB, created in %.2f s; rows per lane %d, per wave %d; %d of %d terms have a unit coefficient" % (
        info["resident_bytes"] / 1e6, time.perf_counter() - t0, info["lane_rows"], info["wave_rows"], info["unit_terms"], info["terms"]), flush=True)
    r, s = 0x1234567 + log_n, 0x7654321 + log_n
    sort = "independent-sort" if os.environ.get("NLX_BUILD_VARIANT") == "g16sort" else "shared-sort"
    if opt.commitments:
        rw, sw, rhow = G.fr_words(r), G.fr_words(s), G.fr_words(0x2468ACE + log_n)
        outs = [np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros((opt.commitments, 8), dtype=np.uint64),
                np.zeros(8, dtype=np.uint64)]

        def committed(abc=(None, None, None)):
            ctx.check(nlx.lib.dll.nlx_bn254_groth16_prove_committed(ctx.handle, key.handle, d_w.data_ptr(), *[None if t is None else t.data_ptr() for t in abc],
                                                                    rw.ctypes.data, sw.ctypes.data, rhow.ctypes.data, *[o.ctypes.data for o in outs]))
        if opt.one_proof:
            committed()
            torch.cuda.synchronize()
            key.close()
            continue
        label = "%d commitments over %d wires, " % (opt.commitments, opt.committed)
        record(log_n, "resident-key, abc supplied, " + label + sort, timed(lambda: committed((d_a, d_b, d_c))), resident_mb=round(info["resident_bytes"] / 1e6, 1))
        record(log_n, "resident-key, abc computed, " + label + sort, timed(committed))
        key.close()
        continue
    if opt.one_proof:
        G.prove(key, d_w, r, s)
        torch.cuda.synchronize()
        key.close()
        continue
    first = G.proof_bytes(*G.prove(key, d_w, r, s, abc=(d_a, d_b, d_c)))
    assert first == G.proof_bytes(*G.prove(key, d_w, r, s)), "a, b, c computed on the device give another proof"
    record(log_n, "resident-key, abc supplied, " + sort, timed(lambda: G.prove(key, d_w, r, s, abc=(d_a, d_b, d_c))), resident_mb=round(info["resident_bytes"] / 1e6, 1))
    record(log_n, "resident-key, abc computed, " + sort, timed(lambda: G.prove(key, d_w, r, s)))
    ctx.kernel_timing(True)
    for _ in range(opt.runs):
        G.r1cs_eval(key, d_w)
    calls, ms, alg_bytes = ctx.kernel_stats("bn254_r1cs_eval")
    ctx.kernel_timing(False)
    gbs = (40.0 * info["terms"] + 96.0 * n) / (ms / calls) / 1e6      # per term: 32 bytes of witness, a wire id and a code; 3 n results
    print("r1cs_eval kernels: %.3f ms per call over %d calls, %.1f GB/s of algorithmic bytes (%d terms)" % (ms / calls, calls, gbs, info["terms"]), flush=True)
    if opt.json:
        with open(opt.json, "a") as f:
            f.write(json.dumps(dict(log_n=log_n, mode="r1cs_eval kernels", calls=calls, ms_per_call=round(ms / calls, 4), terms=info["terms"],
                                    alg_gb_per_s=round(gbs, 1))) + "\n")
    key.close()

if not opt.separate_calls and not opt.one_proof and not opt.commitments:
    # what the baseline leaves out: the blinding tail (five host scalar multiplications, one of them in G2).  A proof of ONE
    # constraint on two wires costs that tail plus the fixed launches of an empty pipeline: an upper bound of the tail's cost
    G = nlx.bn254_groth16
    one = {m: (np.array([0, 1], dtype=np.uint64), np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)) for m in "ABC"}
    one["coeffs"] = words([MONT])
    tiny = G.ProvingKey(ctx, 1, 2, 1, 1, p1[4:6], p1[6:8], p2[3:5], p1[8:9], p1[9:10], np.zeros(2, dtype=np.uint8), np.zeros(2, dtype=np.uint8),
                        p1[1], p1[2], p1[3], p2[1], p2[2], r1cs=one)
    w2 = words([MONT, MONT])
    record(1, "resident-key, 1 constraint (blinding tail + fixed launches)", timed(lambda: G.prove(tiny, w2, 0x1234567, 0x7654321)))
    tiny.close()

