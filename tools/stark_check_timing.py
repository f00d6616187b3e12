"""Time of the STARK trace checker beside proving, in one process, traces resident on the device:
  python3 tools/stark_check_timing.py [--reps 5] [--warmup 2]
The three STARKs of a Sync step at bench.py's shapes (the step main_1 -> main_2 of tests/golden/near, StarkConfig(batch_cols=512),
tagged) and wide_air(256) at 2^14 rows.  Per STARK:
  * prove_ms / check_ms: wall time of prove_rounds (prove) and check_rounds (check) on the same trace and round function - both
    return synchronised and both include the round-1 callback -, median of --reps after --warmup; first_check_ms is the first check
    of a fresh STARK (it uploads the periodic table and the segments' first indices);
  * check_kernel_ms: device time of the checker's kernels alone (HIP events around k_air_check and the row count);
  * vm_quotient_eval_ms: the `quotient_eval` stage of a prover built with NLX_AIR_VM=1 - the interpreter k_air_quotient running
    the same program on n * 2^qdb points -, the number the check is held against.
Writes profiles/stark_check_timing.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(nlx, ctx, name, build, args):
    """build() -> (StarkProver, prove, check): closures over a trace that is already on the device"""
    os.environ.pop("NLX_AIR_VM", None)
    holder, prove, check = build()
    pr = holder.prover if hasattr(holder, "prover") else holder
    res = {"degree_bits": int(pr.stark.desc.degree_bits), "n_cols": int(pr.stark.desc.n_cols), "n_words": int(pr.stark.desc.n_words),
           "qdb": int(pr.stark.desc.quotient_degree_factor).bit_length() - 1}
    rep = [None]

    def run_check():
        rep[0] = check()
        assert rep[0].ok, str(rep[0])
    res["first_check_ms"] = round(ms(run_check), 3)
    res["n_constraints"] = int(rep[0].n_constraints)
    for _ in range(args.warmup):
        run_check()
    ctx.kernel_timing(True)
    later = [ms(run_check) for _ in range(args.reps)]
    calls, dev_ms, _ = ctx.kernel_stats("air_check")
    ctx.kernel_timing(False)
    res["check_ms"] = round(statistics.median(later), 3)
    res["check_kernel_ms"] = round(dev_ms / max(calls, 1), 4)
    for _ in range(args.warmup):
        prove()
    res["prove_ms"] = round(statistics.median([ms(prove) for _ in range(args.reps)]), 3)
    res["generated_quotient_kernel"] = int(nlx.lib.dll.nlx_stark_quotient_kernel(pr.handle))
    holder.close()
    os.environ["NLX_AIR_VM"] = "1"          # read when the STARK is built: this one runs the interpreter
    holder, prove, check = build()
    os.environ.pop("NLX_AIR_VM", None)
    pr = holder.prover if hasattr(holder, "prover") else holder
    assert nlx.lib.dll.nlx_stark_quotient_kernel(pr.handle) == 0
    qe = []
    for _ in range(args.warmup + args.reps):
        prove()
        qe.append(dict(pr.stage_times())["quotient_eval"])
    res["vm_quotient_eval_ms"] = round(statistics.median(qe[args.warmup:]), 4)
    holder.close()
    res["check_kernel_over_vm_quotient_eval"] = round(res["check_kernel_ms"] / res["vm_quotient_eval_ms"], 4)
    res["check_over_prove"] = round(res["check_ms"] / res["prove_ms"], 4)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import nlxpkg
    nlx = nlxpkg.load()
    import torch
    ctx = nlx.Context(0)
    S, NP, SA, SB, E = nlx.stark, nlx.near_protocol, nlx.sha256_air, nlx.sha512_air, nlx.ed25519_air
    near = os.path.join(ROOT, "tests", "golden", "near")
    with open(os.path.join(near, "main_1.json")) as f:
        bps = json.load(f)["body"]["next_bps"]
    with open(os.path.join(near, "main_2.json")) as f:
        nxt = json.load(f)["body"]
    sha_msgs = NP.sync_sha256_messages(nxt)
    stmt = NP.approval_statement(bps, nxt)
    lb256 = max(2, (sum(len(SA.pad_message(m)) for m in sha_msgs) - 1).bit_length())
    lb512 = max(2, (len(stmt["sig_msgs"]) - 1).bit_length())
    log_slots = max(4, (len(stmt["slots"]) - 1).bit_length())
    slot_words = E.slots_to_words(stmt["slots"] + [E.inactive_slot()] * ((1 << log_slots) - len(stmt["slots"])))
    io = nlx.nearx_io
    sync_in, sync_out = io.sync_io(io.load_fixture(os.path.join(near, "main_2.json")))
    tag = S.step_tag(sync_in + sync_out)
    cfg = lambda: nlx.StarkConfig(batch_cols=512)   # noqa: E731

    def sha(mod, cls, msgs, lb, halves):
        def build():
            sp = cls(ctx, lb, cfg(), step_tag=tag)
            blocks, first, _ = mod.blocks_for_messages(msgs, lb)
            _, digest = sp.generate_trace(blocks, first)
            pis = mod.digest_halves(digest) if halves else digest
            return sp, (lambda: sp.prove_trace(pis)), (lambda: sp.check_trace(pis))
        return build

    def ed():
        pr = E.Ed25519Prover(ctx, log_slots, cfg(), step_tag=tag)
        t0 = pr.generate_trace(slot_words)
        fn = lambda rnd, known: t0 if rnd == 0 else pr.round1(known)   # noqa: E731
        return pr, (lambda: pr.prover.prove_rounds(fn, tag)), (lambda: pr.prover.check_rounds(fn, tag))

    def wide():
        air = S.wide_air(256)
        pr = S.Stark(air, 14).build(ctx)
        trace, pis = S.wide_trace(air, 14)
        dev = torch.from_numpy(trace.view(np.int64)).cuda()
        return pr, (lambda: pr.prove(dev, pis)), (lambda: pr.check(dev, pis))

    out = {"reps": args.reps, "warmup": args.warmup, "unit": "ms; wall unless named kernel / stage; traces on the device", "starks": {}}
    for name, build in (("sha256_sync", sha(SA, SA.Sha256Prover, sha_msgs, lb256, False)),
                        ("sha512_sync", sha(SB, SB.Sha512Prover, stmt["sig_msgs"], lb512, True)),
                        ("ed25519_sync", ed), ("wide_air_256_2p14", wide)):
        out["starks"][name] = measure(nlx, ctx, name, build, args)
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "stark_check_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
