"""Time of the STARK verifier for 1, 16 and 64 proofs of one STARK in one call:
  python3 tools/stark_verify_timing.py [--reps 5] [--warmup 2] [--only NAME]
wide_air(64) at 2^12 rows and the three STARKs of a Sync step at bench.py's shapes (the step main_1 -> main_2 of
tests/golden/near, tagged), each with StarkConfig(batch_cols=0) and StarkConfig(batch_cols=512).  Per STARK and batch size:
  * device_ms: the three launches' device time (HIP events around k_fri_paths, k_fri_queries and the k_verify_constraints
    launch groups), summed per call, median of --reps calls after --warmup; paths_ms / fri_ms / constraints_ms are its parts;
  * wall_ms: the whole call, host side included (parsing, the transcript, the copies), median likewise;
  * oracle_ms: for scale only, the oracle's one-thread host verifier (test infrastructure) on the same proof.
The proofs are the GPU prover's; the batch is the same proof n times - the verifier has no cache that could tell.
Writes profiles/stark_verify_timing.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("stark_verify_paths", "stark_verify_fri", "stark_verify_constraints")
BATCHES = (1, 16, 64)


def measure(ctx, orc, name, pr, proof, args):
    d = pr.stark.desc
    res = {"degree_bits": int(d.degree_bits), "n_cols": int(d.n_cols), "n_words": int(d.n_words), "batch_cols": int(d.batch_cols),
           "proof_bytes": len(proof), "queries": int(d.fri_num_queries)}
    t0 = time.perf_counter()
    first = pr.verify(proof)
    res["first_verify_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert first.ok, str(first)
    t0 = time.perf_counter()
    assert orc.stark_verify(d, proof) == 1
    res["oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    for n in BATCHES:
        proofs = [proof] * n
        dev, wall = [], []
        for rep in range(args.warmup + args.reps):
            ctx.kernel_timing(True)
            t0 = time.perf_counter()
            vs = pr.verify_many(proofs)
            w = (time.perf_counter() - t0) * 1e3
            parts = [ctx.kernel_stats(k)[1] for k in KERNELS]
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
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_verify_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import nlxpkg
    import oracle_py as orc
    nlx = nlxpkg.load()
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

    def sha(mod, cls, msgs, lb, halves):
        def build(cfg):
            sp = cls(ctx, lb, cfg, step_tag=tag)
            blocks, first, _ = mod.blocks_for_messages(msgs, lb)
            _, digest = sp.generate_trace(blocks, first)
            return sp, sp.prove_trace(mod.digest_halves(digest) if halves else digest)
        return build

    def ed(cfg):
        pr = E.Ed25519Prover(ctx, log_slots, cfg, step_tag=tag)
        t0 = pr.generate_trace(slot_words)
        return pr, pr.prover.prove_rounds(lambda rnd, known: t0 if rnd == 0 else pr.round1(known), tag)

    def wide(cfg):
        air = S.wide_air(64)
        pr = S.Stark(air, 12, cfg).build(ctx)
        return pr, pr.prove(*S.wide_trace(air, 12))

    out = {"reps": args.reps, "warmup": args.warmup, "batches": list(BATCHES),
           "unit": "ms; device = HIP events around the verifier's launches, wall = the whole call", "starks": {}}
    for name, build in (("wide_air_64_2p12", wide), ("sha256_sync", sha(SA, SA.Sha256Prover, sha_msgs, lb256, False)),
                        ("sha512_sync", sha(SB, SB.Sha512Prover, stmt["sig_msgs"], lb512, True)), ("ed25519_sync", ed)):
        for bc in (0, 512):
            key = "%s_batch_cols_%d" % (name, bc)
            if args.only and args.only not in key:
                continue
            holder, proof = build(nlx.StarkConfig(batch_cols=bc))
            out["starks"][key] = measure(ctx, orc, key, holder.prover if hasattr(holder, "prover") else holder, proof, args)
            holder.close()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
