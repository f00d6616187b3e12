"""What tests/test_stark_verify_cpu.py and tests/test_gpu_stark_verify.py share: the statements whose proofs the STARK verifier
(nlx_stark_verify) is tried on - one per code path -, each with the oracle's proof of it, and the map from the oracle verifier's
return codes to the verifier's reasons.  Proofs come from the oracle's provers, not from the prover the verifier ships with."""
import numpy as np

from conftest import P, rand_field
from test_gpu_stark import _random_air
from test_logup import make_trace, range_air, rounds_fn
from test_stark_cpu import fingerprint_air, fingerprint_rounds, logup_air, logup_case, logup_rounds, make_case, run_program

# oracle/stark.c orc_stark_verify -> NLX_VERIFY_*
MALFORMED, PUBLIC_INPUTS, CONSTRAINTS, POW, TRACE_PATH, FRI_FOLD, FRI_PATH, FINAL_POLY = range(1, 9)
REASON_OF_ORACLE = {-1: MALFORMED, -4: MALFORMED, -6: MALFORMED, -10: MALFORMED, -11: MALFORMED, -2: CONSTRAINTS, -3: POW,
                    -5: TRACE_PATH, -7: FRI_FOLD, -8: FRI_PATH, -9: FINAL_POLY}

# (name, AIR kind, degree_bits, config, program segment size or None)
PLAIN_CASES = [
    ("fib5", "fib", 5, {}, None),                                        # no reduction round, one quotient coset
    ("fib7-nondefault", "fib", 7, dict(num_challenges=1, fri_arity_bits=3, fri_num_queries=20, fri_pow_bits=8, cap_height=2), None),
    ("wide16-rate2-arity4", "wide16", 8, dict(rate_bits=2, fri_arity_bits=2, fri_final_poly_bits=3, fri_num_queries=30), None),
    ("deg4-rate3", "deg4", 9, dict(rate_bits=3), None),
    ("periodic6", "periodic", 6, {}, None),
    ("wide64-group24", "wide64", 10, dict(leaf_group_cols=24), None),     # short last run
    ("wide16-group12", "wide16", 8, dict(leaf_group_cols=12), None),      # last run no longer than a digest
    ("wide64-openings8", "wide64", 9, dict(openings_group=8), None),
    ("wide320-batch64", "wide320", 8, dict(batch_cols=64), None),         # five batches
    ("wide16-batch12", "wide16", 8, dict(batch_cols=12), None),           # a batch whose row is its own digest
    ("wide96-16segments", "wide96", 7, {}, 16),
    ("wide16", "wide16", 8, {}, None),                                    # the tamper tests' first statement
]
ROUND_CASES = ["logup", "range-check", "fingerprint"]
RANDOM_CASES = ["random%d" % s for s in range(4)]
ALL_CASES = [c[0] for c in PLAIN_CASES] + ROUND_CASES + RANDOM_CASES


class Case:
    """a statement (`st`: a Stark), its witness (`t`, `pis` - or `rounds` for a multi-round one) and the oracle's proof"""

    def __init__(self, st, t=None, pis=(), rounds=None):
        self.st, self.t, self.pis, self.rounds = st, t, pis, rounds
        self._proof = None

    def oracle_proof(self, orc):
        if self._proof is None:
            self._proof = (orc.stark_prove_rounds(self.st.desc, self.rounds, self.pis) if self.rounds is not None
                           else orc.stark_prove(self.st.desc, self.t, self.pis))
        return self._proof

    def gpu_proof(self, prover):
        return prover.prove_rounds(self.rounds, self.pis) if self.rounds is not None else prover.prove(self.t, self.pis)


def satisfied_random_case(S, seed):
    """A random program over every instruction (test_gpu_stark._random_air) WITH a trace that satisfies it: every constraint e
    becomes e - s for a fresh column s whose cells are e's values, row by row (the reference interpreter of test_stark_cpu
    computes them); the columns under a boolean constraint hold bits."""
    rng = np.random.default_rng(1000 + seed)
    n_cols, n_pis = int(rng.integers(2, 24)), int(rng.integers(0, 4))
    air = _random_air(S, rng, n_cols, n_pis, with_periodic=bool(seed & 1))
    db = 5 + seed % 3
    n = 1 << db
    t = rand_field(rng, (n_cols, n))
    pis = rand_field(rng, (n_pis,))
    for op, e, _ in air._emits:
        if op == S.AIR_EMIT_BOOL:
            t[e.a] = rng.integers(0, 2, n, dtype=np.uint64)
    words = air.compile(segment_nodes=0)
    rows = [run_program(words, t[:, i], t[:, (i + 1) % n], pis, periodic=[int(c[i % len(c)]) for c in air._periodic]) for i in range(n)]
    slack, emits = [], []
    for k, (op, e, cnt) in enumerate(air._emits):
        if op == S.AIR_EMIT_BOOL:
            emits.append((op, e, cnt))
            continue
        slack.append([rows[i][k][1] for i in range(n)])
        air.n_cols += 1
        emits.append((op, e - air.local(air.n_cols - 1), 1))
    air._emits = emits
    if seed >= 2:
        air.segment_nodes = 3 + seed   # many small segments with different register needs: several launch groups
    rate_bits = 1 if air.quotient_degree_factor() <= 2 else 2
    cfg = S.StarkConfig(rate_bits=rate_bits + (seed % 3 == 2), fri_num_queries=12, fri_pow_bits=6, num_challenges=1 + (seed % 2),
                        fri_arity_bits=2 + seed % 3)
    return Case(S.Stark(air, db, cfg), np.vstack([t, np.array(slack, dtype=np.uint64).reshape(len(slack), n)]), pis)


_cache = {}


def case(nlx, orc, name):
    """the named statement, built once a session"""
    if name in _cache:
        return _cache[name]
    S = nlx.stark
    if name == "logup":
        c = Case(S.Stark(logup_air(S), 7, S.StarkConfig(fri_num_queries=20)), rounds=logup_rounds(*logup_case()), pis=[])
    elif name == "range-check":   # the fused EMIT_LOGUP instruction, periodic table columns, two challenges
        air, _ = range_air(nlx, 5, 6)
        c = Case(S.Stark(air, 7, S.StarkConfig(fri_num_queries=20)), rounds=rounds_fn(orc, make_trace(orc, 5, 6, 7), 5, 6), pis=[])
    elif name == "fingerprint":
        v = np.random.default_rng(5).integers(0, P, 64, dtype=np.uint64)
        c = Case(S.Stark(fingerprint_air(S), 6, S.StarkConfig(fri_num_queries=20)), rounds=fingerprint_rounds(v), pis=[])
    elif name.startswith("random"):
        c = satisfied_random_case(S, int(name[6:]))
    else:
        _, kind, db, cfg, seg = next(x for x in PLAIN_CASES if x[0] == name)
        air, t, pis = make_case(S, kind, db)
        if seg is not None:
            air.segment_nodes = seg
        c = Case(S.Stark(air, db, S.StarkConfig(**cfg)), t, pis)
    _cache[name] = c
    return c
