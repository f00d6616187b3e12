"""What tests/test_plonk_verify_cpu.py and tests/test_gpu_plonk_verify.py share: the circuits whose proofs the plonky2 verifier
(nlx_verify) is tried on - the smallest that takes each branch -, each with the oracle PROVER's proof of its witness, and the map
from the oracle verifier's return codes to the verifier's reasons.  A plain module (not a conftest)."""
from conftest import P

# oracle/plonk.c orc_verify -> NLX_VERIFY_*
MALFORMED, PUBLIC_INPUTS, CONSTRAINTS, POW, TRACE_PATH, FRI_FOLD, FRI_PATH, FINAL_POLY = range(1, 9)
REASON_OF_ORACLE = {-1: MALFORMED, -4: MALFORMED, -6: MALFORMED, -10: MALFORMED, -2: CONSTRAINTS, -3: POW, -5: TRACE_PATH,
                    -7: FRI_FOLD, -8: FRI_PATH, -9: FINAL_POLY}

ALL19 = dict(pct_poseidon=10, pct_arithmetic=10, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=20, pct_u32=30)
_OTHER = dict(pct_poseidon=20, pct_arithmetic=30, pct_base_sum=5, pct_constant=5, pct_extension=10)
# name -> (log_n, SyntheticCircuit arguments, CircuitConfig arguments)
CASES = {
    "rows5": (5, dict(seed=1), {}),                                                   # no FRI reduction round
    "rows6-one-selector": (6, dict(seed=6, pct_poseidon=0, pct_arithmetic=40, pct_base_sum=20, pct_constant=20), {}),
    "all-gates": (9, dict(seed=21, **ALL19), {}),                                     # the tamper tests' statement
    "wide-comparison": (9, dict(seed=25, wide_comparison=True, **ALL19), {}),         # 132 constraints
    # the three non-default configs of test_gpu_prover.py::test_other_configs_match_oracle
    "one-challenge-cap0-arity4": (9, dict(seed=77, **_OTHER), dict(num_challenges=1, cap_height=0, fri_num_queries=5, fri_pow_bits=4,
                                                                   fri_arity_bits=2, fri_final_poly_bits=2)),
    "cap5-no-pow": (9, dict(seed=77, **_OTHER), dict(cap_height=5, fri_num_queries=40, fri_pow_bits=0)),
    "arity8": (9, dict(seed=77, **_OTHER), dict(fri_arity_bits=3, fri_final_poly_bits=3, cap_height=2, fri_num_queries=11, fri_pow_bits=8)),
    # LDE 2^10, arity 4, cap height 6: layer 0's tree has height 8 (two siblings), layer 1's has 6 - no taller than its cap
    "layer-inside-cap": (7, dict(seed=7), dict(cap_height=6, fri_arity_bits=2, fri_final_poly_bits=2, fri_num_queries=10, fri_pow_bits=4)),
    # the shapes of test_gpu_lookup.py
    "lookup-1-table": (9, dict(seed=49, num_luts=1, lut_bits=6, num_lookups=100), {}),
    "lookup-2-tables": (10, dict(seed=50, num_luts=2, lut_bits=8, num_lookups=333), {}),
    "lookup-one-challenge": (10, dict(seed=77, num_luts=2, lut_bits=7, num_lookups=90), dict(num_challenges=1)),
    # one query and no proof of work: the statement on which a tampered final polynomial can reach its own check
    "rows5-one-query": (5, dict(seed=1), dict(fri_num_queries=1, fri_pow_bits=0)),
}
ALL_CASES = list(CASES)
SANITIZER_CASES = ["rows5", "one-challenge-cap0-arity4", "lookup-1-table"]


class Case:
    """a circuit (`syn`: a SyntheticCircuit with its witness), the oracle's circuit data (`ref`) and the oracle prover's proof"""

    def __init__(self, nlx, orc, name):
        log_n, kw, cfg = CASES[name]
        self.name = name
        self.syn = nlx.SyntheticCircuit(log_n, config=nlx.CircuitConfig(**cfg), **kw)
        self.ref = orc.Circuit.from_synthetic(self.syn)
        self.proof = self.ref.prove(self.syn.wires, self.syn.public_inputs)
        assert len(self.proof) > 0
        self.pis = [int(v) for v in self.syn.public_inputs]


_cases = {}


def case(nlx, orc, name):
    if name not in _cases:
        _cases[name] = Case(nlx, orc, name)
    return _cases[name]


def flip(proof, off, bit=0):
    bad = bytearray(proof)
    bad[off] ^= 1 << bit
    return bytes(bad)


def path_length_bytes(lay):
    """the offsets of a proof's path-length bytes"""
    out = set()
    for q in lay["query"]:
        for sp in q["path_len"] + [ly["path_len"] for ly in q["layer"]]:
            out.add(sp[0])
    return out


def word_at(proof, off, plb):
    """(start, value) of the 64-bit word byte `off` is part of - words start right after a path-length byte, or at the start of
    the proof -, or None for a path-length byte; plb: path_length_bytes(lay)"""
    if off in plb:
        return None
    start = max([0] + [b + 1 for b in plb if b < off])
    w0 = off - (off - start) % 8
    return w0, int.from_bytes(proof[w0:w0 + 8], "little")


def shape_args(syn, lay):
    """the descriptor's numbers as tests/tools/layout_check.cpp takes them in its plonk mode"""
    d = syn.desc()
    nc = d.num_challenges
    n_consts = lay["constants"][1] // 16
    return [str(int(x)) for x in (d.degree_bits, d.rate_bits, d.cap_height, d.fri_arity_bits, d.fri_final_poly_bits, d.fri_num_queries,
                                  d.num_public_inputs, n_consts, d.num_routed_wires, d.num_wires, nc, nc * d.num_partial_products,
                                  lay["lookup_zs"][1] // 16, nc * d.quotient_degree_factor)]


assert P == 0xFFFFFFFF00000001
