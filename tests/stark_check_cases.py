"""The yardstick of the STARK trace checker (nlx_stark_check_trace / nlx_stark_check_rounds) and the AIRs its tests share.

check() evaluates a register program on the trace rows in Python integers, through the reference interpreter of
tests/test_stark_cpu.py (run_program), and adds what the checker adds to it: the row predicates of the four filters and the
indexing of the constraints.  tests/test_stark_check_cpu.py pins it against the oracle's prover and verifier;
tests/test_gpu_stark_check.py compares the device's report with it field by field.

Run as a script it records tests/golden/stark_check_cells.json (the oracle's verdicts on the 40 mutated cells)."""
import json
import os
import sys

import numpy as np

from test_stark_cpu import run_program

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "stark_check_cells.json")
P = 0xFFFFFFFF00000001
(LOCAL, NEXT, PUBLIC, CONST, ADD, SUB, MUL, EMIT_TRANSITION, EMIT_FIRST, EMIT_LAST, EMIT, PERIODIC, PACK_LOCAL, PACK_NEXT,
 EMIT_BOOL, LOADV, XOR3, CH, MAJ, SEGMENT, EMIT_LOGUP, MAC) = range(22)
CELLS_SEED, CELLS_LOG_N, N_CELLS = 5, 5, 40


def constraint_table(program):
    """[(kind, word, sub)] per constraint, in emission order over the whole program: kind = the emitting opcode, word = its
    index, sub = the column offset of an EMIT_BOOL, 0 / 1 for the two coefficients of an EMIT_LOGUP, else 0"""
    out, pc = [], 0
    while pc < len(program):
        w = int(program[pc])
        op, b = w & 0xFF, (w >> 40) & 0xFFFF
        if op == CONST:
            pc += 1                      # the immediate is no instruction
        elif EMIT_TRANSITION <= op <= EMIT:
            out.append((op, pc, 0))
        elif op == EMIT_BOOL:
            out += [(op, pc, i) for i in range(max(b, 1))]
        elif op == EMIT_LOGUP:
            out += [(op, pc, 0), (op, pc, 1)]
        pc += 1
    return out


def applies(kind, row, n):
    """the filters as row predicates: a verifier accepts an honest proof exactly when the filtered constraints vanish on H"""
    if kind == EMIT_FIRST:
        return row == 0
    if kind == EMIT_LAST:
        return row == n - 1
    if kind == EMIT_TRANSITION:
        return row < n - 1
    return True                          # EMIT, EMIT_BOOL, EMIT_LOGUP: every row, the wrap at n - 1 included


def check(program, trace, values, periodic=(), period_bits=0, n_public=None, rows=None):
    """The full report for a trace (n_cols, n) - every round's columns - and the values array (public inputs, then round values
    and challenges in the order a prover meets them).  periodic: the flat table, column a at [a * period, (a + 1) * period).
    rows: only these rows (a report on a part of the trace; the default is all of it).
    Returns a dict with the fields of nlx_trace_report and per_constraint."""
    n = trace.shape[1]
    table = constraint_table(program)
    period = 1 << period_bits
    per = [[int(v) for v in periodic[a * period:(a + 1) * period]] for a in range(len(periodic) // period)]
    values = [int(v) for v in values]
    n_public = len(values) if n_public is None else n_public
    counts = [0] * len(table)
    first, rows_bad, pairs_bad = None, 0, 0
    for i in (range(n) if rows is None else rows):
        got = run_program(program, trace[:, i].tolist(), trace[:, (i + 1) % n].tolist(), values, [c[i % period] for c in per], n_public)
        assert len(got) == len(table)
        bad = [k for k, ((_, val), (kind, _, _)) in enumerate(zip(got, table)) if val and applies(kind, i, n)]
        for k in bad:
            counts[k] += 1
        pairs_bad += len(bad)
        rows_bad += 1 if bad else 0
        if bad and first is None:
            kind, word, sub = table[bad[0]]
            first = dict(row=i, constraint=bad[0], kind=kind, word=word, sub=sub, value=got[bad[0]][1])
    rep = dict(satisfied=int(first is None), n_constraints=len(table), rows_bad=rows_bad, pairs_bad=pairs_bad,
               row=0, constraint=0, kind=0, word=0, sub=0, value=0, per_constraint=counts)
    rep.update(first or {})
    return rep


def segment_table_order(program):
    """The program's segments in the order of the device's segment table: sorted by register need (the highest register a
    segment writes, plus one), stable - as nlx_stark_build sorts them.  Returns the list of program-order segment numbers."""
    regs, cur, pc = [], 1, 0
    while pc < len(program):
        w = int(program[pc])
        op, dst = w & 0xFF, (w >> 8) & 0xFFFF
        if op == SEGMENT:
            regs.append(cur)
            cur = 1
        elif op not in (LOADV, EMIT_LOGUP, EMIT_BOOL, EMIT_TRANSITION, EMIT_FIRST, EMIT_LAST, EMIT):
            cur = max(cur, dst + 1)
            pc += op == CONST
        pc += 1
    regs.append(cur)
    return sorted(range(len(regs)), key=lambda i: regs[i])


FIELDS = ("satisfied", "n_constraints", "rows_bad", "pairs_bad", "row", "constraint", "kind", "word", "sub", "value")


def check_stark(stark, trace, values, rows=None):
    return check(stark.program, trace, values, stark.periodic if stark.air._periodic else (), stark.air.period_bits,
                 stark.air.num_public_inputs, rows)


def mutated(trace, col, row, inc=1):
    t = trace.copy()
    t[col, row] = (int(t[col, row]) + inc) % P
    return t


# ---- free_wide_air: wide_air's constraints on the first 32 of 40 columns, so eight columns are unconstrained ----
def free_wide_air(S, segment_nodes=None):
    src = S.wide_air(32)
    air = S.Air(40, 2)
    air.k1 = src.k1
    for g in range(8):
        a, b, c, d = (air.local(4 * g + k) for k in range(4))
        na, nb, nc, nd = (air.next(4 * g + k) for k in range(4))
        air.constraint_transition(na - (a * b + c))
        air.constraint_transition(nb - (b * c + int(air.k1[g])))
        air.constraint_transition(nc - (a + b + c) * d)
        air.constraint(d * (d - 1))
        air.constraint_transition(nd - d)
    air.constraint_first_row(air.local(0) - air.public(0))
    air.constraint_first_row(air.local(1) - air.public(1))
    if segment_nodes is not None:
        air.segment_nodes = segment_nodes
    return air


def free_wide_trace(S, degree_bits):
    """wide_air(32)'s witness and eight columns of anything"""
    t32, pis = S.wide_trace(S.wide_air(32), degree_bits)
    rng = np.random.default_rng(77)
    free = rng.integers(0, P, size=(8, 1 << degree_bits), dtype=np.uint64)
    return np.ascontiguousarray(np.concatenate([t32, free])), pis


def random_cells(log_n=CELLS_LOG_N, seed=CELLS_SEED, count=N_CELLS):
    """[column, row, increment]: the mutated cells, from a fixed seed"""
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(0, 40)), int(rng.integers(0, 1 << log_n)), int(rng.integers(1, P, dtype=np.uint64))] for _ in range(count)]


def oracle_cell_verdicts(nlx, orc):
    """[column, row, increment, 1 if the oracle's verifier accepts the oracle's proof of the mutated trace] per cell"""
    S = nlx.stark
    st = S.Stark(free_wide_air(S), CELLS_LOG_N, S.StarkConfig(fri_num_queries=20))
    trace, pis = free_wide_trace(S, CELLS_LOG_N)
    return [[c, r, inc, int(orc.stark_verify(st.desc, orc.stark_prove(st.desc, mutated(trace, c, r, inc), pis)) == 1)]
            for c, r, inc in random_cells()]


def golden_cells():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- every_op_air: two rounds at 2^4 rows, every opcode of the register program ----
EO_LOG_N = 4
EO_BITS, EO_W, EO_WN, EO_X3, EO_CH, EO_MAJ, EO_ADD, EO_SUB, EO_MAC, EO_PER, EO_ACC, EO_V1, EO_V2 = 0, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22
EO_COLS0 = 23
EO_HPAIR, EO_HONE, EO_RV = EO_COLS0, EO_COLS0 + 2, EO_COLS0 + 4      # round-1 columns
EO_COLS1 = 5
EO_PERIODIC = (3, 1, 4, 1)


def every_op_air(S):
    """Round 0: eleven bit columns, their word (pack, local and next), xor3 / ch / maj of the first three, a shifted add, a
    shifted subtract, a multiply-add, a periodic column of period 4, a running sum pinned to the public inputs at both ends, two
    looked-up columns; two challenges.  Round 1: the LogUp helper of the pair and of the single lookup, and a column that
    repeats the round's one value.  segment_nodes = 6 cuts the program into several segments."""
    air = S.Air(EO_COLS0 + EO_COLS1, 2, rounds=[(EO_COLS0, 2), (EO_COLS1, 0)], round_values=[0, 1])
    L, N = air.local, air.next  # noqa: N806
    per = air.periodic(EO_PERIODIC)
    air.constraint_boolean(EO_BITS, 11)                                   # crosses the kernel's batch of 8
    air.constraint(L(EO_W) - air.pack(EO_BITS, 11))
    air.constraint(L(EO_WN) - air.pack(EO_BITS, 11, next_row=True))
    air.constraint(L(EO_X3) - air.xor3(L(0), L(1), L(2)))
    air.constraint(L(EO_CH) - air.ch(L(0), L(1), L(2)))
    air.constraint(L(0) * (L(1) - L(2)) - (L(EO_CH) - L(2)))              # the same, written out: a plain MUL
    air.constraint(L(EO_MAJ) - air.maj(L(0), L(1), L(2)))
    air.constraint(L(EO_ADD) - (L(EO_W) + L(EO_X3) * 4))                  # a + b * 2^2
    air.constraint(L(EO_SUB) - (L(EO_W) - L(EO_CH) * 8))                  # a - b * 2^3
    air.constraint(L(EO_MAC) - (L(EO_W) * L(EO_X3) + L(EO_MAJ)))          # c + a * b
    air.constraint(L(EO_PER) - (per + L(0) + 5))
    air.constraint_first_row(L(EO_ACC) - air.public(0))
    air.constraint_transition(N(EO_ACC) - L(EO_ACC) - L(EO_W))
    air.constraint_last_row(L(EO_ACC) - air.public(1))
    air.constraint_logup(EO_V1, EO_V2, EO_HPAIR, 0)
    air.constraint_logup(EO_V1, None, EO_HONE, 0)
    air.constraint(L(EO_RV) - air.round_value(1, 0))
    air.segment_nodes = 6
    return air


def _ext_inv(a, b):
    """1 / (a + b X), X^2 = 7"""
    d = pow((a * a - 7 * b * b) % P, P - 2, P)
    return a * d % P, (P - b) * d % P


def every_op_round0(seed=9):
    """(round-0 columns, public inputs)"""
    n = 1 << EO_LOG_N
    rng = np.random.default_rng(seed)
    t = np.zeros((EO_COLS0, n), dtype=np.uint64)
    bits = rng.integers(0, 2, size=(11, n))
    t[:11] = bits
    word = [sum(int(bits[k, i]) << k for k in range(11)) for i in range(n)]
    acc = 17
    for i in range(n):
        x, y, z = (int(bits[k, i]) for k in range(3))
        x3, ch, mj = x ^ y ^ z, (y if x else z), int(x + y + z >= 2)
        t[EO_W, i], t[EO_WN, i] = word[i], word[(i + 1) % n]
        t[EO_X3, i], t[EO_CH, i], t[EO_MAJ, i] = x3, ch, mj
        t[EO_ADD, i], t[EO_SUB, i], t[EO_MAC, i] = word[i] + 4 * x3, (word[i] - 8 * ch) % P, word[i] * x3 + mj
        t[EO_PER, i] = EO_PERIODIC[i % 4] + x + 5
        t[EO_ACC, i] = acc
        acc += word[i]
    t[EO_V1], t[EO_V2] = rng.integers(0, 1 << 16, size=n), rng.integers(0, 1 << 16, size=n)
    return t, np.array([17, int(t[EO_ACC, n - 1])], dtype=np.uint64)


def every_op_round1(t0, known):
    """(round-1 columns, [the round value]) for the challenges known = [alpha0, alpha1]: the h columns in Python integers"""
    n = t0.shape[1]
    a0, a1 = int(known[0]), int(known[1])
    t = np.zeros((EO_COLS1, n), dtype=np.uint64)
    rv = (3 * a0 + 1) % P
    for i in range(n):
        i1 = _ext_inv((a0 + int(t0[EO_V1, i])) % P, a1)
        i2 = _ext_inv((a0 + int(t0[EO_V2, i])) % P, a1)
        t[0, i], t[1, i] = (i1[0] + i2[0]) % P, (i1[1] + i2[1]) % P
        t[2, i], t[3, i] = i1
        t[4, i] = rv
    return t, [rv]


def every_op_round_fn(t0, mutate1=None, mutate_rv=0):
    """round_fn for prove_rounds / check_rounds; mutate1 = (round-1 column, row, increment); mutate_rv is added to the round value"""
    def fn(rnd, known):
        if rnd == 0:
            return t0
        t1, rv = every_op_round1(t0, known)
        if mutate1:
            t1 = mutated(t1, *mutate1)
        return t1, [(rv[0] + mutate_rv) % P]
    return fn


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(HERE, ".."))
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
    import nlxpkg
    import oracle_py
    oracle_py.dll()
    with open(GOLDEN, "w") as f:
        json.dump(oracle_cell_verdicts(nlxpkg.load(), oracle_py), f)
        f.write("\n")
