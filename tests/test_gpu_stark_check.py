"""GPU tests of the STARK trace checker (nlx_stark_check_trace / nlx_stark_check_rounds, StarkProver.check / check_rounds): the
device's report equals the yardstick's (tests/stark_check_cases.py, pinned against the oracle by tests/test_stark_check_cpu.py)
in every field, per_constraint included."""
import ctypes
import hashlib
import struct
import sys

import numpy as np
import pytest

import stark_check_cases as sc
from conftest import P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(nlx):
    return nlx.stark


def same(rep, want, all_fields=True):
    """the device's TraceReport against the yardstick's dict"""
    fields = sc.FIELDS if all_fields else ("satisfied", "n_constraints", "row", "constraint", "kind", "word", "sub", "value")
    got = {k: int(getattr(rep, k)) for k in fields}
    assert got == {k: want[k] for k in fields}
    if all_fields:
        assert rep.per_constraint.tolist() == want["per_constraint"]
    if want["satisfied"]:
        assert rep.ok and rep.message == "" and rep.raise_if_unsatisfied() is rep
    else:
        assert "row %d" % want["row"] in rep.message and "constraint %d" % want["constraint"] in rep.message
        assert "word %d" % want["word"] in rep.message and str(want["value"]) in rep.message
        with pytest.raises(ValueError):
            rep.raise_if_unsatisfied()


def segment_of(program, word):
    """which segment a program word lies in (no CONST immediate of these programs reads as a boundary)"""
    return sum(1 for w in program[:word] if int(w) == sc.SEGMENT)


@pytest.mark.parametrize("db", [4, 10])
def test_fibonacci(S, ctx, db):
    st = S.Stark(S.fibonacci_air(), db, S.StarkConfig(fri_num_queries=20))
    pr = st.build(ctx)
    trace, pis = S.fibonacci_trace(db)
    n = 1 << db
    same(pr.check(trace, pis), sc.check_stark(st, trace, pis))
    bad = sc.mutated(trace, 1, n // 2 + 1)
    want = sc.check_stark(st, bad, pis)
    assert (want["row"], want["rows_bad"]) == (n // 2, 2)
    same(pr.check(bad, pis), want)
    for k in range(3):
        wrong = pis.copy()
        wrong[k] = (int(wrong[k]) + 1) % P
        want = sc.check_stark(st, trace, wrong)
        assert want["row"] == (n - 1 if k == 2 else 0) and want["pairs_bad"] == 1
        same(pr.check(trace, wrong), want)
    pr.close()


@pytest.fixture(scope="module")
def wide6(S, ctx):
    air = sc.free_wide_air(S, segment_nodes=8)
    st = S.Stark(air, 6, S.StarkConfig(fri_num_queries=20))
    assert sum(1 for w in st.program if int(w) & 0xFF == sc.SEGMENT) + 1 >= 3
    trace, pis = sc.free_wide_trace(S, 6)
    pr = st.build(ctx)
    yield st, pr, trace, pis
    pr.close()


def test_golden_cells(wide6):
    st, pr, trace, pis = wide6
    same(pr.check(trace, pis), sc.check_stark(st, trace, pis))
    verdicts = []
    for c, r, inc, _ in sc.golden_cells():
        bad = sc.mutated(trace, c, r, inc)
        want = sc.check_stark(st, bad, pis)
        same(pr.check(bad, pis), want)
        verdicts.append(want["satisfied"])
    assert 5 <= sum(verdicts) <= sc.N_CELLS - 5


def test_lower_index_wins_across_segments(wide6):
    st, pr, trace, pis = wide6
    table = sc.constraint_table(st.program)
    one = {}
    for g in (6, 1):               # the d column of two groups, row 0: constraint 5 g + 2 is the lowest that reads it there
        want = sc.check_stark(st, sc.mutated(trace, 4 * g + 3, 0, 2), pis)
        assert (want["row"], want["constraint"]) == (0, 5 * g + 2)
        one[g] = segment_of(st.program, table[want["constraint"]][1])
    assert one[6] != one[1]
    bad = sc.mutated(sc.mutated(trace, 27, 0, 2), 7, 0, 2)
    want = sc.check_stark(st, bad, pis)
    assert (want["row"], want["constraint"]) == (0, 7)
    same(pr.check(bad, pis), want)
    # and two cells whose constraints' segments the device's table holds in the OPPOSITE order (it is sorted by register need): a
    # checker that took indices or precedence from table positions gives another answer here.  The d cell of group g in row 0
    # fails constraint 5 g + 2 first; in row 1 it fails 5 g + 4 (next.d = d) at row 0
    order = sc.segment_table_order(st.program)
    assert order != sorted(order)
    place = {seg: k for k, seg in enumerate(order)}
    cands = sorted([(5 * g + 2, (4 * g + 3, 0)) for g in range(8)] + [(5 * g + 4, (4 * g + 3, 1)) for g in range(8)])
    table_place = lambda c: place[segment_of(st.program, table[c][1])]   # noqa: E731
    lo, cell_lo, hi, cell_hi = next((a, ca, b, cb) for a, ca in cands for b, cb in cands
                                    if a < b and ca[0] != cb[0] and table_place(a) > table_place(b))
    for cell, c in ((cell_lo, lo), (cell_hi, hi)):
        want = sc.check_stark(st, sc.mutated(trace, *cell, 2), pis)
        assert (want["row"], want["constraint"]) == (0, c)
    bad = sc.mutated(sc.mutated(trace, *cell_hi, 2), *cell_lo, 2)
    want = sc.check_stark(st, bad, pis)
    assert (want["row"], want["constraint"]) == (0, lo)
    same(pr.check(bad, pis), want)


def test_lower_row_wins(wide6):
    st, pr, trace, pis = wide6
    bad = sc.mutated(sc.mutated(trace, 2, 40, 5), 30, 9, 5)        # the later group's cell sits in the earlier row
    want = sc.check_stark(st, bad, pis)
    assert want["row"] == 8 and want["constraint"] >= 35 and want["rows_bad"] == 4
    same(pr.check(bad, pis), want)


@pytest.fixture(scope="module")
def every_op(S, ctx):
    st = S.Stark(sc.every_op_air(S), sc.EO_LOG_N, S.StarkConfig(fri_num_queries=20))
    pr = st.build(ctx)
    t0, pis = sc.every_op_round0()
    yield st, pr, t0, pis
    pr.close()


EO_MUTATIONS = {
    "honest": {},
    "periodic": dict(cell0=(sc.EO_PER, 6, 1)),
    "pack_bit": dict(cell0=(5, 3, 1)),
    "ninth_boolean": dict(cell0=(8, 0, 2)),      # row 0: the row that reads it as `next` is the last one
    "h_pair": dict(mutate1=(0, 5, 1)),
    "h_single": dict(mutate1=(3, 15, 1)),
    "round_value": dict(mutate_rv=1),
}


@pytest.mark.parametrize("challenges", [None, (12345678901234567, 98765432109876543)])
@pytest.mark.parametrize("name", list(EO_MUTATIONS))
def test_every_op_rounds(every_op, name, challenges):
    st, pr, t0, pis = every_op
    m = dict(EO_MUTATIONS[name])
    cell0 = m.pop("cell0", None)
    t0m = sc.mutated(t0, *cell0) if cell0 else t0
    fn, seen = sc.every_op_round_fn(t0m, **m), []

    def spy(rnd, known):
        seen.append((rnd, list(known)))
        return fn(rnd, known)

    rep = pr.check_rounds(spy, pis, challenges)
    assert [r for r, _ in seen] == [0, 1] and seen[0][1] == [] and len(seen[1][1]) == 2     # `known` as in proving
    known = seen[1][1]
    if challenges is not None:
        assert known == list(challenges)
    t1, rv = fn(1, known)
    want = sc.check_stark(st, np.concatenate([t0m, t1]), list(pis) + known + rv)
    assert want["satisfied"] == int(name == "honest")
    if name == "ninth_boolean":
        assert (want["kind"], want["sub"], want["row"]) == (sc.EMIT_BOOL, 8, 0)
    if name.startswith("h_"):
        assert want["kind"] == sc.EMIT_LOGUP
    if name == "round_value":
        assert want["rows_bad"] == 1 << sc.EO_LOG_N
    same(rep, want)
    if challenges is None:                         # deterministic: the same statement and values give the same challenges
        del seen[:]
        pr.check_rounds(spy, pis)
        assert seen[1][1] == known and all(0 < v < P for v in known)


@pytest.fixture(scope="module")
def sha256(nlx, ctx):
    sha = nlx.sha256_air
    sp = sha.Sha256Prover(ctx, 2)
    blocks, first, _ = sha.blocks_for_messages([b"abc"], 2)
    _, digest = sp.generate_trace(blocks, first)
    yield sha, sp, blocks, first, digest
    sp.close()


def test_sha256_trace(nlx, orc, sha256):
    import torch
    sha, sp, blocks, first, digest = sha256
    kernel = nlx.lib.dll.nlx_stark_quotient_kernel(sp.prover.handle)
    assert [int(x) for x in digest] == list(struct.unpack(">8I", hashlib.sha256(b"abc").digest()))
    before = sp.prove_trace(digest)
    rep = sp.check_trace(digest)
    assert rep.ok and rep.n_constraints == sp.stark.air.num_constraints and not rep.per_constraint.any()
    # one flipped bit cell, on the device: the first column under a boolean constraint, row 2
    word = next(w for kind, w, _ in sc.constraint_table(sp.stark.program) if kind == sc.EMIT_BOOL)
    col = (int(sp.stark.program[word]) >> 24) & 0xFFFF
    gamma = [11, 22]
    sp._trace[col, 2] ^= 1
    torch.cuda.synchronize()                       # the library reads on its own stream
    try:
        rep = sp.check_trace(digest, gamma)
        acc, total = sp.round1(gamma)
        full = np.concatenate([sp._trace.cpu().numpy(), acc.cpu().numpy()]).view(np.uint64)
        pis = [int(v) for v in digest]
        want = sc.check_stark(sp.stark, full, pis + gamma + total, rows=range(3))
        assert want["satisfied"] == 0 and want["row"] in (1, 2)
        assert not rep.ok and rep.rows_bad >= 1 and rep.pairs_bad >= rep.rows_bad
        assert int(rep.per_constraint.sum()) == rep.pairs_bad and rep.per_constraint[rep.constraint] >= 1
        same(rep, want, all_fields=False)
        assert rep.site is not None and ".py:" in rep.site
    finally:
        sp._trace[col, 2] ^= 1
    torch.cuda.synchronize()
    assert sp.check_trace(digest).ok
    assert nlx.lib.dll.nlx_stark_quotient_kernel(sp.prover.handle) == kernel
    # nothing is disturbed: the same proof bytes after the checks, and they are the oracle's
    assert sp.prove_trace(digest) == before
    ref_trace, _ = sha.reference_trace(blocks, first)
    assert before == orc.stark_prove_rounds(sp.stark.desc, sha.cpu_rounds(blocks, first, ref_trace), digest)


def test_sha512_and_ed25519_honest_traces(nlx, ctx):
    s5 = nlx.sha512_air
    sp = s5.Sha512Prover(ctx, 2)
    blocks, first, _ = s5.blocks_for_messages([b"abc"], 2)
    _, digest = sp.generate_trace(blocks, first)
    rep = sp.check_trace(s5.digest_halves(digest))
    assert rep.ok and rep.n_constraints == sp.stark.air.num_constraints, str(rep)
    sp.close()
    from test_ed25519_air import rfc_slots
    E = nlx.ed25519_air
    pr = E.Ed25519Prover(ctx, 4)
    slots = (rfc_slots(nlx) + [E.inactive_slot()]) * 4
    rep = pr.check(slots)
    assert rep.ok and rep.n_constraints == pr.stark.air.num_constraints, str(rep)
    pr.close()


def test_proof_bytes_unchanged_by_a_check_and_device_traces(S, ctx, orc):
    import torch
    st = S.Stark(S.fibonacci_air(), 10)
    pr = st.build(ctx)
    trace, pis = S.fibonacci_trace(10)
    before = pr.prove(trace, pis)
    bad = sc.mutated(trace, 0, 77)
    host = pr.check(bad, pis)
    dev = pr.check(torch.from_numpy(bad.view(np.int64)).cuda(), pis)
    assert not host.ok and host.row == 76
    assert bytes(host) == bytes(dev) and host.per_constraint.tolist() == dev.per_constraint.tolist() and host.message == dev.message
    assert pr.check(torch.from_numpy(trace.view(np.int64)).cuda(), pis).ok
    assert pr.prove(trace, pis) == before == orc.stark_prove(st.desc, trace, pis)
    pr.close()


def test_arguments(nlx, S, ctx, every_op):
    dll = nlx.lib.dll
    st = S.Stark(S.fibonacci_air(), 4)
    pr = st.build(ctx)
    trace, pis = S.fibonacci_trace(4)
    rep = S.TraceReport()
    assert dll.nlx_stark_num_constraints(pr.handle) == 5 and dll.nlx_stark_num_constraints(None) == 0
    assert dll.nlx_stark_check_trace(pr.handle, trace.ctypes.data, pis.ctypes.data, None, None) == -1          # NLX_E_INVAL
    rep.satisfied = rep.row = 7
    assert dll.nlx_stark_check_trace(pr.handle, None, pis.ctypes.data, ctypes.byref(rep), None) == -1
    assert (rep.satisfied, rep.row) == (0, 0)                                      # zero-filled before anything else
    assert dll.nlx_stark_check_trace(pr.handle, trace.ctypes.data, None, ctypes.byref(rep), None) == -1        # it has public inputs
    rep.satisfied = rep.row = 7
    assert dll.nlx_stark_check_trace(None, trace.ctypes.data, pis.ctypes.data, ctypes.byref(rep), None) == -1
    assert (rep.satisfied, rep.row) == (0, 0)                                      # also without a handle
    big = pis.copy()
    big[0] = P
    assert dll.nlx_stark_check_trace(pr.handle, trace.ctypes.data, big.ctypes.data, ctypes.byref(rep), None) == -4      # NLX_E_RANGE
    assert dll.nlx_stark_check_rounds(pr.handle, None, None, pis.ctypes.data, None, ctypes.byref(rep), None) == -1
    assert dll.nlx_stark_check_trace(pr.handle, trace.ctypes.data, pis.ctypes.data, ctypes.byref(rep), None) == 0 and rep.satisfied == 1
    pr.close()
    # a two-round STARK is not checked through the single-round entry
    st2, pr2, t0, pis2 = every_op
    assert dll.nlx_stark_check_trace(pr2.handle, t0.ctypes.data, pis2.ctypes.data, ctypes.byref(rep), None) == -1
    assert b"nlx_stark_check_rounds" in dll.nlx_last_error(ctx.handle)
    # a callback that returns NULL: the message of proving
    null_fn = S._ROUND_FN(lambda *a: None)
    assert dll.nlx_stark_check_rounds(pr2.handle, null_fn, None, pis2.ctypes.data, None, ctypes.byref(rep), None) == -1
    assert dll.nlx_last_error(ctx.handle) == b"round 0: the round callback returned NULL"
    # a round function that raises: the exception comes through and the prover goes on working
    def boom(rnd, known):
        if rnd == 1:
            raise KeyError("round 1")
        return t0
    with pytest.raises(KeyError):
        pr2.check_rounds(boom, pis2)
    assert pr2.check_rounds(sc.every_op_round_fn(t0), pis2).ok
    with pytest.raises(ValueError):
        pr2.check_rounds(sc.every_op_round_fn(t0), pis2, [1])


def test_site(S, ctx):
    air = S.Air(2, 0)
    air.constraint(air.local(0) - air.local(1))
    line = sys._getframe().f_lineno + 1
    air.constraint_transition(air.next(0) - air.local(0) - 1)
    st = S.Stark(air, 4)
    trace = np.stack([np.arange(16, dtype=np.uint64)] * 2)
    bad = sc.mutated(trace, 0, 9, 3)
    bad[1, 9] = bad[0, 9]                       # constraint 0 holds everywhere: the transition into row 9 is what breaks
    pr = st.build(ctx)
    assert pr.check(trace).site is None
    rep = pr.check(bad)
    assert (rep.row, rep.constraint, rep.kind_name) == (8, 1, "transition")
    assert rep.site == "%s:%d" % (__file__, line) and rep.site in str(rep)
    pr.close()
    pr = S.Stark(air, 4, program=st.program.copy()).build(ctx)
    rep = pr.check(bad)
    assert (rep.row, rep.constraint) == (8, 1) and rep.site is None
    pr.close()
