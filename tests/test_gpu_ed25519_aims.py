"""GPU tests on the aimed Ed25519 slots (tests/ed25519_aims.py).  What checks k_ed_scan4 - four lanes per slot, DPP quad
broadcasts, an LDS addend table, spare quads that redo the last slot - and the row kernel behind it:

  * nlx_ed25519_trace called directly, from one slot (fifteen spare quads, the slot its own predecessor) to two scan blocks, into a
    poisoned host array: every cell equals the Python reference;
  * nlx_ed25519_bind_round on that trace equals binding_columns and the fingerprint;
  * false statements come back as NLX_E_INVAL naming the smallest false slot, and the context goes on to produce the good trace;
  * the prover at its smallest size (2^4 slots, the range table spread over sixteen columns) proves the aimed slots: the extreme
    signed limbs go through the lazily reduced AIR kernels; bytes equal the oracle prover's;
  * nlx_fe25519_ops: fe25519_fast.hpp and the quad moves on the device, at the operands of the host check, against Python integers.

Every comparison is exact.  The reference is CPU work shared over the module (ed25519_aims caches it for the session)."""
import numpy as np
import pytest

import ed25519_aims as aims
import sha2_inputs
from test_ed25519_air import oracle_round1

pytestmark = pytest.mark.gpu

P = aims.P
POISON = 0xDEADDEADDEADDEAD
NLX_E_INVAL = -1


def raw_trace(nlx, ctx, slot_list, log_slots):
    """(return code, trace): nlx_ed25519_trace into a host array in which every cell is poison (the device writes zero into the
    multiplicity columns, so every cell of the result is the device's)"""
    E = nlx.ed25519_air
    words = np.ascontiguousarray(E.slots_to_words(slot_list), dtype=np.uint64)
    assert words.shape == (1 << log_slots, E.SLOT_WORDS)
    out = np.full((E.N_COLS0, E.ROWS << log_slots), POISON, dtype=np.uint64)
    return nlx.lib.dll.nlx_ed25519_trace(ctx.handle, words.ctypes.data, log_slots, out.ctypes.data), out


@pytest.fixture(scope="module")
def traces():
    """device traces by size label, so that the binding round runs on the trace the first test compared"""
    held = {}
    yield held
    held.clear()


def good_trace(nlx, ctx, traces, label):
    if label not in traces:
        _, log_slots, names = next(s for s in aims.SIZES if s[0] == label)
        rc, got = raw_trace(nlx, ctx, aims.slot_list(nlx, names), log_slots)
        ctx.check(rc)
        traces[label] = got
    return traces[label]


@pytest.mark.parametrize("label,log_slots,names", aims.SIZES, ids=[s[0] for s in aims.SIZES])
def test_device_trace_equals_reference(nlx, ctx, traces, label, log_slots, names):
    want = aims.reference(nlx, names)
    got = good_trace(nlx, ctx, traces, label)
    diff = aims.first_difference(nlx, got, want, names)
    assert diff is None, "the device trace differs from the reference at " + diff


@pytest.mark.parametrize("label", ["2^0", "2^4", "2^5"])
def test_binding_round_on_the_device_trace(nlx, ctx, traces, label):
    E = nlx.ed25519_air
    _, log_slots, names = next(s for s in aims.SIZES if s[0] == label)
    t0 = good_trace(nlx, ctx, traces, label)
    n = t0.shape[1]
    for gamma in sha2_inputs.GAMMAS:
        acc = np.full((2, n), POISON, dtype=np.uint64)
        g, total = np.array(gamma, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        ctx.check(nlx.lib.dll.nlx_ed25519_bind_round(ctx.handle, t0.ctypes.data, log_slots, g.ctypes.data, acc.ctypes.data, total.ctypes.data))
        want, want_total = E.binding_columns(t0, gamma)
        if not np.array_equal(acc, want):
            col, row = np.argwhere(acc != want)[0]
            pytest.fail("gamma %r: accumulator column %d differs first at row %d (slot %s): %#x, expected %#x"
                        % (gamma, col, row, names[row // E.ROWS], int(acc[col, row]), int(want[col, row])))
        assert (int(total[0]), int(total[1])) == tuple(want_total) == E.fingerprint(aims.slot_list(nlx, names), gamma), gamma


def test_false_statements_are_named_and_the_context_goes_on(nlx, ctx):
    want = aims.reference(nlx, aims.ORDER)
    for what, replaced, reported in aims.false_statements(nlx):
        rc, _ = raw_trace(nlx, ctx, aims.with_replaced(nlx, replaced), 4)
        assert rc == NLX_E_INVAL, what
        with pytest.raises(nlx.NlxError, match=r"slot %d: the statement is false" % reported):
            ctx.check(rc)
        rc, got = raw_trace(nlx, ctx, aims.slot_list(nlx, aims.ORDER), 4)
        assert rc == 0 and aims.first_difference(nlx, got, want, aims.ORDER) is None, what


def test_prover_at_its_smallest_size(nlx, ctx, orc):
    E = nlx.ed25519_air
    slot_list = aims.slot_list(nlx, aims.ORDER)
    pr = E.Ed25519Prover(ctx, 4, nlx.StarkConfig(fri_num_queries=20))
    assert pr.es.table_cols == 16 and pr.es.layout["n_cols0"] == E.N_COLS0 + 15 and pr.stark.desc.period_bits == 12
    report = pr.check(slot_list)
    assert report.ok and report.n_constraints == pr.es.air.num_constraints, str(report)
    t0 = np.zeros((pr.es.layout["n_cols0"], 1 << 12), dtype=np.uint64)
    t0[:E.N_COLS0] = aims.reference(nlx, aims.ORDER)
    t0[E.MULT:E.MULT + 16] = orc.logup_multiplicities(t0, E.LOOKUPS, 16, 16)
    t0[E.MULT9] = orc.logup_multiplicities(t0, E.LOOKUPS9, 9)
    got = pr.generate_trace(slot_list).cpu().numpy().view(np.uint64)
    diff = aims.first_difference(nlx, got[:E.N_COLS0], t0[:E.N_COLS0], aims.ORDER)
    assert diff is None, diff
    assert np.array_equal(got[E.N_COLS0:], t0[E.N_COLS0:])           # the further multiplicity columns of the spread table
    proof = pr.prove(slot_list)
    assert proof == orc.stark_prove_rounds(pr.stark.desc, lambda rnd, known: t0 if rnd == 0 else oracle_round1(orc, E, t0, known, 16), [])
    assert pr.verify(proof).ok and orc.stark_verify(pr.stark.desc, proof) == 1
    vals = orc.stark_values(pr.stark.desc, proof)
    assert len(vals) == 6 and tuple(vals[4:6]) == E.fingerprint(slot_list, vals[2:4]) == pr.last_total
    pr.close()


@pytest.fixture(scope="module")
def probe_operands():
    ops = aims.device_operands()
    assert len(ops) > 1024 and len(ops) % 4 == 3          # many blocks, and the whole list ends in a partial quad
    values = [(aims.value(a) % P, aims.value(a) * aims.value(b) % P) for a, b in ops]
    return ops, values


@pytest.mark.parametrize("n", [0, 1, 5, 63, 64, 65, None])
def test_field_probe_against_integers(nlx, ctx, probe_operands, n):
    ops, values = probe_operands
    n = len(ops) if n is None else n
    a = np.array([o[0] for o in ops[:n]], dtype=np.int32).reshape(n, 10)
    b = np.array([o[1] for o in ops[:n]], dtype=np.int32).reshape(n, 10)
    out = nlx.fe25519_ops(ctx, a, b)
    assert out.shape == (n, 58)
    got = out.tolist()

    def number(words):
        assert max(words) <= 0xFFFF
        return sum(w << (16 * i) for i, w in enumerate(words))
    for i in range(n):
        va, vab = values[i]
        assert number(got[i][:16]) == va, ("freeze", i, ops[i][0])
        assert number(got[i][16:32]) == vab, ("freeze of the product", i, ops[i])
        limbs = [w - (1 << 32) if w >> 31 else w for w in got[i][32:42]]
        assert aims.value(limbs) % P == vab, ("the product's limbs", i, ops[i])
        aims.assert_mul_limbs_in_bound(limbs, ops[i])
        nxt = min(4 * (i // 4) + (i + 1) % 4, n - 1)      # a lane past n stands for element n - 1
        assert number(got[i][42:58]) == values[nxt][1], ("the next lane's product", i, nxt)


def test_field_probe_refuses_null(nlx, ctx):
    a = np.zeros((1, 10), dtype=np.int32)
    out = np.zeros((1, 58), dtype=np.uint32)
    dll = nlx.lib.dll
    for args in ((None, a.ctypes.data, 1, out.ctypes.data), (a.ctypes.data, None, 1, out.ctypes.data), (a.ctypes.data, a.ctypes.data, 1, None),
                 (None, None, 0, None)):
        assert dll.nlx_fe25519_ops(ctx.handle, *args) == NLX_E_INVAL
    assert dll.nlx_fe25519_ops(ctx.handle, a.ctypes.data, a.ctypes.data, 0, out.ctypes.data) == 0
