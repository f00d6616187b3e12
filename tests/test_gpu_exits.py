"""GPU: every way out of the Goldilocks provers gives the context back what the call took.

On one context: prove once (this builds the lazily made tables), record the bytes in use (nlx_ctx_memory) and the proof bytes, then
take each refusing exit - every one a host-side refusal, none makes the device fail - and require the stated code, the same bytes
in use, and the same proof bytes from a further successful call.  The stage-level calls that hand a commitment out must grow the
bytes in use by exactly that commitment's tables, and give them back when it is closed."""
import ctypes

import numpy as np
import pytest

from conftest import P

pytestmark = pytest.mark.gpu

NLX_E_INVAL, NLX_E_RANGE = -1, -4
BN = "poseidon_bn128"
BASIC = dict(pct_poseidon=20, pct_arithmetic=30, pct_base_sum=5, pct_constant=5)


@pytest.fixture(scope="module")
def own(nlx):
    """a context of this module's own: nothing else allocates on it or closes a handle of it while a test counts bytes"""
    c = nlx.Context(0)
    yield c
    c.close()


def _refused(nlx, code, call):
    with pytest.raises(nlx.NlxError) as e:
        call()
    assert e.value.code == code, e.value
    return e.value


def _exits_give_everything_back(ctx, prove, exits):
    good = prove()
    in_use = ctx.memory()[1]
    assert prove() == good and ctx.memory()[1] == in_use          # the warm state is a fixed point
    for name, take in exits:
        take()
        assert ctx.memory()[1] == in_use, "%s: %d bytes in use, %d before" % (name, ctx.memory()[1], in_use)
        assert prove() == good, name
        assert ctx.memory()[1] == in_use, name
    return good


def _prove_raw(nlx, cd, wires, pis, cap):
    """nlx_prove with a buffer of `cap` bytes: (code, proof_len)"""
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    pis = np.ascontiguousarray(pis, dtype=np.uint64)
    ln = ctypes.c_size_t(12345)
    rc = nlx.lib.dll.nlx_prove(cd.handle, nlx.lib.ptr(wires), nlx.lib.ptr(pis), buf.ctypes.data, cap, ctypes.byref(ln))
    return rc, ln.value


def test_prove_buffer_one_byte_short(nlx, own):
    """(a) nlx_prove, proof_cap one byte short: NLX_E_RANGE after every stage has run"""
    syn = nlx.SyntheticCircuit(10, seed=61)
    cd = nlx.CircuitData.from_synthetic(own, syn)
    size = len(cd.prove(syn.wires, syn.public_inputs))

    def short():
        assert _prove_raw(nlx, cd, syn.wires, syn.public_inputs, size - 1) == (NLX_E_RANGE, 0)
        assert b"proof buffer too small" in nlx.lib.dll.nlx_last_error(own.handle)

    try:
        _exits_give_everything_back(own, lambda: cd.prove(syn.wires, syn.public_inputs), [("proof_cap one byte short", short)])
        assert _prove_raw(nlx, cd, syn.wires, syn.public_inputs, size) == (0, size)
    finally:
        cd.close()


def test_lookup_outside_its_table(nlx, own):
    """(b) a looked-up input outside its table: NLX_E_INVAL after the wires commitment"""
    syn = nlx.SyntheticCircuit(9, seed=5, num_luts=1, lut_bits=6, num_lookups=100)
    cd = nlx.CircuitData.from_synthetic(own, syn)
    w = syn.wires.copy()
    w[0, syn.lookup_rows[0, 0]] = 60000

    def outside():
        assert "not in its table" in str(_refused(nlx, NLX_E_INVAL, lambda: cd.prove(w, syn.public_inputs)))

    try:
        _exits_give_everything_back(own, lambda: cd.prove(syn.wires, syn.public_inputs), [("lookup outside the table", outside)])
    finally:
        cd.close()


def test_bn128_unsatisfied_witness(nlx, own):
    """(c) an unsatisfied witness under the BN128 config: refused by the quotient degree check, with three commitments live"""
    syn = nlx.SyntheticCircuit(7, seed=3, **BASIC)
    cd = nlx.CircuitData.from_synthetic(own, syn, hasher=BN)
    w = syn.wires.copy()
    w[0, 0] = (int(w[0, 0]) + 1) % P
    try:
        _exits_give_everything_back(own, lambda: cd.prove(syn.wires, syn.public_inputs), [
            ("unsatisfied witness", lambda: _refused(nlx, NLX_E_INVAL, lambda: cd.prove(w, syn.public_inputs)))])
    finally:
        cd.close()


def test_stark_rounds_exits(nlx, own):
    """(d) the round callback returns NULL at round 1, after round 0 is committed: NLX_E_INVAL; (e) proof_cap one byte short:
    NLX_E_RANGE.  The two-round LogUp STARK of test_gpu_stark.py at its 2^7 rows."""
    from test_stark_cpu import logup_air, logup_case, logup_rounds
    S = nlx.stark
    st = S.Stark(logup_air(S), 7, S.StarkConfig(fri_num_queries=20))
    rounds = logup_rounds(*logup_case(7))
    pr = st.build(own)
    size = len(pr.prove_rounds(rounds))
    dll = nlx.lib.dll

    def raw(stop_at, cap):
        keep, seen = [], []

        def cb(_user, rnd, ch_ptr, n_ch, _values_out):
            seen.append(rnd)
            if rnd == stop_at:
                return None
            keep.append(np.ascontiguousarray(rounds(rnd, [int(ch_ptr[i]) for i in range(n_ch)]), dtype=np.uint64))
            return keep[-1].ctypes.data

        buf = np.zeros(size, dtype=np.uint8)
        ln = ctypes.c_size_t(12345)
        rc = dll.nlx_stark_prove_rounds(pr.handle, S._ROUND_FN(cb), None, None, buf.ctypes.data, cap, ctypes.byref(ln))
        return rc, ln.value, seen

    def null_round():
        assert raw(1, size) == (NLX_E_INVAL, 0, [0, 1])
        assert b"round 1: the round callback returned NULL" in dll.nlx_last_error(own.handle)

    def short():
        assert raw(None, size - 1) == (NLX_E_RANGE, 0, [0, 1])

    try:
        _exits_give_everything_back(own, lambda: pr.prove_rounds(rounds), [("NULL at round 1", null_round), ("proof_cap one byte short", short)])
        assert raw(None, size)[:2] == (0, size)
    finally:
        pr.close()


def _commit_bytes(nlx, n_cols, log_n, rate_bits, cap_height):
    """device bytes of one commitment: coefficients, LDE table, Merkle digests, each a block of whole 256 bytes"""
    n, L = 1 << log_n, 1 << (log_n + rate_bits)
    blocks = (n_cols * n * 8, n_cols * L * 8, 8 * nlx.lib.dll.nlx_merkle_digest_words(L, cap_height))
    return sum((b + 255) // 256 * 256 for b in blocks)


def test_fri_exit_and_stage_calls(nlx, own):
    """(f) nlx_fri_prove, proof_cap one byte short: NLX_E_RANGE and the caller's challenger is unchanged; (g) the two stage calls
    that return a commitment hold exactly that commitment afterwards"""
    pk = nlx.plonk
    syn = nlx.SyntheticCircuit(10, seed=62)
    cfg = syn.config
    cd = nlx.CircuitData.from_synthetic(own, syn)
    cw = nlx.PolynomialBatch.from_values(own, syn.wires, cfg.rate_bits, cfg.cap_height)
    try:
        zeta = np.array([3, 5], dtype=np.uint64)
        o0 = cw.eval_at(zeta)
        fp = pk.FriParams(cfg.fri_arity_bits, cfg.fri_final_poly_bits, cfg.fri_pow_bits, cfg.fri_num_queries)
        none = np.zeros((0, 2), np.uint64)

        def challenger():
            ch = pk.Challenger()
            ch.observe(np.arange(1, 14, dtype=np.uint64))       # a full absorb and a partly filled input buffer
            return ch

        def fri(cap_bytes=1 << 22, ch=None):
            return pk.fri_prove(own, [cw], [0], zeta, o0, none, fp, ch or challenger(), cap_bytes=cap_bytes)

        size = len(fri())

        def short():
            ch = challenger()
            before = bytes(ch.s)
            _refused(nlx, NLX_E_RANGE, lambda: fri(size - 1, ch))
            assert bytes(ch.s) == before
            assert len(fri(size, ch)) == size and bytes(ch.s) != before      # and the successful call does advance it

        _exits_give_everything_back(own, fri, [("proof_cap one byte short", short)])

        # (g) with the free list empty, every table of the commitment is a block of exactly its size
        b2, g2, a2 = (np.array(v, dtype=np.uint64) for v in ([3, 5], [7, 11], [13, 17]))
        n_zs = cfg.num_challenges * (1 + cfg.num_partial_products)
        n_q = cfg.num_challenges * cfg.quotient_degree_factor
        own.trim()
        base = own.memory()[1]
        cz = cd.partial_products_and_zs(syn.wires, b2, g2)
        assert own.memory()[1] - base == _commit_bytes(nlx, n_zs, 10, cfg.rate_bits, cfg.cap_height)
        own.trim()
        with_zs = own.memory()[1]
        cq = cd.quotient_eval(cw, cz, b2, g2, a2, pk.hash_no_pad(syn.public_inputs))
        assert own.memory()[1] - with_zs == _commit_bytes(nlx, n_q, 10, cfg.rate_bits, cfg.cap_height)
        cq.close()
        assert own.memory()[1] == with_zs
        cz.close()
        assert own.memory()[1] == base
    finally:
        cw.close()
        cd.close()


def test_stark_batch_prove_survives_a_worker_thread_that_does_not_start(nlx):
    """nlx_stark_batch_prove when creating a worker's std::thread fails (simulated: nlx_abi_selftest 3 = the second worker, 4 = the
    first; a host thread failure, no device work is made to fail): the call returns, every job is proved, and the bytes are the
    single-worker ones.  The workers that did start are joined - a joinable std::thread destroyed would be std::terminate."""
    S = nlx.stark
    dll = nlx.lib.dll
    air = S.wide_air(16, seed=4)
    st = S.Stark(air, 9)
    ctxs = [nlx.Context(0) for _ in range(3)]
    prs = [st.build(c) for c in ctxs]
    traces = [S.wide_trace(air, 9, seed=70 + i) for i in range(6)]
    cap = dll.nlx_stark_proof_max_bytes(prs[0].handle)

    def batch(n_workers):
        bufs = [np.zeros(cap, dtype=np.uint8) for _ in traces]
        jobs = (nlx.ProveJob * len(traces))()
        for i, (t, pis) in enumerate(traces):
            jobs[i].wires, jobs[i].public_inputs = t.ctypes.data, pis.ctypes.data
            jobs[i].proof_out, jobs[i].proof_cap = bufs[i].ctypes.data, cap
            jobs[i].status = -99
        handles = (ctypes.c_void_p * n_workers)(*[p.handle for p in prs[:n_workers]])
        assert dll.nlx_stark_batch_prove(handles, n_workers, jobs, len(traces)) == 0
        assert all(jobs[i].status == 0 for i in range(len(traces)))
        return [bufs[i][:jobs[i].proof_len].tobytes() for i in range(len(traces))]

    try:
        expect = batch(1)
        assert len(set(expect)) == len(traces)
        try:
            for kind in (3, 4):
                assert dll.nlx_abi_selftest(kind) == 0
                assert batch(3) == expect, kind
        finally:
            assert dll.nlx_abi_selftest(5) == 0
        assert batch(3) == expect
    finally:
        for p in prs:
            p.close()
        for c in ctxs:
            c.close()
