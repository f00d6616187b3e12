"""GPU: whole plonky2 proofs under plonky2x's PoseidonBN128GoldilocksConfig (nlx_circuit_build_hasher, hasher 1) against the pure
Python model of the config and its proof replay verifier (tools/bn128_config_model.py), with every committed polynomial pinned to
the frozen oracle's for the transcript's own challenges.  All comparisons are exact.  The model costs 1-2 ms per permutation:
each test stays below about 20 000 of them."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, P, POW2_GEN, rand_field

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn128_config_model as cm  # noqa: E402

m = cm.m
pytestmark = pytest.mark.gpu

R = cm.R
NLX_E_INVAL, NLX_E_RANGE, NLX_E_UNSUPPORTED = -1, -4, -5
BN, GOLD = "poseidon_bn128", "poseidon_goldilocks"
BASIC = dict(pct_poseidon=20, pct_arithmetic=30, pct_base_sum=5, pct_constant=5)
OUTER = dict(pct_poseidon=25, pct_arithmetic=20, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=10, pct_u32=15)


def _ints(words):
    return [m.from_words(w) for w in np.asarray(words).reshape(-1, 4)]


def _model_cap(leaves, cap_height):
    return m.merkle_digests([[int(v) for v in row] for row in leaves], cap_height)[-1]


def _eval(coeffs, z):
    import oracle_py
    return oracle_py.eval_poly_ext(coeffs, z)


def _check_openings(t, cs_c, w_c, z_c, q_c, sh, rows=None):
    """every opening of the proof = the Horner value of the oracle's coefficients (`rows`: sample that many per group);
    the *_c are sequences of coefficient vectors or, where only a sample is wanted, (length, getter) pairs"""
    class Lazy:
        def __init__(self, n, get, lo=0):
            self.n, self.get, self.lo = n, get, lo

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            if isinstance(i, slice):
                lo, hi, _ = i.indices(self.n)
                return Lazy(hi - lo, self.get, self.lo + lo)
            return self.get(self.lo + i)
    cs_c, w_c, z_c, q_c = (Lazy(*x) if isinstance(x, tuple) else x for x in (cs_c, w_c, z_c, q_c))
    op = t["proof"]["openings"]
    zeta = t["zeta"]
    g = pow(POW2_GEN, 1 << (32 - sh.degree_bits), P)
    gzeta = (zeta[0] * g % P, zeta[1] * g % P)
    nc = sh.nc
    groups = [("constants_sigmas", cs_c, zeta), ("wires", w_c, zeta), ("zs", z_c[:nc], zeta), ("zs_next", z_c[:nc], gzeta),
              ("partial_products", z_c[nc:], zeta), ("quotient", q_c, zeta)]
    rng = np.random.default_rng(99)
    for name, polys, at in groups:
        assert len(op[name]) == len(polys), name
        idx = range(len(polys)) if rows is None or len(polys) <= rows else sorted(rng.choice(len(polys), rows, replace=False))
        for i in idx:
            assert op[name][i] == tuple(_eval(polys[i], at)), "%s[%d]" % (name, i)


def _ifft_rows(orc, values):
    return np.stack([orc.fft(col, inverse=True) for col in values])


def _oracle_polys(orc, syn, t):
    """the frozen oracle's polynomials for the replayed challenges: (wires coefficients, Zs / partial products on H, their
    coefficients, quotient chunk coefficients)"""
    oc = orc.Circuit.from_synthetic(syn)
    w_c = _ifft_rows(orc, syn.wires)
    zs = oc.partial_products_and_zs(syn.wires, t["betas"], t["gammas"])
    z_c = _ifft_rows(orc, zs)
    q = oc.quotient_polys(w_c, z_c, t["betas"], t["gammas"], t["alphas"], np.array(t["public_inputs_hash"], dtype=np.uint64))
    oc.close()
    return w_c, zs, z_c, q


def _cs_values(syn):
    return np.ascontiguousarray(np.concatenate([syn.constants, syn.sigmas]))


# ---- 1. whole proof, everything against the model ----
@pytest.fixture(scope="module")
def small(nlx, ctx, orc):
    syn = nlx.SyntheticCircuit(5, seed=505, **BASIC)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=BN)
    proof = cd.prove(syn.wires, syn.public_inputs)
    c = syn.config
    cs = orc.commit(_cs_values(syn), c.rate_bits, c.cap_height)
    cs_cap = _model_cap(cs["leaves"], c.cap_height)
    out = dict(syn=syn, proof=proof, cs=cs, cs_cap=cs_cap, sh=cm.Shape.from_synthetic(syn),
               digest=m.from_words(cd.circuit_digest), dev_cap=_ints(cd.constants_sigmas_cap), hasher=cd.hasher)
    cd.close()
    return out


def test_whole_proof_equals_model(small, orc):
    syn, sh, proof = small["syn"], small["sh"], small["proof"]
    c = syn.config
    assert small["hasher"] == BN
    assert sh.n_rounds == 0                                  # this size has no reduction round: test_commit_phase_trees covers them
    assert small["dev_cap"] == small["cs_cap"]
    assert small["digest"] == cm.circuit_digest(small["cs_cap"], syn.log_n)
    t = cm.verify(proof, sh, small["digest"], small["cs_cap"])
    p = t["proof"]
    assert p["public_inputs"] == [int(x) for x in syn.public_inputs]
    w_c, zs, z_c, q = _oracle_polys(orc, syn, t)
    wc, zc = orc.commit(syn.wires, c.rate_bits, c.cap_height), orc.commit(zs, c.rate_bits, c.cap_height)
    assert np.array_equal(wc["coeffs"], w_c) and np.array_equal(zc["coeffs"], z_c)
    assert p["wires_cap"] == _model_cap(wc["leaves"], c.cap_height)
    assert p["zs_cap"] == _model_cap(zc["leaves"], c.cap_height)
    qc = orc.commit(q, c.rate_bits, c.cap_height, from_coeffs=True)
    assert p["quotient_cap"] == _model_cap(qc["leaves"], c.cap_height)
    _check_openings(t, small["cs"]["coeffs"], w_c, z_c, q, sh)


# ---- 2. commit-phase trees ----
@pytest.mark.parametrize("log_n,cfg,rounds", [
    (8, dict(fri_arity_bits=2, fri_final_poly_bits=2, cap_height=2, fri_num_queries=11, fri_pow_bits=8), 3),
    (12, dict(), 2),
    (9, dict(fri_arity_bits=3, fri_final_poly_bits=3, cap_height=2, fri_num_queries=9, fri_pow_bits=8), 2),
])
def test_commit_phase_trees(nlx, ctx, orc, log_n, cfg, rounds):
    syn = nlx.SyntheticCircuit(log_n, seed=600 + log_n, config=nlx.CircuitConfig(**cfg), **BASIC)
    c = syn.config
    sh = cm.Shape.from_synthetic(syn)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=BN)
    proof = cd.prove(syn.wires, syn.public_inputs)
    pb = nlx.PolynomialBatch

    def cap_of(data, from_coeffs=False):
        b = (pb.from_coeffs if from_coeffs else pb.from_values)(ctx, np.ascontiguousarray(data), c.rate_bits, c.cap_height, hasher=BN)
        cap, coeffs = _ints(b.cap), (None if from_coeffs else b.coeffs())
        b.close()
        return cap, coeffs

    cs_cap, cs_coeffs = cap_of(_cs_values(syn))
    assert _ints(cd.constants_sigmas_cap) == cs_cap
    digest = m.from_words(cd.circuit_digest)
    assert digest == cm.circuit_digest(cs_cap, log_n)
    t = cm.verify(proof, sh, digest, cs_cap)
    p = t["proof"]
    assert sh.n_rounds == rounds and len(p["commit_caps"]) == rounds
    assert all(len(q["steps"]) == rounds and len(q["steps"][0][0]) == 1 << c.fri_arity_bits for q in p["queries"])
    w_c, zs, z_c, q = _oracle_polys(orc, syn, t)
    assert p["wires_cap"] == cap_of(syn.wires)[0]
    assert p["zs_cap"] == cap_of(zs)[0]
    assert p["quotient_cap"] == cap_of(q, from_coeffs=True)[0]
    assert np.array_equal(cs_coeffs, _ifft_rows(orc, _cs_values(syn)))
    _check_openings(t, cs_coeffs, w_c, z_c, q, sh, rows=None if log_n <= 9 else 6)
    cd.close()


# ---- 3. / 4. the stage seam ----
def _stagewise(nlx, ctx, syn, cd, hasher, fri=None):
    """the proof assembled through the stage entries with a host Challenger, as tests/test_gpu_stages.py does"""
    pk = nlx.plonk
    cfg = syn.config
    nc, log_n = cfg.num_challenges, syn.log_n
    out = bytearray()
    ch = pk.Challenger()
    pih = pk.hash_no_pad(syn.public_inputs)
    cw = nlx.PolynomialBatch.from_values(ctx, syn.wires, cfg.rate_bits, cfg.cap_height, hasher=hasher)
    out += cw.cap.tobytes()
    ch.observe_hash(cd.circuit_digest, hasher)
    ch.observe(pih)
    ch.observe_hash(cw.cap, hasher)
    b2, g2, a2 = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    b2[:nc], g2[:nc] = ch.challenges(nc), ch.challenges(nc)
    cz = cd.partial_products_and_zs(syn.wires, b2, g2)
    assert cz.hasher == hasher
    out += cz.cap.tobytes()
    ch.observe_hash(cz.cap, hasher)
    a2[:nc] = ch.challenges(nc)
    cq = cd.quotient_eval(cw, cz, b2, g2, a2, pih)
    assert cq.hasher == hasher
    out += cq.cap.tobytes()
    ch.observe_hash(cq.cap, hasher)
    zeta = ch.challenges(2)
    g = pow(POW2_GEN, 1 << (32 - log_n), P)
    gzeta = np.array([int(zeta[0]) * g % P, int(zeta[1]) * g % P], dtype=np.uint64)
    cs = cd.constants_sigmas_batch()
    assert cs.hasher == hasher
    o_cs, o_w, o_zs, o_q = (b.eval_at(zeta) for b in (cs, cw, cz, cq))
    o_next = cz.eval_at(gzeta)[:nc]
    out += o_cs.tobytes() + o_w.tobytes() + o_zs[:nc].tobytes() + o_next.tobytes() + o_zs[nc:].tobytes() + o_q.tobytes()
    openings_zeta = np.concatenate([o_cs, o_w, o_zs, o_q])
    ch.observe(openings_zeta)
    ch.observe(o_next)
    fp = pk.FriParams(cfg.fri_arity_bits, cfg.fri_final_poly_bits, cfg.fri_pow_bits, cfg.fri_num_queries)
    fri = fri or (lambda *a: pk.fri_prove(*a, hasher=hasher))
    out += fri(ctx, [cs, cw, cz, cq], [0, 0, nc, 0], zeta, openings_zeta, o_next, fp, ch)
    out += np.uint64(syn.public_inputs.size).tobytes() + syn.public_inputs.tobytes()
    return bytes(out), (cw, cz, cq, cs)


@pytest.mark.parametrize("log_n", [8, 5])
def test_stage_seam_reproduces_the_whole_proof(nlx, ctx, log_n):
    pk = nlx.plonk
    syn = nlx.SyntheticCircuit(log_n, seed=300 + log_n, **BASIC)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=BN)
    want = cd.prove(syn.wires, syn.public_inputs)
    got, (cw, cz, cq, cs) = _stagewise(nlx, ctx, syn, cd, BN)
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        pytest.fail("stage-wise BN128 proof differs from nlx_prove, first at byte %d of %d" % (int(np.nonzero(a != b)[0][0]), len(want)))
    # mismatched hashers are refused
    cfg = syn.config
    z = np.zeros(2, np.uint64)
    gw = nlx.PolynomialBatch.from_values(ctx, syn.wires, cfg.rate_bits, cfg.cap_height)           # a Goldilocks commitment
    with pytest.raises(nlx.NlxError) as e:
        cd.quotient_eval(gw, cz, z, z, z, np.zeros(4, np.uint64))
    assert e.value.code == NLX_E_UNSUPPORTED
    with pytest.raises(nlx.NlxError) as e:
        cd.quotient_eval(cw, gw, z, z, z, np.zeros(4, np.uint64))
    assert e.value.code == NLX_E_UNSUPPORTED
    fp = pk.FriParams(cfg.fri_arity_bits, cfg.fri_final_poly_bits, cfg.fri_pow_bits, cfg.fri_num_queries)
    n_w = syn.wires.shape[0]
    o0, o1 = np.zeros((2 * n_w, 2), np.uint64), np.zeros((0, 2), np.uint64)
    with pytest.raises(nlx.NlxError) as e:
        pk.fri_prove(ctx, [cw, gw], [0, 0], z, o0, o1, fp, pk.Challenger(), hasher=BN)
    assert e.value.code == NLX_E_UNSUPPORTED
    with pytest.raises(nlx.NlxError) as e:
        pk.fri_prove(ctx, [cw], [0], z, o0[:n_w], o1, fp, pk.Challenger(), hasher=GOLD)
    assert e.value.code == NLX_E_UNSUPPORTED
    # hasher 7
    dll = nlx.lib.dll
    h = ctypes.c_void_p()
    d = syn.desc()
    assert dll.nlx_circuit_build_hasher(ctx.handle, ctypes.byref(d), syn.constants.ctypes.data, syn.sigmas.ctypes.data, 7, ctypes.byref(h)) == NLX_E_RANGE
    hs = (ctypes.c_void_p * 1)(cw.handle)
    nn = (ctypes.c_uint32 * 1)(0)
    buf = np.zeros(1 << 20, np.uint8)
    ln = ctypes.c_size_t()
    chal = pk.Challenger()
    assert dll.nlx_fri_prove_hasher(ctx.handle, hs, 1, nn, z.ctypes.data, o0.ctypes.data, None, ctypes.byref(fp), 7, ctypes.byref(chal.s),
                                    buf.ctypes.data, buf.size, ctypes.byref(ln)) == NLX_E_RANGE
    with pytest.raises(ValueError):
        nlx.CircuitData.from_synthetic(ctx, syn, hasher="sha256")
    for b in (cw, cz, cq, gw):
        b.close()
    cd.close()


def test_goldilocks_through_the_new_entries(nlx, ctx):
    """hasher 0 of nlx_circuit_build_hasher / nlx_fri_prove_hasher gives the bytes of the old entries"""
    pk, dll = nlx.plonk, nlx.lib.dll
    syn = nlx.SyntheticCircuit(8, seed=41, **BASIC)
    cd = nlx.CircuitData.from_synthetic(ctx, syn)
    want = cd.prove(syn.wires, syn.public_inputs)
    assert cd.hasher == GOLD
    h = ctypes.c_void_p()
    d = syn.desc()
    assert dll.nlx_circuit_build_hasher(ctx.handle, ctypes.byref(d), syn.constants.ctypes.data, syn.sigmas.ctypes.data, 0, ctypes.byref(h)) == 0
    assert dll.nlx_circuit_hasher(h) == 0
    dig = np.zeros(4, np.uint64)
    dll.nlx_circuit_digest(h, dig.ctypes.data)
    assert np.array_equal(dig, cd.circuit_digest)
    buf = np.zeros(dll.nlx_proof_max_bytes(h), np.uint8)
    ln = ctypes.c_size_t()
    assert dll.nlx_prove(h, syn.wires.ctypes.data, syn.public_inputs.ctypes.data, buf.ctypes.data, buf.size, ctypes.byref(ln)) == 0
    assert buf[:ln.value].tobytes() == want
    dll.nlx_circuit_destroy(h)

    def fri0(ctx_, oracles, n_next, zeta, o0, o1, fp, ch):
        hs = (ctypes.c_void_p * len(oracles))(*[o.handle for o in oracles])
        nn = (ctypes.c_uint32 * len(oracles))(*n_next)
        z = np.ascontiguousarray(zeta, dtype=np.uint64)
        a, b = np.ascontiguousarray(o0.reshape(-1)), np.ascontiguousarray(o1.reshape(-1))
        out = np.zeros(1 << 22, np.uint8)
        n = ctypes.c_size_t()
        assert dll.nlx_fri_prove_hasher(ctx_.handle, hs, len(oracles), nn, z.ctypes.data, a.ctypes.data, b.ctypes.data, ctypes.byref(fp), 0,
                                        ctypes.byref(ch.s), out.ctypes.data, out.size, ctypes.byref(n)) == 0
        return out[:n.value].tobytes()

    got, batches = _stagewise(nlx, ctx, syn, cd, GOLD, fri=fri0)
    assert got == want
    for b in batches[:3]:
        b.close()
    cd.close()


# ---- 5. refusals at build ----
def test_build_refusals(nlx, ctx):
    lk = nlx.SyntheticCircuit(9, seed=5, num_luts=1, lut_bits=6, num_lookups=100)
    with pytest.raises(nlx.NlxError) as e:
        nlx.CircuitData.from_synthetic(ctx, lk, hasher=BN)
    assert e.value.code == NLX_E_UNSUPPORTED
    nlx.CircuitData.from_synthetic(ctx, lk).close()                       # the Goldilocks config takes it
    # num_challenges * quotient_degree_factor <= 4: a quotient leaf would be its own digest
    narrow = nlx.SyntheticCircuit(6, seed=6, config=nlx.CircuitConfig(num_challenges=1, rate_bits=2, quotient_degree_factor=4), **BASIC)
    with pytest.raises(nlx.NlxError) as e:
        nlx.CircuitData.from_synthetic(ctx, narrow, hasher=BN)
    assert e.value.code == NLX_E_UNSUPPORTED


def test_unsatisfied_witness_is_refused(nlx, ctx, orc):
    """An unsatisfied witness gives NLX_E_INVAL under the BN128 config (the quotient degree check of csrc/prover.hip: the top
    quotient_degree_factor coefficients of the quotient must be zero).  Which witnesses are unsatisfied is decided by the frozen
    oracle's verifier on the Goldilocks proof of the same witness: the issue's mutation (wire 0 of row 0), and single cells
    changed at random - a cell no constraint reads leaves the witness satisfied, and then the BN128 proof must come back."""
    syn = nlx.SyntheticCircuit(7, seed=3, **BASIC)
    gold = nlx.CircuitData.from_synthetic(ctx, syn)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=BN)
    ref = orc.Circuit.from_synthetic(syn)
    sh = cm.Shape.from_synthetic(syn)
    rng = np.random.default_rng(55)
    cells = [(0, 0)] + [(int(rng.integers(0, 135)), int(rng.integers(0, 1 << 7))) for _ in range(24)]
    refused = accepted = 0
    try:
        for col, row in cells:
            w = syn.wires.copy()
            w[col, row] = (int(w[col, row]) + 1 + int(rng.integers(0, 5))) % P
            satisfied = ref.verify(gold.prove(w, syn.public_inputs)) == 1
            if satisfied:
                proof = cd.prove(w, syn.public_inputs)
                assert len(cm.parse_proof(proof, sh)["queries"]) == sh.num_queries, (col, row)
                accepted += 1
            else:
                with pytest.raises(nlx.NlxError) as e:
                    proof = cd.prove(w, syn.public_inputs)
                    print("unsatisfied witness (wire %d, row %d): nlx_prove returned NLX_OK and %d proof bytes" % (col, row, len(proof)))
                assert e.value.code == NLX_E_INVAL, (col, row)
                refused += 1
        print("unsatisfied witnesses refused: %d, satisfied ones proved: %d" % (refused, accepted))
        assert refused >= 1                                   # wire 0 of row 0 at the least
        # the stage entry refuses the same way: Zs and quotient of the issue's witness
        w = syn.wires.copy()
        w[0, 0] = (int(w[0, 0]) + 1) % P
        cfg = syn.config
        cw = nlx.PolynomialBatch.from_values(ctx, w, cfg.rate_bits, cfg.cap_height, hasher=BN)
        b2, g2, a2 = (np.array(v, dtype=np.uint64) for v in ([3, 5], [7, 11], [13, 17]))
        cz = cd.partial_products_and_zs(w, b2, g2)
        with pytest.raises(nlx.NlxError) as e:
            cd.quotient_eval(cw, cz, b2, g2, a2, nlx.plonk.hash_no_pad(syn.public_inputs))
        assert e.value.code == NLX_E_INVAL
        cw.close()
        cz.close()
        # and the satisfied witness is still proved afterwards
        assert len(cd.prove(syn.wires, syn.public_inputs)) > 0
    finally:
        ref.close()
        gold.close()
        cd.close()


# ---- 6. the lane-split kernel ----
def _edge_digest_rows():
    """rows of four words that ARE their digests (hash_or_noop's no-op branch): the extremes a two_to_one can meet.  A row's
    words are Goldilocks elements, so limbs all at the mask cannot be written as a row; p - 1 in every word is the nearest."""
    top = (R >> 192) - 1
    vals = [R - 1, 0, 1, R - 2, (P - 1) | ((P - 1) << 64) | ((P - 1) << 128) | (top << 192), (P - 1) << 128]
    rows = []
    for v in vals:
        w = m.to_words(v)
        assert all(x < P for x in w), hex(v)
        rows.append(w)
    return rows


def _levels_of(tree, n_leaves, cap_height):
    out, off, lv = [], 0, n_leaves
    while lv >= (1 << cap_height):
        out.append(_ints(tree.digests[off:off + 4 * lv]))
        off += 4 * lv
        lv >>= 1
    assert off == tree.digests.size
    return out


def test_quad_kernel_equals_one_lane_kernel_and_model(nlx, monkeypatch):
    rng = np.random.default_rng(66)
    ctxs = {}
    for name, val in (("quad", str(1 << 30)), ("one_lane", "0")):
        monkeypatch.setenv("NLX_PBN_QUAD_MAX_PARENTS", val)
        ctxs[name] = nlx.Context(0)
    monkeypatch.delenv("NLX_PBN_QUAD_MAX_PARENTS")
    try:
        edges = _edge_digest_rows()
        # 2^10 leaves of four words: every level against the model, with every ordered pair of extremes among the siblings
        leaves = rand_field(rng, (1 << 10, 4))
        leaves[:, 3] %= np.uint64(R >> 192)
        k = 0
        for a in edges:
            for b in edges:
                leaves[2 * k], leaves[2 * k + 1] = a, b
                k += 1
        leaves[-2], leaves[-1] = edges[0], edges[0]
        want = m.merkle_digests([[int(v) for v in row] for row in leaves], 0)
        for name, c in ctxs.items():
            t = nlx.MerkleTree(c, leaves, 0, hasher=BN)
            assert _levels_of(t, 1 << 10, 0) == want, name
        # 2^17 leaves of 9 words (hashed leaves): the two settings agree level by level
        big = rand_field(rng, (1 << 17, 9))
        trees = {name: nlx.MerkleTree(c, big, 3, hasher=BN) for name, c in ctxs.items()}
        la, lb = _levels_of(trees["quad"], 1 << 17, 3), _levels_of(trees["one_lane"], 1 << 17, 3)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert x == y, "level %d" % i
        # a whole proof with commit-phase rounds (the quad leaf kernel runs there) is byte-equal
        syn = nlx.SyntheticCircuit(10, seed=610, config=nlx.CircuitConfig(fri_arity_bits=3, fri_final_poly_bits=2), **BASIC)
        proofs = {}
        for name, c in ctxs.items():
            cd = nlx.CircuitData.from_synthetic(c, syn, hasher=BN)
            proofs[name] = cd.prove(syn.wires, syn.public_inputs)
            cd.close()
        assert cm.Shape.from_synthetic(syn).n_rounds >= 2
        assert proofs["quad"] == proofs["one_lane"]
        for ab in (2, 4):
            syn = nlx.SyntheticCircuit(9, seed=611 + ab, config=nlx.CircuitConfig(fri_arity_bits=ab, fri_final_poly_bits=1, cap_height=1), **BASIC)
            got = []
            for name, c in ctxs.items():
                cd = nlx.CircuitData.from_synthetic(c, syn, hasher=BN)
                got.append(cd.prove(syn.wires, syn.public_inputs))
                cd.close()
            assert got[0] == got[1], "arity_bits %d" % ab
    finally:
        for c in ctxs.values():
            c.close()


# ---- 7. the outer workload's size ----
def test_proof_at_2p16_rows(nlx, ctx, orc):
    syn = nlx.SyntheticCircuit(16, seed=1616, num_public_inputs=64, **OUTER)
    sh = cm.Shape.from_synthetic(syn)
    cd = nlx.CircuitData.from_synthetic(ctx, syn, hasher=BN)
    proof = cd.prove(syn.wires, syn.public_inputs)
    cs_cap = _ints(cd.constants_sigmas_cap)
    digest = m.from_words(cd.circuit_digest)
    assert digest == cm.circuit_digest(cs_cap, 16)
    cd.close()
    assert sh.n_rounds == 3
    t = cm.verify(proof, sh, digest, cs_cap)
    w_c, zs, z_c, q = _oracle_polys(orc, syn, t)
    cs_v = _cs_values(syn)
    _check_openings(t, (len(cs_v), lambda i: orc.fft(cs_v[i], inverse=True)), w_c, z_c, q, sh, rows=2)


# ---- 8. the replay verifier can say no ----
def test_replay_verifier_rejects_mutations(small):
    sh, proof = small["sh"], small["proof"]
    off = cm.parse_proof(proof, sh)["offsets"]
    ncap = 1 << small["syn"].config.cap_height

    def flipped(pos):
        b = bytearray(proof)
        b[pos] ^= 1
        return bytes(b)

    nonce_at = off["pow_witness"][0]
    changed_nonce = bytearray(proof)
    nonce = int.from_bytes(proof[nonce_at:nonce_at + 8], "little")
    changed_nonce[nonce_at:nonce_at + 8] = ((nonce + 1) % P).to_bytes(8, "little")
    mutations = {
        "a byte of the wires cap": flipped(off["caps"][0] + 5),
        "a byte of the quotient cap": flipped(off["caps"][0] + 2 * 32 * ncap + 40),
        "a byte of an opening": flipped(off["openings"][0] + 16 * 7 + 3),
        "a byte of a Merkle sibling": flipped(off["first_sibling"][0] + 9),
        "a byte of the final polynomial": flipped(off["final_poly"][0] + 17),
        "the nonce": bytes(changed_nonce),
    }
    cm.verify(proof, sh, small["digest"], small["cs_cap"])   # the unmutated proof is accepted
    for name, bad in mutations.items():
        with pytest.raises(cm.Reject):
            cm.verify(bad, sh, small["digest"], small["cs_cap"])
            print("accepted:", name)
