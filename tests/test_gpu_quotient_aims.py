"""The quotient (k_quotient, k_quotient_poseidon) and Z / partial-product (k_zs_row_products) stages on witnesses aimed at their
worst cases (tests/quotient_aims.py): whole proofs must give the oracle's bytes, the stage calls the oracle's stage entries
(orc_partial_products_and_zs, orc_quotient_polys), with PoseidonGate's partial rounds in their own kernel and inside k_quotient
(NLX_QUOTIENT_POSEIDON_INLINE, read at circuit build)."""
import numpy as np
import pytest

import quotient_aims as qa
from conftest import P, rand_field

pytestmark = pytest.mark.gpu

SHAPES = [
    (9, dict(pct_poseidon=10, pct_arithmetic=10, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=20, pct_u32=30)),  # all 19 gates
    (10, dict(pct_poseidon=30, pct_arithmetic=30, pct_base_sum=5, pct_constant=5)),                                            # Poseidon-heavy
]
CONSTANT_EDGES = (P - 1, qa.EPS, qa.EPS + 1)
PIH_EDGE = [P - 1, 0, qa.EPS, qa.EPS + 1]


def _same(got, want, what):
    assert len(got) == len(want), what
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        pytest.fail("%s: proof bytes differ from the oracle, first at byte %d of %d" % (what, int(np.nonzero(a != b)[0][0]), len(want)))


def _circuits(nlx, ctx, syn, monkeypatch):
    """the circuit with PoseidonGate's partial rounds in k_quotient_poseidon ("0") and inside k_quotient ("1")"""
    out = {}
    for inline in ("0", "1"):
        monkeypatch.setenv("NLX_QUOTIENT_POSEIDON_INLINE", inline)
        out[inline] = nlx.CircuitData.from_synthetic(ctx, syn)
    return out


@pytest.mark.parametrize("log_n,kw", SHAPES)
def test_aimed_witness_proofs_equal_the_oracle(nlx, ctx, orc, monkeypatch, log_n, kw):
    """a witness whose LDE holds the gate rows and the PoseidonGate traces on one class, and witnesses whose every column is a
    constant edge value (so is every LDE value): the oracle proves each, the GPU gives its bytes"""
    rng = np.random.default_rng(700 + log_n)
    syn = nlx.SyntheticCircuit(log_n, seed=700 + log_n, **kw)
    ref = orc.Circuit.from_synthetic(syn)
    r = 1 + log_n % 7
    g, prows = qa.gate_aim_rows(shift=37 * log_n)
    placed = qa.place_rows(g, prows, log_n)
    _, aimed = qa.interpolate(orc, qa.rows_to_targets({k: row for k, (_, row) in placed.items()}, r), 135, log_n, rng)
    witnesses = [("aimed on class %d" % r, aimed)]
    witnesses += [("every column %#x" % v, np.full((135, 1 << log_n), v, dtype=np.uint64)) for v in CONSTANT_EDGES]
    wants = [ref.prove(w, syn.public_inputs) for _, w in witnesses]
    for (name, _), want in zip(witnesses, wants):
        assert len(want) > 0, "the oracle refused the witness %s" % name
    cds = _circuits(nlx, ctx, syn, monkeypatch)
    for inline, cd in cds.items():
        for (name, w), want in zip(witnesses, wants):
            _same(cd.prove(w, syn.public_inputs), want, "%s, NLX_QUOTIENT_POSEIDON_INLINE=%s" % (name, inline))
        cd.close()
    ref.close()


def _permutation_and_gate_rows(syn, log_n, betas, gammas, xs_of, sigma_at, shift, zero_numerators):
    """{k: row}: permutation_rows for challenge 0 at lanes 2, 3 (mod 32), for challenge 1 at lanes 4, 5, the gate rows and
    PoseidonGate traces at every other index"""
    pos = qa.permutation_positions(log_n)
    rows = {}
    for c, lanes in ((0, (2, 3)), (1, (4, 5))):
        xs = {k: xs_of(k) for k in pos if k % 32 in lanes}
        rows.update(qa.permutation_rows(syn.k_is, sigma_at, betas[c], gammas[c], xs, zero_numerators=zero_numerators))
    g, prows = qa.gate_aim_rows(shift=shift)
    for k, (_, row) in qa.place_rows(g, prows, log_n, skip=pos).items():
        rows[k] = row
    return rows


@pytest.mark.parametrize("log_n,kw", SHAPES)
def test_aimed_stages_equal_the_oracle(nlx, ctx, orc, monkeypatch, log_n, kw):
    """partial_products_and_zs on an aimed witness on H, and quotient_eval on aimed from_coeffs wires and Zs under edge
    challenges (alpha at p - 1, 2^32 - 1 and random; beta = p - 1, gamma = 2^32 - 1 for challenge 0; an edge public-inputs hash)
    equal the oracle's stage entries: Zs and chunk coefficients, and the caps"""
    rng = np.random.default_rng(800 + log_n)
    n = 1 << log_n
    syn = nlx.SyntheticCircuit(log_n, seed=800 + log_n, **kw)
    oc = orc.Circuit.from_synthetic(syn)
    cds = _circuits(nlx, ctx, syn, monkeypatch)
    rnd = [int(x) for x in rand_field(rng, 4)]
    betas, gammas = [P - 1, rnd[0]], [qa.EPS, rnd[1]]
    b2, g2 = np.array(betas, dtype=np.uint64), np.array(gammas, dtype=np.uint64)
    nzs = 2 * (1 + syn.config.num_partial_products)

    # ---- Z / partial products: the factors aimed on H (x = w_n^k, sigma_j the circuit's values there) ----
    w_n = qa.root(log_n)
    rows = _permutation_and_gate_rows(syn, log_n, betas, gammas, lambda k: pow(w_n, k, P), lambda j, k: int(syn.sigmas[j, k]),
                                      shift=11 * log_n, zero_numerators=False)
    wh = rand_field(rng, (135, n))
    for k, row in rows.items():
        for c, v in enumerate(row):
            if v is not None:
                wh[c, k] = v
    want_zs = oc.partial_products_and_zs(wh, betas, gammas)
    want = orc.commit(want_zs, 3, 4)
    for inline, cd in cds.items():
        cz = cd.partial_products_and_zs(wh, b2, g2)
        assert np.array_equal(cz.coeffs(), want["coeffs"]), "Zs differ (NLX_QUOTIENT_POSEIDON_INLINE=%s)" % inline
        assert np.array_equal(cz.cap, want["cap"])
        cz.close()

    # ---- quotient: wires and Zs aimed on class r of the LDE ----
    r = 3 + log_n % 5
    sig = [orc.fft(syn.sigmas[j], inverse=True) for j in range(syn.config.num_routed_wires)]
    xs = {k: qa.point(r, k, log_n) for k in range(n)}
    rows = _permutation_and_gate_rows(syn, log_n, betas, gammas, xs.__getitem__, lambda j, k: orc.eval_poly(sig[j], xs[k]),
                                      shift=23 * log_n, zero_numerators=True)
    wc, _ = qa.interpolate(orc, qa.rows_to_targets(rows, r), 135, log_n, rng)
    zc, _ = qa.interpolate(orc, qa.zs_targets(nzs, r, range(n)), nzs, log_n, rng)
    cw = nlx.PolynomialBatch.from_coeffs(ctx, wc, 3, 4)
    cz = nlx.PolynomialBatch.from_coeffs(ctx, zc, 3, 4)
    # the device's LDE holds every aimed row at its point of class r
    leaves = cw.leaves()
    for k, row in rows.items():
        got = leaves[qa.lde_row(r, k, log_n)]
        assert all(v is None or int(got[c]) == v for c, v in enumerate(row)), "aim at class %d, index %d missed" % (r, k)
    pih = np.array(PIH_EDGE, dtype=np.uint64)
    for alphas in ([P - 1, qa.EPS], [rnd[2], P - 1], [qa.EPS, rnd[3]]):
        want_q = oc.quotient_polys(wc, zc, betas, gammas, alphas, pih)
        want_cap = orc.commit(want_q, 3, 4, from_coeffs=True)["cap"]
        for inline, cd in cds.items():
            cq = cd.quotient_eval(cw, cz, b2, g2, np.array(alphas, dtype=np.uint64), pih)
            got = cq.coeffs()
            if not np.array_equal(got, want_q):
                bad = np.argwhere(got != want_q)
                pytest.fail("quotient chunks differ (alphas %s, NLX_QUOTIENT_POSEIDON_INLINE=%s): %d coefficients, first at %s"
                            % ([hex(a) for a in alphas], inline, len(bad), tuple(bad[0])))
            assert np.array_equal(cq.cap, want_cap)
            cq.close()
    for b in (cw, cz, *cds.values()):
        b.close()
    oc.close()
