"""CPU checks of tests/quotient_aims.py (the aimed witnesses of the quotient and Z stages) and of the oracle's stage entries
orc_partial_products_and_zs / orc_quotient_polys, which tests/test_gpu_quotient_aims.py compares the device stages with: the aims
land where they are meant to, and the stage entries are what the whole oracle proof computes.  The last test runs this file again
under the other generator set of include/nlx_field.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

import poseidon_aims as pa
import quotient_aims as qa
from conftest import GEN_SET, P, ROOT

LOG_N = 6
ALL_GATES = dict(pct_poseidon=10, pct_arithmetic=10, pct_base_sum=5, pct_constant=5, pct_extension=10, pct_misc=20, pct_u32=30)


def test_interpolated_polynomials_take_their_targets(orc):
    """each aimed polynomial takes its value at its point (Horner at x), the witness on H is its NTT, and the committed LDE holds
    the value in the leaf row of (class, index) - the map from class r to coset_base[r] = g w_L^r checked against the LDE"""
    rng = np.random.default_rng(1)
    n = 1 << LOG_N
    targets = {}
    for c in range(12):
        for m, k in enumerate((0, 1, 31, 32, 33, 63)):
            targets[(c, c % 8, k)] = qa.EDGES[(c + m) % len(qa.EDGES)]
    coeffs, on_h = qa.interpolate(orc, targets, 14, LOG_N, rng)
    for (c, r, k), v in targets.items():
        assert orc.eval_poly(coeffs[c], qa.point(r, k, LOG_N)) == v % P, (c, r, k)
    w_n = qa.root(LOG_N)
    for c in (0, 7, 13):
        for i in (0, 5, n - 1):
            assert orc.eval_poly(coeffs[c], pow(w_n, i, P)) == int(on_h[c, i])
    com = orc.commit(on_h, 3, 4)
    assert np.array_equal(com["coeffs"], coeffs)
    for (c, r, k), v in targets.items():
        assert int(com["leaves"][qa.lde_row(r, k, LOG_N), c]) == v % P, (c, r, k)
    with pytest.raises(AssertionError):
        qa.interpolate(orc, {(0, 1, 0): 1, (0, 2, 0): 1}, 1, LOG_N, rng)


@pytest.mark.parametrize("log_n", [9, 10])
def test_whole_witness_aims_land_in_the_lde(orc, log_n):
    """the witness of test_aimed_witness_proofs_equal_the_oracle: committed from its values on H, its LDE holds every placed row
    (gate rows and PoseidonGate traces) at its point of the aimed class"""
    rng = np.random.default_rng(5)
    r = 1 + log_n % 7
    g, prows = qa.gate_aim_rows(shift=37 * log_n)
    placed = qa.place_rows(g, prows, log_n)
    assert sorted(placed) == list(range(1 << log_n))
    _, on_h = qa.interpolate(orc, qa.rows_to_targets({k: row for k, (_, row) in placed.items()}, r), 135, log_n, rng)
    leaves = orc.commit(on_h, 3, 4)["leaves"]
    for k, (name, row) in placed.items():
        assert [int(v) for v in leaves[qa.lde_row(r, k, log_n)]] == row, (k, name)


def test_poseidon_gate_rows_reach_their_targets(orc):
    """every PoseidonGate aim row is an honest trace (the oracle's permutation gives its outputs) whose state at the named layer
    is the target: the naive MDS input, the device's held one at a block start, or element 0's S-box input"""
    aims = qa.poseidon_gate_aims()
    assert {a[2][0] for a in aims} == {"held", "mds", "sbox0"}
    assert {a[2][1] for a in aims if a[2][0] == "held"} == set(pa.block_start_layers())
    assert {a[2][1] for a in aims if a[2][0] == "mds"} == {r for r in range(pa.NR) if pa.is_full(r)}
    _, prows = qa.gate_aim_rows()
    assert len(prows) == len(aims)
    for i, ((name, inp, (kind, layer, target)), (rname, row)) in enumerate(zip(aims, prows)):
        assert rname.startswith("poseidon " + name)
        swap = row[24]
        assert swap == i % 2
        st = list(row[0:12])
        if swap:
            st[0:4], st[4:8] = row[4:8], row[0:4]
        assert st == [int(x) % P for x in inp], name
        assert row[25:29] == [swap * (row[j + 4] - row[j]) % P for j in range(4)]
        sbox_in, mds_in, out = pa.trace(st)
        assert row[12:24] == out
        if kind == "mds":
            assert mds_in[layer] == [x % P for x in target], name
        elif kind == "held":
            d = pa.device_offset(layer)
            assert [(x - y) % P for x, y in zip(mds_in[layer], d)] == [x % P for x in target], name
        else:
            assert sbox_in[layer][0] == target % P, name
        for rnd in (1, 2, 3):
            assert row[29 + 12 * (rnd - 1): 41 + 12 * (rnd - 1)] == sbox_in[rnd]
        assert row[65:87] == [sbox_in[4 + j][0] for j in range(22)]
        for rnd in range(4):
            assert row[87 + 12 * rnd: 99 + 12 * rnd] == sbox_in[26 + rnd]
        if i < 16:
            assert [int(x) for x in orc.poseidon_permute(st)[0]] == out


def test_gate_rows_cover_the_limb_extremes():
    rows = dict(qa.gate_rows())
    assert all(len(r) == qa.NUM_WIRES and all(0 <= v < P for v in r) for r in rows.values())
    for v in (0, 1, 2, qa.EPS, qa.EPS + 1, P - 1):
        assert rows["fill %#x" % v] == [v] * qa.NUM_WIRES
    # every wire at each of 0 / 2^32 - 1 / 2^32 under the three rotations of that cycle
    cyc = [r for name, r in rows.items() if name.startswith(("cycle 0x0/", "cycle 0xffffffff/0x100000000/",
                                                              "cycle 0x100000000/0x0/"))]
    assert len(cyc) == 3
    for c in range(qa.NUM_WIRES):
        assert {r[c] for r in cyc} == {0, qa.EPS, qa.EPS + 1}


def test_placement_puts_every_gate_row_somewhere_and_at_the_lane_classes():
    g, prows = qa.gate_aim_rows()
    for log_n in (9, 10):
        skip = qa.permutation_positions(log_n)
        placed = qa.place_rows(g, prows, log_n, skip=skip)
        assert sorted(list(placed) + skip) == list(range(1 << log_n))
        names = [nm for nm, _ in placed.values()]
        assert {nm for nm, _ in g} <= set(names)
        lane_rows = {placed[k][0] for k in placed if k % 64 in pa.LANE_CLASSES}
        assert lane_rows <= {nm for nm, _ in g}
        n_pos = sum(nm.startswith("poseidon ") for nm in set(names))
        assert n_pos == min(len(prows), len(placed) - max(len(g), 6 * ((1 << log_n) // 64)))


@pytest.mark.parametrize("on_h", [True, False])
def test_permutation_rows_hit_their_factors(nlx, orc, on_h):
    """w + beta k_i x + gamma (even positions) and w + beta sigma_i(x) + gamma (odd positions) take FACTOR_TARGETS values, no
    denominator is 0, and without zero_numerators no numerator either; on H and on an LDE class"""
    syn = nlx.SyntheticCircuit(LOG_N, seed=7)
    beta, gamma = P - 1, qa.EPS
    ks = [0, 1, 2, 3, 31, 32, 33, 34, 62, 63]
    if on_h:
        xs = {k: pow(qa.root(LOG_N), k, P) for k in ks}
        sigma = lambda j, k: int(syn.sigmas[j, k])  # noqa: E731
    else:
        sig = [orc.fft(syn.sigmas[j], inverse=True) for j in range(80)]
        xs = {k: qa.point(5, k, LOG_N) for k in ks}
        sigma = lambda j, k: orc.eval_poly(sig[j], xs[k])  # noqa: E731
    for zero_numerators in (True, False):
        rows = qa.permutation_rows(syn.k_is, sigma, beta, gamma, xs, zero_numerators=zero_numerators)
        seen = set()
        for m, k in enumerate(ks):
            for j in range(80):
                w = rows[k][j]
                num = (w + beta * int(syn.k_is[j]) * xs[k] + gamma) % P
                den = (w + beta * sigma(j, k) + gamma) % P
                assert den != 0
                if m % 2 == 0:
                    assert num in qa.FACTOR_TARGETS and (num or zero_numerators)
                    seen.add(num)
                else:
                    assert den in qa.FACTOR_TARGETS or den == 3
                    seen.add(den)
            assert rows[k][80:] == [None] * (qa.NUM_WIRES - 80)
        assert set(qa.FACTOR_TARGETS) - {0} <= seen and (0 in seen) == zero_numerators


@pytest.mark.parametrize("log_n,kw", [(6, ALL_GATES), (5, dict(pct_poseidon=40, pct_arithmetic=20, pct_base_sum=5, pct_constant=5))])
def test_stage_entries_equal_the_traced_proof(nlx, orc, log_n, kw):
    """orc_partial_products_and_zs and orc_quotient_polys, under the transcript's own challenges, give what orc_prove_traced
    dumps, and the proof is the untraced one"""
    syn = nlx.SyntheticCircuit(log_n, seed=40 + log_n, **kw)
    oc = orc.Circuit.from_synthetic(syn)
    proof, info = oc.prove(syn.wires, syn.public_inputs, trace=True)
    assert proof == oc.prove(syn.wires, syn.public_inputs) and oc.verify(proof) == 1
    zs = oc.partial_products_and_zs(syn.wires, info["betas"], info["gammas"])
    assert np.array_equal(zs, info["zs_partial_values"])
    wc = np.stack([orc.fft(w, inverse=True) for w in syn.wires])
    zc = np.stack([orc.fft(z, inverse=True) for z in zs])
    pih = orc.hash_no_pad(syn.public_inputs)
    q = oc.quotient_polys(wc, zc, info["betas"], info["gammas"], info["alphas"], pih)
    assert np.array_equal(q, info["quotient_chunk_coeffs"])
    oc.close()


def test_aimed_witness_is_proved_by_the_oracle(nlx, orc):
    """an aimed witness is not refused: the oracle proves it (the proof does not verify: the witness satisfies nothing), and the
    stage entries run on it, on aimed Zs and under edge challenges, without inverting a zero"""
    rng = np.random.default_rng(9)
    syn = nlx.SyntheticCircuit(LOG_N, seed=11, **ALL_GATES)
    oc = orc.Circuit.from_synthetic(syn)
    g, prows = qa.gate_aim_rows()
    placed = qa.place_rows(g, prows, LOG_N)
    wc, wh = qa.interpolate(orc, qa.rows_to_targets({k: row for k, (_, row) in placed.items()}, 2), 135, LOG_N, rng)
    proof = oc.prove(wh, syn.public_inputs)
    assert len(proof) > 0 and oc.verify(proof) < 1
    zs = oc.partial_products_and_zs(wh, [P - 1, 5], [qa.EPS, 7])
    assert zs.shape == (20, 1 << LOG_N) and (zs < np.uint64(P)).all()
    zc, _ = qa.interpolate(orc, qa.zs_targets(20, 2, range(1 << LOG_N)), 20, LOG_N, rng)
    q = oc.quotient_polys(wc, zc, [P - 1, 5], [qa.EPS, 7], [P - 1, qa.EPS], [P - 1, 0, qa.EPS, 1])
    assert q.shape == (16, 1 << LOG_N) and (q < np.uint64(P)).all()
    oc.close()


def test_other_generator_set():
    """every test above again, in a fresh interpreter, under the other generator set (conftest and the oracle read
    NLX_GL_GENERATOR_SET at import)"""
    other = "2021" if GEN_SET == "7" else "7"
    env = dict(os.environ, NLX_GL_GENERATOR_SET=other)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu", os.path.abspath(__file__),
                        "-k", "not other_generator_set"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
