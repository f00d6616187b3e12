"""GPU tests of PoseidonBN128 (csrc/poseidon_bn128.hip): permutation, hash_or_noop rows, Merkle trees and BN128 commitments
against the Python reference model (tools/gen_poseidon_bn128.py).  The model costs ~1-2 ms per permutation, so full-tree checks
stay below ~20 k permutations and the large commitment is checked through sampled openings."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT, rand_field

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_bn128 as m  # noqa: E402

pytestmark = pytest.mark.gpu

R = m.R
NLX_E_RANGE, NLX_E_UNSUPPORTED = -4, -5
BN = "poseidon_bn128"


def _ints(words):
    """(n, 4) uint64 little-endian words -> Python ints"""
    return [m.from_words(w) for w in np.asarray(words)]


def test_permute_ragged_counts(nlx, ctx):
    rng = random.Random(11)
    edges = [0, 1, R - 1, (1 << 192) - 1]
    for n in (1, 63, 65, 1000, (1 << 16) + 3):
        states = [[rng.randrange(R) for _ in range(4)] for _ in range(n)]
        for k in range(min(n, 40)):
            states[k] = [rng.choice(edges) for _ in range(4)]
        got = nlx.poseidon_bn128_permute(ctx, states)
        check = range(n) if n <= 1000 else sorted(set(rng.sample(range(n), 200)) | {0, 1, n - 2, n - 1})
        for i in check:
            assert got[i] == m.permute(states[i]), (n, i)
    # the array form, and a non-canonical element is refused with nothing written
    arr = nlx.bn254_pack([[3, 1, 4, 1], [5, 9, 2, 6]])
    out = nlx.poseidon_bn128_permute(ctx, arr)
    assert _ints(out[0]) == m.permute([3, 1, 4, 1]) and _ints(out[1]) == m.permute([5, 9, 2, 6])
    bad = nlx.bn254_pack([[0, 0, 0, 0], [0, R, 0, 0]])
    with pytest.raises(nlx.NlxError) as e:
        nlx.poseidon_bn128_permute(ctx, bad)
    assert e.value.code == NLX_E_RANGE


def test_hash_rows_lengths(nlx, ctx):
    rng = np.random.default_rng(12)
    for row_len in (1, 2, 3, 4, 5, 9, 10, 18, 19, 135):
        n = 70 if row_len < 100 else 66
        rows = rand_field(rng, (n, row_len))
        rows[0] = 0xFFFFFFFF00000000                                               # p - 1 everywhere
        rows[1] = (rows[1] & np.uint64(0xFFFFFFFF)) + np.uint64(0xFFFFFFFF00000001)   # values >= p: taken mod p
        if row_len == 4:
            rows[:, 3] %= np.uint64(R >> 192)   # a 4-element row is its own digest and must pack below r
        got = nlx.poseidon_bn128_hash_rows(ctx, rows, as_ints=True)
        for i in range(n):
            assert got[i] == m.hash_or_noop([int(v) for v in rows[i]]), (row_len, i)
    with pytest.raises(nlx.NlxError) as e:
        nlx.poseidon_bn128_hash_rows(ctx, np.array([[0, 0, 0, (R >> 192) + 1]], dtype=np.uint64))
    assert e.value.code == NLX_E_RANGE


def _check_levels(digests, levels):
    off = 0
    for lv in levels:
        assert _ints(digests[off:off + 4 * len(lv)].reshape(-1, 4)) == lv
        off += 4 * len(lv)
    assert off == digests.size


def test_merkle_build_full_tree(nlx, ctx):
    rng = np.random.default_rng(13)
    leaves = rand_field(rng, (1 << 10, 7))
    levels = m.merkle_digests([[int(v) for v in row] for row in leaves], 0)
    for cap_height in (0, 4):
        t = nlx.MerkleTree(ctx, leaves, cap_height, hasher=BN)
        want = levels[:len(levels) - cap_height]
        _check_levels(t.digests, want)
        assert _ints(t.cap) == want[-1]
        for idx in (0, 5, 1023):   # MerkleTree.prove on the BN128 digests walks to the cap
            path = [m.from_words(w) for w in t.prove(idx)]
            ci, h = m.merkle_root_from_path(levels[0][idx], idx, path)
            assert h == want[-1][ci]


@pytest.mark.parametrize("rate_bits", [1, 2, 3])
def test_commitment_small_equals_model(nlx, ctx, rate_bits):
    rng = np.random.default_rng(20 + rate_bits)
    vals = rand_field(rng, (20, 1 << 8))
    cap_height = 2
    gold = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_height)
    bn = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_height, hasher=BN)
    assert gold.hasher == "poseidon_goldilocks" and bn.hasher == BN
    leaves = bn.leaves()
    assert np.array_equal(leaves, gold.leaves())
    assert np.array_equal(bn.coeffs(), gold.coeffs())
    assert np.array_equal(bn.eval_at([3, 7]), gold.eval_at([3, 7]))
    levels = m.merkle_digests([[int(v) for v in row] for row in leaves], cap_height)
    _check_levels(bn.digests(), levels)
    assert _ints(bn.cap) == levels[-1]
    rows, paths = bn.open_rows(np.array([0, 77, bn.lde_size - 1], dtype=np.uint64))
    for j, idx in enumerate((0, 77, bn.lde_size - 1)):
        assert np.array_equal(rows[j], leaves[idx])
        ci, h = m.merkle_root_from_path(levels[0][idx], idx, [m.from_words(w) for w in paths[j]])
        assert h == levels[-1][ci]
    # from_coeffs: the same pipeline from coefficients (full tree at rate 1, the leaf level and cap otherwise)
    cb = nlx.PolynomialBatch.from_coeffs(ctx, gold.coeffs(), rate_bits, cap_height, hasher=BN)
    assert np.array_equal(cb.leaves(), leaves) and np.array_equal(cb.cap, bn.cap) and np.array_equal(cb.digests(), bn.digests())
    coeffs = rand_field(rng, (20, 1 << 8))
    gc = nlx.PolynomialBatch.from_coeffs(ctx, coeffs, rate_bits, cap_height)
    cc = nlx.PolynomialBatch.from_coeffs(ctx, coeffs, rate_bits, cap_height, hasher=BN)
    assert np.array_equal(cc.leaves(), gc.leaves())
    if rate_bits == 1:
        lv = m.merkle_digests([[int(v) for v in row] for row in cc.leaves()], cap_height)
        _check_levels(cc.digests(), lv)
    for c in (gold, bn, cb, gc, cc):
        c.close()


def test_commitment_large_sampled_paths(nlx, ctx):
    rng = np.random.default_rng(31)
    log_n, rate_bits, cap_height, n_cols = 16, 3, 4, 135
    vals = rand_field(rng, (n_cols, 1 << log_n))
    ctx.kernel_timing(True)
    bn = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_height, hasher=BN)
    L = bn.lde_size
    assert ctx.kernel_units("hash_lde_leaves_bn128") == L * ((n_cols + 8) // 9)
    assert ctx.kernel_units("merkle_levels_bn128") == L - (1 << cap_height)
    assert ctx.kernel_units("hash_lde_leaves") == 0   # the Goldilocks leaf kernel did not run
    ctx.kernel_timing(False)
    gold = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_height)
    idx = np.array(sorted(random.Random(32).sample(range(L), 62)) + [0, L - 1], dtype=np.uint64)
    rows, paths = bn.open_rows(idx)
    grows, _ = gold.open_rows(idx, with_paths=False)
    assert np.array_equal(rows, grows)
    cap = _ints(bn.cap)
    assert paths.shape == (64, log_n + rate_bits - cap_height, 4)
    for j, i in enumerate(idx):
        ci, h = m.merkle_root_from_path(m.hash_or_noop([int(v) for v in rows[j]]), int(i), [m.from_words(w) for w in paths[j]])
        assert h == cap[ci], int(i)
    bn.close()
    gold.close()


def test_goldilocks_refuses_nothing_and_bad_inputs_are_refused(nlx, ctx):
    dll = nlx.lib.dll
    rng = np.random.default_rng(40)
    vals = rand_field(rng, (8, 1 << 6))
    h = ctypes.c_void_p()
    cap = np.zeros((1, 4), dtype=np.uint64)
    assert dll.nlx_commit_from_values_hasher(ctx.handle, vals.ctypes.data, 8, 6, 1, 0, 7, cap.ctypes.data, ctypes.byref(h)) == NLX_E_RANGE
    # hasher 0 through the new entry is today's commitment
    assert dll.nlx_commit_from_values_hasher(ctx.handle, vals.ctypes.data, 8, 6, 1, 0, 0, cap.ctypes.data, ctypes.byref(h)) == 0
    assert dll.nlx_commit_hasher(h) == 0
    gold = nlx.PolynomialBatch.from_values(ctx, vals, 1, 0)
    assert np.array_equal(cap, gold.cap)
    dll.nlx_commit_destroy(h)
    # four columns: a leaf is its own digest, and a random LDE row packs to a value >= r somewhere (P(all below r) ~ 0.19^128)
    four = rand_field(rng, (4, 1 << 6))
    with pytest.raises(nlx.NlxError) as e:
        nlx.PolynomialBatch.from_values(ctx, four, 1, 0, hasher=BN)
    assert e.value.code == NLX_E_RANGE
    with pytest.raises(ValueError):
        nlx.PolynomialBatch.from_values(ctx, vals, 1, 0, hasher="sha256")


def test_transcript_entries_refuse_bn128(nlx, ctx):
    pk = nlx.plonk
    syn = nlx.SyntheticCircuit(7, seed=5)
    cd = nlx.CircuitData.from_synthetic(ctx, syn)
    cfg = syn.config
    cw = nlx.PolynomialBatch.from_values(ctx, syn.wires, cfg.rate_bits, cfg.cap_height, hasher=BN)
    z = np.zeros(2, np.uint64)
    b, g = np.array([7, 11], np.uint64), np.array([13, 17], np.uint64)
    cz = cd.partial_products_and_zs(syn.wires, b, g)
    with pytest.raises(nlx.NlxError) as e:
        cd.quotient_eval(cw, cz, b, g, z, np.zeros(4, np.uint64))
    assert e.value.code == NLX_E_UNSUPPORTED
    fp = pk.FriParams(cfg.fri_arity_bits, cfg.fri_final_poly_bits, cfg.fri_pow_bits, cfg.fri_num_queries)
    n_w = syn.wires.shape[0]
    with pytest.raises(nlx.NlxError) as e:
        pk.fri_prove(ctx, [cw], [0], z, np.zeros((n_w, 2), np.uint64), np.zeros((0, 2), np.uint64), fp, pk.Challenger())
    assert e.value.code == NLX_E_UNSUPPORTED
    cw.close()
    cz.close()
    cd.close()
