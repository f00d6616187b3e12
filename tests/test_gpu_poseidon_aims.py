"""GPU: the Poseidon kernels on aimed states (tests/poseidon_aims.py) - inputs whose state at a chosen layer is a worst case of
that layer's byte planes, folds, fused-block S-box inputs or BN128 MDS rows.

Random states and edge inputs never bring such a case past the first round.  Every aimed state sits at lanes 0, 1, 31, 32, 33
and 63 of some wave (the matrix cores treat lanes n and n + 32 differently) and as the last item of a batch (whose lane the
spare lanes of the last wave copy); the rest of a batch is random.  Results are compared with the C oracle and the Python
models.  The leaf-hashing kernels (row-major leaves, k_hash_lde_leaves) only see what a row puts into the rate slots of the
first layer: rows are aimed there."""
import os
import re

import numpy as np
import pytest

from conftest import P, ROOT, rand_field
import poseidon_aims as pa

pytestmark = pytest.mark.gpu

gpb = pa.gpb


def _gl_expected():
    return [gpb.naive(st) for _, st, _ in pa.gl_aims()]


def test_permute_aimed_states(nlx, ctx, orc):
    aims = pa.gl_aims()
    want = _gl_expected()
    rng = np.random.default_rng(2026)
    n, where = pa.placement(len(aims))
    st = rand_field(rng, (n, 12))
    for pos, i in where.items():
        st[pos] = aims[i][1]
    got = nlx.poseidon_permute(ctx, st)
    assert np.array_equal(got, orc.poseidon_permute(st))
    assert (got < np.uint64(P)).all()
    for pos, i in where.items():
        assert got[pos].tolist() == want[i], (pos, aims[i][0])
    # every aimed state as the last item of a short batch (lengths 1 .. 64: the last item in every lane, spare lanes copying it)
    for i, (name, s, _) in enumerate(aims):
        k = 1 + i % 64
        b = np.array([aims[(i + j) % len(aims)][1] for j in range(k - 1, -1, -1)], dtype=np.uint64)
        out = nlx.poseidon_permute(ctx, b)
        assert out[-1].tolist() == want[i], name
        assert out.tolist() == [want[(i + j) % len(aims)] for j in range(k - 1, -1, -1)], name


def _gl_rows(row_len):
    return [(name, pa.gl_rate_row(z[:8], row_len)) for name, z in pa.gl_patterns()]


@pytest.mark.parametrize("row_len", [8, 9, 16, 135])
def test_hash_rows_aimed_first_layer(nlx, ctx, orc, row_len):
    """k_hash_leaves_rowmajor: every absorb's first layer holds a pattern in its eight rate slots"""
    rows_aimed = _gl_rows(row_len)
    rng = np.random.default_rng(row_len)
    n, where = pa.placement(len(rows_aimed))
    rows = rand_field(rng, (n, row_len))
    for pos, i in where.items():
        rows[pos] = rows_aimed[i][1]
    got = nlx.hash_rows(ctx, rows)
    want = np.array([orc.hash_or_noop(r) for r in rows])
    assert np.array_equal(got, want), row_len
    for pos, i in where.items():
        assert got[pos].tolist() == want[pos].tolist(), rows_aimed[i][0]


@pytest.mark.parametrize("leaf_len,cap_h", [(135, 4), (9, 0)])
def test_merkle_tree_aimed_leaves(nlx, ctx, orc, leaf_len, cap_h):
    rows_aimed = _gl_rows(leaf_len)
    rng = np.random.default_rng(leaf_len)
    n, where = pa.placement(len(rows_aimed), n=2048)
    leaves = rand_field(rng, (n, leaf_len))
    for pos, i in where.items():
        leaves[pos] = rows_aimed[i][1]
    t = nlx.MerkleTree(ctx, leaves, cap_h)
    dig, cap = orc.merkle_build(leaves, cap_h)
    assert np.array_equal(t.digests, dig)
    assert np.array_equal(t.cap, cap)


def _wide_kernel_max_rows():
    """launch_hash_lde_leaves sends a table of more than 16 columns and at most this many rows to k_hash_lde_leaves_wide"""
    with open(os.path.join(ROOT, "near-light-client_amd", "csrc", "hash_kernels.hip")) as f:
        m = re.search(r"HASH_LEAVES_WIDE_MAX_ROWS = \(size_t\)1 << (\d+);", f.read())
    assert m, "HASH_LEAVES_WIDE_MAX_ROWS moved: this test must still pick the kernel it names"
    return 1 << int(m.group(1))


@pytest.mark.parametrize("n_cols", [135, 20])
def test_commit_constant_columns_aimed(nlx, ctx, orc, n_cols):
    """k_hash_lde_leaves (one state per lane): PolynomialBatch.from_values with constant columns, whose LDE is that constant on
    every row, so the leaf kernel hashes the aimed row at every one of the 2^14 points - above the row count up to which wide
    tables go to the wide kernel.  Every leaf digest is the oracle's hash of the row; each Merkle level above is compress(d, d)
    of the level below."""
    log_n, rate_bits, cap_h = 11, 3, 4
    L = 1 << (log_n + rate_bits)
    assert L > _wide_kernel_max_rows()
    for name, row in _gl_rows(n_cols):
        col = np.array(row, dtype=np.uint64)
        vals = np.repeat(col[:, None], 1 << log_n, axis=1)
        pb = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h)
        coeffs = np.zeros_like(vals)
        coeffs[:, 0] = col
        assert np.array_equal(pb.coeffs(), coeffs), name
        d = orc.hash_or_noop(col)
        dig = pb.digests().reshape(-1, 4)
        off, lvl = 0, L
        while True:
            assert (dig[off:off + lvl] == d).all(), (name, lvl)
            off += lvl
            if lvl <= 1 << cap_h:
                break
            d = orc.merkle_build(np.tile(d, (2, 1)), 0)[1][0]   # a 4-element leaf is its own digest: one compress(d, d)
            lvl >>= 1
        assert off == len(dig)
        assert (pb.cap == d).all(), name


@pytest.mark.parametrize("n_cols", [135, 20])
def test_commit_constant_columns_aimed_wide_kernel(nlx, ctx, orc, n_cols):
    """the same aimed rows through k_hash_lde_leaves_wide (128 rows: one element per lane, the linear layer through LDS), against
    the oracle's whole commitment"""
    log_n, rate_bits, cap_h = 4, 3, 2
    assert (1 << (log_n + rate_bits)) <= _wide_kernel_max_rows()
    for name, row in _gl_rows(n_cols):
        vals = np.repeat(np.array(row, dtype=np.uint64)[:, None], 1 << log_n, axis=1)
        pb = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h)
        ref = orc.commit(vals, rate_bits, cap_h)
        assert np.array_equal(ref["leaves"][5], np.array(row, dtype=np.uint64)), name
        assert np.array_equal(pb.cap, ref["cap"]), name
        assert np.array_equal(pb.coeffs(), ref["coeffs"]), name
        assert np.array_equal(pb.digests(), ref["digests"]), name


def test_bn128_permute_aimed_states(nlx, ctx):
    aims = pa.bn_aims()
    want = [pa.pbn.permute(st) for _, st, _ in aims]
    rng = np.random.default_rng(254)
    n, where = pa.placement(len(aims))
    fill = rng.integers(0, len(aims), size=n)             # the rest: other aimed states, in random order (their results are known)
    idx = [where.get(pos, int(fill[pos])) for pos in range(n)]
    got = nlx.poseidon_bn128_permute(ctx, [aims[i][1] for i in idx])
    for pos, i in enumerate(idx):
        assert got[pos] == want[i], (pos, aims[i][0])
    for i, (name, s, _) in enumerate(aims):
        k = 1 + i % 64
        b = [(i + j) % len(aims) for j in range(k - 1, -1, -1)]
        out = nlx.poseidon_bn128_permute(ctx, [aims[j][1] for j in b])
        assert out == [want[j] for j in b], name
