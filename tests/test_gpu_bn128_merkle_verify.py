"""GPU: nlx_poseidon_bn128_merkle_verify_batch - plonky2's verify_merkle_proof_to_cap under PoseidonBN128 on a quad of lanes, the
device code of the proof verifier's path kernel (csrc/poseidon_bn128_path.hpp) - at its smallest failing shapes.  The reference
for every byte is the pure Python model (tools/gen_poseidon_bn128.py: hash_or_noop, merkle_root_from_path); the trees the honest
paths come from are built by nlx.MerkleTree, which is not under test here (tests/test_gpu_poseidon_bn128.py pins it to the same
model).  Model cost: ceil(leaf_len / 9) + path_len permutations a triple, a few hundred a test."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, P, rand_field

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_bn128 as m  # noqa: E402

pytestmark = pytest.mark.gpu

BN = "poseidon_bn128"
R = m.R
NLX_E_RANGE = -4


def _model(leaves, indices, siblings, cap):
    """the model's answer for every triple"""
    cap = [m.from_words(w) for w in np.asarray(cap).reshape(-1, 4)]
    out = []
    for leaf, idx, path in zip(leaves, indices, siblings):
        ci, h = m.merkle_root_from_path(m.hash_or_noop([int(v) for v in leaf]), int(idx), [m.from_words(s) for s in path])
        out.append(ci < len(cap) and h == cap[ci])
    return np.array(out, dtype=bool)


def _check(nlx, ctx, leaves, indices, siblings, cap, want_any_false=None):
    leaves = np.ascontiguousarray(leaves, dtype=np.uint64)
    siblings = np.ascontiguousarray(siblings, dtype=np.uint64)
    siblings = siblings.reshape(len(leaves), -1, 4) if siblings.size else np.zeros((len(leaves), 0, 4), np.uint64)
    got = nlx.poseidon_bn128_merkle_verify(ctx, leaves, indices, siblings, cap)
    want = _model(leaves, indices, siblings, cap)
    assert got.dtype == bool and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (got.astype(int).tolist(), want.astype(int).tolist())
    if want_any_false is not None:
        assert bool((~want).any()) == want_any_false
    return want


def _tree(nlx, ctx, rng, leaf_len, path_len, cap_height):
    leaves = rand_field(rng, (1 << (path_len + cap_height), leaf_len))
    if leaf_len == 4:
        leaves[:, 3] %= np.uint64(R >> 192)   # a four-word leaf is its own digest and must pack to a value below r
    return nlx.MerkleTree(ctx, leaves, cap_height, hasher=BN)


def _triples(tree, indices):
    idx = np.array(indices, dtype=np.uint64)
    leaves = tree.leaves[idx.astype(np.int64)].copy()
    path_len = (tree.n_leaves >> tree.cap_height).bit_length() - 1
    sib = np.zeros((len(idx), path_len, 4), dtype=np.uint64)
    for j, i in enumerate(idx):
        sib[j] = tree.prove(int(i))
    return leaves, idx, sib


def _tampered(tree, rng, path_len, cap_height):
    """honest triples of a few leaves, then one tamper a triple: a flipped leaf word, a flipped sibling at every level, an index
    with one flipped bit (every bit), and - in a cap copy returned as the second value - a wrong cap entry"""
    n_leaves = tree.n_leaves
    picks = sorted({0, n_leaves - 1, int(rng.integers(0, n_leaves))})
    rows = [(i, "honest") for i in picks]
    i0 = picks[-1]
    rows.append((i0, "leaf"))
    rows += [(i0, ("sibling", k)) for k in range(path_len)]
    rows += [(i0, ("index", b)) for b in range(path_len + cap_height)]
    leaves, idx, sib = _triples(tree, [i for i, _ in rows])
    for j, (_, what) in enumerate(rows):
        if what == "leaf":
            c = int(rng.integers(0, leaves.shape[1]))
            leaves[j, c] = (int(leaves[j, c]) + 1) % P
        elif what != "honest" and what[0] == "sibling":
            sib[j, what[1], int(rng.integers(0, 3))] ^= np.uint64(1 << int(rng.integers(0, 60)))
        elif what != "honest":
            idx[j] ^= np.uint64(1 << what[1])
    return leaves, idx, sib, len(picks)


@pytest.mark.parametrize("leaf_len", list(range(5, 20)) + [27, 135])
def test_every_chunk_remainder(nlx, ctx, leaf_len):
    """leaf lengths 5 .. 19: every remainder 1 .. 9 of the last chunk with one chunk and with two; 27: three whole chunks; 135:
    the wires row of a proof.  Four leaves under one root."""
    rng = np.random.default_rng(1000 + leaf_len)
    tree = _tree(nlx, ctx, rng, leaf_len, 2, 0)
    leaves, idx, sib, n_honest = _tampered(tree, rng, 2, 0)
    want = _check(nlx, ctx, leaves, idx, sib, tree.cap, want_any_false=True)
    assert want[:n_honest].all() and not want[n_honest:].any()
    # the last word of the row alone: a word of the short last chunk
    leaves, idx, sib = _triples(tree, [1, 2])
    leaves[1, leaf_len - 1] ^= np.uint64(1)
    assert _check(nlx, ctx, leaves, idx, sib, tree.cap).tolist() == [True, False]


@pytest.mark.parametrize("cap_height", [0, 2])
@pytest.mark.parametrize("path_len", [0, 1, 2, 5])
def test_path_lengths_and_caps(nlx, ctx, path_len, cap_height):
    rng = np.random.default_rng(77 + 10 * path_len + cap_height)
    tree = _tree(nlx, ctx, rng, 7, path_len, cap_height)
    leaves, idx, sib, n_honest = _tampered(tree, rng, path_len, cap_height)
    want = _check(nlx, ctx, leaves, idx, sib, tree.cap)
    assert want[:n_honest].all() and not want[n_honest:].any()
    # a wrong cap entry: the honest triples under it fail, the others hold
    cap = tree.cap.copy()
    entry = int(idx[0]) >> path_len
    cap[entry, 1] ^= np.uint64(4)
    want = _check(nlx, ctx, leaves[:n_honest], idx[:n_honest], sib[:n_honest], cap, want_any_false=True)
    assert [bool(w) for w in want] == [(int(i) >> path_len) != entry for i in idx[:n_honest]]


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_item_counts_around_one_block(nlx, ctx, n):
    """16 quads make a block: one item, one quad short of a block, a whole block, and one quad into a second block - every third
    triple with a flipped leaf word, so that a quad answering for its neighbour shows"""
    rng = np.random.default_rng(500 + n)
    tree = _tree(nlx, ctx, rng, 10, 1, 0)
    leaves, idx, sib = _triples(tree, [int(i) for i in rng.integers(0, 2, n)])
    for j in range(0, n, 3):
        leaves[j, j % 10] ^= np.uint64(2)
    want = _check(nlx, ctx, leaves, idx, sib, tree.cap)
    assert [bool(w) for w in want] == [j % 3 != 0 for j in range(n)]


def test_short_leaves_are_their_own_digest(nlx, ctx):
    """leaf_len <= 4: hash_or_noop's no-op branch, with nlx_poseidon_bn128_hash_rows' range rule"""
    rng = np.random.default_rng(4)
    for leaf_len in (1, 3, 4):
        tree = _tree(nlx, ctx, rng, leaf_len, 2, 0)
        leaves, idx, sib, n_honest = _tampered(tree, rng, 2, 0)
        want = _check(nlx, ctx, leaves, idx, sib, tree.cap)
        assert want[:n_honest].all() and not want[n_honest:].any()
    # path_len = 0: the packed leaf is the cap entry itself
    leaf = np.array([[5, 6, 7, 8]], dtype=np.uint64)
    cap = leaf.copy()
    assert _check(nlx, ctx, leaf, [0], np.zeros((1, 0, 4), np.uint64), cap).tolist() == [True]
    top = np.array([[0, 0, 0, (R >> 192) + 1]], dtype=np.uint64)     # packs to a value >= r: no digest
    with pytest.raises(nlx.NlxError) as e:
        nlx.poseidon_bn128_merkle_verify(ctx, top, [0], np.zeros((1, 0, 4), np.uint64), cap)
    assert e.value.code == NLX_E_RANGE


def test_digest_words_are_not_field_words(nlx, ctx):
    """a sibling one of whose words is >= p while the digest is below r is a valid digest: taken as input, and the answer is the
    model's; a sibling (or a cap entry) >= r, or an index past the tree, is NLX_E_RANGE"""
    rng = np.random.default_rng(9)
    leaf = rand_field(rng, (1, 12))
    for word in (0, 2):
        sib = np.zeros((1, 1, 4), dtype=np.uint64)
        sib[0, 0, word] = np.uint64(2 ** 64 - 1)
        sib[0, 0, 3] = np.uint64(12345)
        assert int(sib[0, 0, word]) >= P and m.from_words(sib[0, 0]) < R
        h = m.hash_or_noop([int(v) for v in leaf[0]])
        for index in (0, 1):
            root = m.two_to_one(m.from_words(sib[0, 0]), h) if index else m.two_to_one(h, m.from_words(sib[0, 0]))
            cap = np.array([m.to_words(root)], dtype=np.uint64)
            assert _check(nlx, ctx, leaf, [index], sib, cap).tolist() == [True]
            assert _check(nlx, ctx, leaf, [index ^ 1], sib, cap).tolist() == [False]
    cap = np.array([m.to_words(R - 1)], dtype=np.uint64)
    for bad in (R, R + 5, 2 ** 256 - 1):
        sib = np.array([[m.to_words(bad)]], dtype=np.uint64)
        with pytest.raises(nlx.NlxError) as e:
            nlx.poseidon_bn128_merkle_verify(ctx, leaf, [0], sib, cap)
        assert e.value.code == NLX_E_RANGE, hex(bad)
    ok_sib = np.array([[m.to_words(R - 1)]], dtype=np.uint64)
    assert _check(nlx, ctx, leaf, [1], ok_sib, cap).tolist() == [False]      # r - 1 is a digest
    with pytest.raises(nlx.NlxError) as e:
        nlx.poseidon_bn128_merkle_verify(ctx, leaf, [0], ok_sib, np.array([m.to_words(R)], dtype=np.uint64))
    assert e.value.code == NLX_E_RANGE
    with pytest.raises(nlx.NlxError) as e:
        nlx.poseidon_bn128_merkle_verify(ctx, leaf, [2], ok_sib, cap)
    assert e.value.code == NLX_E_RANGE
    assert nlx.poseidon_bn128_merkle_verify(ctx, np.zeros((0, 12), np.uint64), [], np.zeros((0, 1, 4), np.uint64), cap).size == 0
