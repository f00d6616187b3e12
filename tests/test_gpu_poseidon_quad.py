"""GPU: the sub-wave Poseidon (hash_kernels.hip, pquad::permute: one state per quad of lanes, three elements per lane, DPP quad
rotations) through the three kernels built on it - k_merkle_fused (tree tops), k_hash_lde_leaves_wide (leaves of short wide
tables) and k_fri_leaves_wide<2,3,4> (FRI layers) - reached through the C ABI and compared with the CPU oracle word for word.

Shapes are the smallest at which each kernel takes another path: fewer levels than one fused launch holds, exactly as many, one
more, and two chained launches; caps at the leaf level (nothing launched); one tree and several (blockIdx.y, tree_words); leaf
rows with every ragged last chunk; launches whose last wave holds spare quads (fewer than sixteen items)."""
import numpy as np
import pytest

from conftest import P, rand_field

pytestmark = pytest.mark.gpu


# ---- tree tops: k_merkle_fused --------------------------------------------------------------------------------------------------

# 2^1 .. 2^12 leaves down to caps of 2^0, 2^1 and 2^4 digests: 0 levels (the cap IS the leaf level: nothing launched), 1 .. 5 in one
# launch, 6 (a full one), 6 + 1 (a second launch of one level) and 6 + 6 / 6 + 5 / 6 + 2 (two chained); a tree of two leaves has no cap 2^4
@pytest.mark.parametrize("log_leaves,cap_h", [(1, 0), (1, 1), (5, 0), (5, 1), (5, 4), (6, 0), (6, 1), (6, 4), (7, 0), (7, 1), (7, 4),
                                              (12, 0), (12, 1), (12, 4)])
def test_tree_tops_every_level(nlx, ctx, orc, log_leaves, cap_h):
    n = 1 << log_leaves
    rng = np.random.default_rng(1000 * log_leaves + cap_h)
    leaves = rand_field(rng, (n, 5))
    t = nlx.MerkleTree(ctx, leaves, cap_h)
    dig, cap = orc.merkle_build(leaves, cap_h)
    assert np.array_equal(t.digests, dig)          # every level, level-major
    assert np.array_equal(t.cap, cap)
    for idx in sorted({0, 1, n // 3, n - 2, n - 1}):
        path = t.prove(idx)
        assert np.array_equal(path, np.asarray(orc.merkle_prove(dig, n, cap_h, idx), dtype=np.uint64).reshape(-1, 4))
        assert orc.merkle_verify(leaves[idx], idx, path, t.cap, cap_h)


WORDS = [0, 1, P - 1, 0xFFFFFFFF, 1 << 32, (1 << 64) - (1 << 32)]   # the last one is p - 1 again, as the issue lists it


def test_tree_level_of_worst_case_words(nlx, ctx, orc):
    """A four-word leaf is its own digest, so the first level's children ARE these words: every word in every one of the eight
    rate positions of a quad (slots 0 and 1 of lanes 0 .. 3) beside random words, in all eight at once, and in random mixtures.
    (Words in [p, 2^64) cannot reach a tree level through the ABI: every digest is canonical where it is stored, a four-word
    leaf included - the last assertion pins that.)"""
    rng = np.random.default_rng(64)
    states = []
    for w in WORDS:
        for pos in range(8):
            s = rand_field(rng, 8)
            s[pos] = w
            states.append(s)
        states.append(np.full(8, w, dtype=np.uint64))
    n_states = 128
    while len(states) < n_states:
        states.append(np.array([WORDS[i] for i in rng.integers(0, len(WORDS), size=8)], dtype=np.uint64))
    leaves = np.array(states, dtype=np.uint64).reshape(2 * n_states, 4)
    t = nlx.MerkleTree(ctx, leaves, 0)
    dig, cap = orc.merkle_build(leaves, 0)
    assert np.array_equal(t.digests, dig)
    assert np.array_equal(t.cap, cap)
    assert (t.digests < np.uint64(P)).all()
    loose = leaves.copy()
    loose[3] = [P, P + 1, (1 << 64) - 1, 0xFFFFFFFF00000002]
    canon = loose.copy()
    canon[3] = [int(v) % P for v in loose[3]]
    assert np.array_equal(nlx.MerkleTree(ctx, loose, 0).digests, orc.merkle_build(canon, 0)[0])


def _stark_bytes_equal(nlx, ctx, orc, air, t, pis, db, cfg):
    S = nlx.stark
    st = S.Stark(air, db, S.StarkConfig(**cfg))
    want = orc.stark_prove(st.desc, t, pis)
    pr = st.build(ctx)
    got = pr.prove(t, pis)
    pr.close()
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        pytest.fail("STARK proof bytes differ from the oracle, first at byte %d of %d" % (int(np.nonzero(a != b)[0][0]), len(want)))
    assert orc.stark_verify(st.desc, got) == 1


@pytest.mark.parametrize("db,cap_h", [(5, 4), (6, 0), (7, 1), (11, 4)])
def test_three_trees_per_launch(nlx, ctx, orc, db, cap_h):
    """batch_cols = 24 on 64 columns: three trees per commitment round (24 + 24 + 16), every launch covers them (blockIdx.y, trees
    tree_words apart); the proof holds each tree's cap and the opened paths.  2^(db + 1) leaves per tree: 2, 7 (6 + 1), 7 and 8
    (6 + 2) levels."""
    S = nlx.stark
    air = S.wide_air(64, seed=db)
    t, pis = S.wide_trace(air, db, seed=db + 1)
    _stark_bytes_equal(nlx, ctx, orc, air, t, pis, db, dict(batch_cols=24, cap_height=cap_h, fri_num_queries=12, fri_pow_bits=4))


def test_three_trees_where_the_launchers_count_trees(nlx, ctx, orc):
    """2^13 parents on the first level of each of three trees: a level that a single tree hands to the fused sub-wave kernel and
    three trees together (half * n_trees) do not - or the other way round wherever the crossover sits between 2^13 and 3 * 2^13"""
    S = nlx.stark
    air = S.wide_air(24, seed=13)
    t, pis = S.wide_trace(air, 13, seed=14)
    _stark_bytes_equal(nlx, ctx, orc, air, t, pis, 13, dict(batch_cols=8, fri_num_queries=12, fri_pow_bits=4))


# ---- short-trace leaves: k_hash_lde_leaves_wide ---------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,rate_bits", [(2, 1), (0, 3), (5, 1), (3, 3)])   # 2^3 LDE rows: half a wave of quads, the rest spare
@pytest.mark.parametrize("n_cols", [5, 8, 9, 17, 135])                        # last chunk of 5, 0 (full), 1, 1 and 7 words
def test_short_trace_leaves(nlx, ctx, orc, log_n, rate_bits, n_cols):
    rng = np.random.default_rng(100 * n_cols + 10 * log_n + rate_bits)
    vals = rand_field(rng, (n_cols, 1 << log_n))
    cap_h = 1
    pb = nlx.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h)
    ref = orc.commit(vals, rate_bits, cap_h)
    assert np.array_equal(pb.digests(), ref["digests"])
    assert np.array_equal(pb.cap, ref["cap"])
    L = 1 << (log_n + rate_bits)
    idx = np.array(sorted({0, 1, L // 2, L - 1}), dtype=np.uint64)
    rows, paths = pb.open_rows(idx)
    for j, i in enumerate(idx):
        assert np.array_equal(rows[j], ref["leaves"][int(i)])
        assert np.array_equal(paths[j], orc.merkle_prove(ref["digests"], L, cap_h, int(i)))


def _progression_case(S, n_cols, db, seed):
    """column c is the progression a_c + i k_c: any column count, every row different"""
    rng = np.random.default_rng(seed)
    air = S.Air(n_cols, 1)
    a = [int(v) for v in rand_field(rng, n_cols)]
    k = [int(v) for v in rand_field(rng, n_cols)]
    for c in range(n_cols):
        air.constraint_transition(air.next(c) - (air.local(c) + k[c]))
    air.constraint_first_row(air.local(0) - air.public(0))
    i = np.arange(1 << db, dtype=object)
    t = np.array([[(a[c] + int(j) * k[c]) % P for j in i] for c in range(n_cols)], dtype=np.uint64)
    return air, t, np.array([a[0]], dtype=np.uint64)


@pytest.mark.parametrize("n_cols,batch_cols,db", [(19, 8, 5), (19, 8, 4), (51, 24, 5), (51, 24, 4)])
def test_last_batch_is_its_own_digest(nlx, ctx, orc, n_cols, batch_cols, db):
    """19 columns in batches of 8 and 51 in batches of 24: the last batch has three columns, so its leaf is the row itself
    (hash_or_noop).  Batches of 24 are wide enough for the sub-wave leaf kernel, whose three-column case this reaches (2^5 LDE
    rows are the shortest STARK the library builds; launches with spare quads are test_short_trace_leaves' 2^3 rows)."""
    S = nlx.stark
    air, t, pis = _progression_case(S, n_cols, db, seed=n_cols + db)
    cfg = dict(batch_cols=batch_cols, cap_height=min(4, db + 1), fri_num_queries=12, fri_pow_bits=4)
    if db < 5:
        cfg.update(fri_final_poly_bits=2)
    _stark_bytes_equal(nlx, ctx, orc, air, t, pis, db, cfg)


# ---- FRI leaves: k_fri_leaves_wide<2, 3, 4> ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("arity_bits", [2, 3, 4])
@pytest.mark.parametrize("log_n", [6, 10])
def test_fri_layers_below_the_crossover(nlx, ctx, orc, log_n, arity_bits):
    """whole proofs whose every FRI layer (2^(log_n + 3 - arity_bits) leaves and fewer) is hashed by the sub-wave kernel; at
    2^6 rows the later layers have fewer than sixteen leaves (spare quads)"""
    config = nlx.CircuitConfig(fri_arity_bits=arity_bits, fri_final_poly_bits=1, cap_height=1, fri_num_queries=9, fri_pow_bits=4)
    syn = nlx.SyntheticCircuit(log_n, seed=500 + 10 * log_n + arity_bits, config=config, pct_poseidon=20, pct_arithmetic=30,
                               pct_base_sum=5, pct_constant=5)
    ref = orc.Circuit.from_synthetic(syn)
    cd = nlx.CircuitData.from_synthetic(ctx, syn)
    want = ref.prove(syn.wires, syn.public_inputs)
    got = cd.prove(syn.wires, syn.public_inputs)
    cd.close()
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        pytest.fail("proof bytes differ from the oracle, first at byte %d of %d" % (int(np.nonzero(a != b)[0][0]), len(want)))
    assert ref.verify(got) == 1
    ref.close()
