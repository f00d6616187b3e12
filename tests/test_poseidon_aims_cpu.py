"""CPU: aimed Poseidon states (tests/poseidon_aims.py) - inputs run backwards from a worst case at a chosen layer.

Checks the construction (every aimed input, traced forward, meets its target at its layer and hashes like the naive model, the C
oracle and the BN128 reference model), then runs the device-schedule models on the worst cases: the generator's model of the
fused partial rounds (tools/gen_poseidon_blocks.py) with the representative and junk-slot choices pinned at their extremes
instead of drawn at random, and the BN128 device header built on the host (tests/native/poseidon_bn128_check.cpp) with its
bounds asserted mid-permutation."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import poseidon_aims as pa

gpb = pa.gpb
P, R = pa.P, pa.R


class Pinned:
    """a stand-in for the model's random.Random: `random()` picks loose()'s representative (< 0.5: x + p wherever it is below
    2^64) and cycles through `reps`, one entry per call - loose() is called for the twelve state elements, then the block's two
    S-box outputs, so a cycle of two alternates the choice element by element; `randrange` fills the junk K slots 14, 15"""

    def __init__(self, reps, junk):
        self.reps, self.junk, self.i = list(reps), junk, 0

    def random(self):
        self.i += 1
        return self.reps[(self.i - 1) % len(self.reps)]

    def randrange(self, a, b):
        assert a <= self.junk < b
        return self.junk


def test_gl_aims_hit_their_targets(orc):
    aims = pa.gl_aims()
    seen = set()
    outs = []
    for name, st, (kind, layer, z) in aims:
        assert all(0 <= x < P for x in st)
        sbox_in, mds_in, out = pa.trace(st)
        if kind == "mds":
            assert mds_in[layer] == z, name
        elif kind == "held":
            assert mds_in[layer] == [(x + d) % P for x, d in zip(z, pa.device_offset(layer))], name
        else:
            assert sbox_in[layer][0] == z and mds_in[layer][1:] == [z] * (pa.T - 1), name
        assert out == gpb.naive(st), name
        outs.append(out)
        seen.add((kind, layer, name.split(" @ ")[0]))
    pats = [n for n, _ in pa.gl_patterns()]
    assert {(k, l, n) for k, l, n in seen if k == "mds"} == {("mds", l, n) for l in range(30) for n in pats}
    assert {(k, l, n) for k, l, n in seen if k == "held"} == {("held", l, n) for l in (4, 7, 10, 13, 16, 19, 22, 25) for n in pats}
    assert {(k, l) for k, l, _ in seen if k == "sbox0"} == {("sbox0", l) for l in range(4, 26)}
    got = orc.poseidon_permute(np.array([st for _, st, _ in aims], dtype=np.uint64))
    assert got.tolist() == outs


@pytest.mark.parametrize("row_len", [8, 9, 16, 20, 135])
def test_gl_rate_rows_hit_the_first_layer(orc, row_len):
    """an aimed sponge row (the GPU tests' leaf rows): every absorb's first-layer MDS input holds the pattern in the slots the
    absorb overwrites, whatever the capacity and the slots it keeps hold"""
    for name, z in pa.gl_patterns():
        row = pa.gl_rate_row(z[:8], row_len)
        s = [0] * pa.T
        for c in range(0, row_len, 8):
            chunk = row[c:c + 8]
            s[:len(chunk)] = chunk
            _, mds_in, s = pa.trace(s)
            assert mds_in[0][:len(chunk)] == z[:len(chunk)], (name, c)
        assert s[:4] == orc.hash_or_noop(np.array(row, dtype=np.uint64)).tolist(), name


def test_device_offset_is_the_block_models():
    """an aim in the device's basis lands in the state the generator's device model holds: its block_model's input (z_held =
    that state after element 0's S-box) at blocks 0 .. 6, the last block's output at round 25"""
    tb = gpb.tables()
    blocks, layer = gpb.constants(tb)
    held = []
    orig = gpb.block_model

    def spy(tb_, kap, s, rnd):
        held.append(list(s))
        out = orig(tb_, kap, s, rnd)
        held.append(list(out[0]))
        return out
    gpb.block_model = spy
    try:
        for name, st, (kind, lay, z) in pa.gl_aims():
            if kind != "held" or name.split(" @ ")[0] not in ("fill p-2", "half p-1/eps", "row0 max"):
                continue
            del held[:]
            gpb.model(tb, blocks, layer, st, Pinned([0.5], 0))
            b = (lay - gpb.FIRST) // gpb.K
            s = held[2 * b] if b < gpb.N_BLOCKS else held[-1]
            assert [gpb.sbox(s[0])] + s[1:] == z, name
    finally:
        gpb.block_model = orig


def _block_aims():
    """the aims whose worst case is inside the fused blocks or at round 25: naive-basis layers 4 .. 25, the device-basis ones,
    element 0's S-box inputs"""
    return [a for a in pa.gl_aims() if a[2][0] in ("held", "sbox0") or 4 <= a[2][1] <= 25]


def _run_block_model(aims, rnd):
    """the generator's model on `aims` with `rnd`: equal to the naive permutation, plane sums >= 0 (asserted inside
    block_model) and within the bound; returns (largest plane sum, every representative loose() chose)"""
    tb = gpb.tables()
    blocks, layer = gpb.constants(tb)
    reps = []
    orig = gpb.loose

    def spy(x, rnd_):
        v = orig(x, rnd_)
        reps.append(v)
        return v
    gpb.loose = spy
    try:
        worst = 0
        for name, st, _ in aims:
            got, dmax = gpb.model(tb, blocks, layer, st, rnd)
            assert got == gpb.naive(st), name
            assert dmax <= tb["dmax_main"], name
            worst = max(worst, dmax)
    finally:
        gpb.loose = orig
    assert all(0 <= v < 1 << 64 for v in reps)
    assert worst > tb["dmax_main"] // 2
    return worst, reps


@pytest.mark.parametrize("rep,junk", [(0.0, -128), (0.99, 127)], ids=["x+p,-128", "x,127"])
def test_block_model_worst_representatives(rep, junk):
    """the generator's check() draws the device's representatives (loose(): x or x + p) and the junk slots at random, and its
    random states never hold a value below 2^32 - 1 at a block, where x + p exists.  Here the aimed states run with every choice
    x + p (junk slots -128), then every choice x (junk 127): the result equals the naive permutation, every plane sum is >= 0
    and the largest stays within the bound the recombination is written for.  (bounds() in the generator covers the analytic
    worst case over all byte values; this runs the schedule itself on the states closest to it.)"""
    _, reps = _run_block_model(_block_aims(), Pinned([rep], junk))
    if rep < 0.5:
        assert (1 << 64) - 1 in reps and P in reps         # the all-0xFF representative of eps - 1, and 0 held as p
    else:
        assert not any(v >= P for v in reps)


@pytest.mark.parametrize("cycle", [(0.0, 0.99), (0.99, 0.0), (0.0, 0.0, 0.99)], ids=["x+p,x", "x,x+p", "x+p,x+p,x"])
def test_block_model_mixed_representatives(cycle):
    """the choice mixed element by element (with signed digits a mix can reach sums that all-x + p or all-x cannot), on the
    aims held at the blocks' own inputs and element 0's S-box inputs"""
    aims = [a for a in pa.gl_aims() if a[2][0] in ("held", "sbox0")]
    _, reps = _run_block_model(aims, Pinned(cycle, -128))
    assert any(v >= P for v in reps) and any(v < (1 << 64) - P for v in reps)


def test_bn_aims_hit_their_targets():
    seen = set()
    for name, st, (where, rnd, v) in pa.bn_aims():
        assert all(0 <= x < R for x in st)
        sbox_in, mds_in, out = pa.bn_trace(st)
        assert (sbox_in if where == "sbox" else mds_in)[rnd] == v, name
        assert out == pa.pbn.permute(st), name
        seen.add((where, rnd, name.split(" @ ")[0]))
    pats = [n for n, _ in pa.bn_patterns()]
    assert seen == {(w, r, n) for w in ("sbox", "mds") for r in range(64) for n in pats}
    assert pa.LIMBS_AT_MASK < R and pa.LIMBS_AT_MASK + (1 << 232) > R
    assert all((pa.LIMBS_AT_MASK >> (29 * i)) & pa.LIMB_MASK == pa.LIMB_MASK for i in range(8))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pbn_aims") / "poseidon_bn128_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "poseidon_bn128_check.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.split("\n")[:len(lines)]
    return run


def test_bn_header_on_aimed_states(native):
    """the device header's permutation on every aimed state equals the model, and the bounds its header comment states hold
    round after round: state < 2^255 on entry, < 2^256 after the constants, S-box and MDS-row outputs < 2^255, limbs 0..7
    normalised"""
    aims = pa.bn_aims()
    want = [pa.bn_trace(st)[2] for _, st, _ in aims]
    perm = native(["perm " + " ".join("%x" % v for v in st) for _, st, _ in aims])
    trace = native(["trace " + " ".join("%x" % v for v in st) for _, st, _ in aims])
    worst = [0] * 4
    for (name, st, _), w, a, b in zip(aims, want, perm, trace):
        assert [int(x, 16) for x in a.split()] == w, name
        f = b.split()
        assert [int(x, 16) for x in f[:4]] == w, name
        entry, added, sboxed, rows = (int(x, 16) for x in f[4:8])
        assert entry < 1 << 255 and added < 1 << 256 and sboxed < 1 << 255 and rows < 1 << 255, name
        assert f[8] == "1", name
        worst = [max(x, y) for x, y in zip(worst, (entry, added, sboxed, rows))]
    assert worst[1] > R                                          # the lazy representatives do leave [0, r)
