"""GPU: gnark-crypto's point bytes on the device (nlx_bn254_g1_decode / g2_decode / g1_encode / g2_encode; csrc/bn254_codec.hpp /
.hip, near-light-client_amd/bn254_codec.py) against the big-integer model tools/gnark_bytes_model.py.
Counts 1, 63, 64, 65 and 257 (the wave and block edges), both groups, both modes, host and device pointers; every malformed input
alone, at index 0 and at index 64 of a batch.  Every comparison is exact: bytes or words."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_py as bn  # noqa: E402
import gnark_bytes_model as gb  # noqa: E402

pytestmark = pytest.mark.gpu
Q, R = gb.Q, gb.R
E_INVAL, E_RANGE = -1, -4
COUNTS = (1, 63, 64, 65, 257)
HALF_LO, HALF_HI = (Q - 1) // 2, (Q + 1) // 2
UNSET = 0xFFFFFFFF


class Group:
    """one of the two groups: its model functions, sizes and seeded points, made once per module"""

    def __init__(self, g2):
        self.g2, self.width = g2, 16 if g2 else 8
        self.encode, self.decode, self.words = (gb.g2_encode, gb.g2_decode, gb.g2_words) if g2 else (gb.g1_encode, gb.g1_decode, gb.g1_words)
        self.size = gb.G2_SIZE if g2 else gb.G1_SIZE
        rng = random.Random("codec-g2" if g2 else "codec-g1")
        mul, add, gen = (bn.g2_mul, bn.g2_add, bn.G2) if g2 else (bn.g1_mul, bn.g1_add, bn.G1)
        p, step = mul(rng.randrange(1, R), gen), mul(rng.randrange(1, R), gen)
        self.seeded = []
        for _ in range(max(COUNTS)):           # k0 + i d times the generator
            self.seeded.append(p)
            p = add(p, step)
        self.gen, self.neg = gen, mul(R - 1, gen)

    def batch(self, n):
        """seeded multiples, the generator and its negative, infinity at the first, the last and a middle index"""
        pts = list(self.seeded[:n])
        if n >= 5:
            pts[1], pts[2] = self.gen, self.neg
            pts[0] = pts[n - 1] = pts[n // 2] = None
        return pts

    def pack(self, pts):
        return np.array([self.words(p) for p in pts], dtype=np.uint64).reshape(len(pts), self.width)

    def bytes_of(self, pts, raw):
        return b"".join(self.encode(p, raw) for p in pts)


@pytest.fixture(scope="module")
def groups():
    return {False: Group(False), True: Group(True)}


def _decode(nlx, ctx, grp, data, raw, subgroup=True, device=False):
    """(the error or None, words, status) of one call: out and status are handed in, so they are there after a refusal"""
    n = len(data) // grp.size[raw]
    kw = {} if not grp.g2 else {"subgroup": subgroup}
    fn = nlx.bn254_g2_decode if grp.g2 else nlx.bn254_g1_decode
    err = None
    if device:
        import torch
        inp = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        out = torch.full((n, grp.width), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()                 # the fills run on torch's stream, the library on its own
    else:
        inp, out, status = data, np.full((n, grp.width), 0x5A5A5A5A, dtype=np.uint64), np.full(n, UNSET, dtype=np.uint32)
    try:
        assert fn(ctx, inp, raw=raw, out=out, status=status, **kw) is out
    except nlx.NlxError as e:
        err = e
    if device:
        out, status = out.cpu().numpy().view(np.uint64), status.cpu().numpy().view(np.uint32)
    return err, out, status


def _encode(nlx, ctx, grp, words, raw, device=False):
    fn = nlx.bn254_g2_encode if grp.g2 else nlx.bn254_g1_encode
    if device:
        import torch
        out = fn(ctx, torch.from_numpy(words.view(np.int64)).to("cuda:0"), raw=raw)
        assert out.is_cuda
        return out.cpu().numpy().tobytes()
    return fn(ctx, words, raw=raw)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
@pytest.mark.parametrize("g2", (False, True), ids=("g1", "g2"))
def test_decode_and_encode_equal_the_model(nlx, ctx, groups, g2, raw, n):
    grp = groups[g2]
    batches = [grp.batch(n)] if n > 1 else [[p] for p in (grp.seeded[0], grp.gen, grp.neg, None)]
    for pts in batches:
        data, words = grp.bytes_of(pts, raw), grp.pack(pts)
        for device in (False, True):
            err, got, status = _decode(nlx, ctx, grp, data, raw, device=device)
            assert err is None, err
            assert np.array_equal(got, words) and not status.any()
            assert _encode(nlx, ctx, grp, words, raw, device=device) == data
            assert _encode(nlx, ctx, grp, got, raw, device=device) == data            # encode(decode(x)) == x


def test_encode_flag_choice_on_synthetic_coordinates(nlx, ctx, groups):
    """encode does not test the curve, so (x, y) pairs that lie on none reach the flag choice: y at the (q +- 1) / 2 boundaries,
    at 1 and q - 1, and over Fq2 with y.A1 = 0 (decided on A0) and with A1 at the boundaries against the opposite A0"""
    ys = (HALF_LO, HALF_HI, 1, Q - 1, HALF_LO - 1, HALF_HI + 1)
    g1 = [(7 + i, y) for i, y in enumerate(ys)]
    g2 = [((7 + i, 9), yy) for i, y in enumerate(ys) for yy in ((y, 0), (Q - 1 - y, y), (0, y))]
    for grp, pts in ((groups[False], g1), (groups[True], g2)):
        flags = {grp.encode(p, False)[0] >> 6 for p in pts}
        assert flags == {2, 3}
        for raw in (False, True):
            assert _encode(nlx, ctx, grp, grp.pack(pts), raw) == grp.bytes_of(pts, raw)


def _with_flag(data, flag):
    return bytes([(data[0] & 0x3F) | (flag << 6)]) + data[1:]


def _twist_x_with_root(rng, want_outside):
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = gb.f2_sqrt(gb.f2_add(gb.f2_mul(gb.f2_mul(x, x), x), gb.B2))
        if y is not None and (not want_outside or not gb.g2_in_subgroup((x, y))):
            return x, y


def _malformed(grp, raw):
    """(name, bytes of one bad point) for this group and mode; the model names the status"""
    rng = random.Random("malformed-%d-%d" % (grp.g2, raw))
    good = grp.seeded[7]
    data = grp.encode(good, raw)
    size = grp.size[raw]
    out = []
    if raw:
        out += [("flag 10 in raw mode", _with_flag(data, 2)), ("flag 11 in raw mode", _with_flag(data, 3))]
    else:
        out.append(("flag 00 in compressed mode", _with_flag(data, 0)))
    out += [("0x40 and a non-zero last byte", bytes([0x40]) + bytes(size - 2) + b"\x01"), ("0x40 and a non-zero second byte", b"\x40\x07" + bytes(size - 2)),
            ("0x41", b"\x41" + bytes(size - 1))]
    lead = 0 if raw else 0x80
    for name, x in (("q", Q), ("2^254 - 1", (1 << 254) - 1)):
        head = bytearray(x.to_bytes(32, "big"))
        head[0] |= lead
        out.append(("first coordinate = " + name, bytes(head) + data[32:]))
    if grp.g2:
        out.append(("A0 = q", data[:32] + Q.to_bytes(32, "big") + data[64:]))
        if raw:
            out += [("Y.A1 = q", data[:64] + Q.to_bytes(32, "big") + data[96:]), ("Y.A0 = q", data[:96] + Q.to_bytes(32, "big"))]
    elif raw:
        out.append(("y = q", data[:32] + Q.to_bytes(32, "big")))
    if raw:
        bumped = (good[0], gb.f2_add(good[1], (1, 0))) if grp.g2 else (good[0], (good[1] + 1) % Q)
        out.append(("a raw point with y + 1", grp.encode(bumped, True)))
    else:
        while True:                                  # an x with no root
            x = (rng.randrange(Q), rng.randrange(Q)) if grp.g2 else rng.randrange(Q)
            rhs = gb.f2_sqrt(gb.f2_add(gb.f2_mul(gb.f2_mul(x, x), x), gb.B2)) if grp.g2 else gb.fq_sqrt(x ** 3 + 3)
            if rhs is None:
                break
        out.append(("an x with no root", _with_flag(grp.encode((x, (0, 0) if grp.g2 else 0), True)[:size], 2)))
    if grp.g2:
        out.append(("a twist point outside the subgroup", grp.encode(_twist_x_with_root(rng, True), raw)))
    return out


@pytest.mark.parametrize("raw", (False, True), ids=("compressed", "raw"))
@pytest.mark.parametrize("g2", (False, True), ids=("g1", "g2"))
def test_malformed_points_alone_first_and_at_64(nlx, ctx, groups, g2, raw):
    grp = groups[g2]
    base = grp.batch(66)
    base_bytes, base_words = grp.bytes_of(base, raw), grp.pack(base)
    size = grp.size[raw]
    seen = set()
    for name, bad in _malformed(grp, raw):
        want_status, _ = grp.decode(bad, raw)
        assert want_status != gb.OK, name
        seen.add(want_status)
        for place in (None, 0, 64):
            if place is None:
                data, words, index = bad, np.zeros((1, grp.width), dtype=np.uint64), 0
            else:
                data = base_bytes[:place * size] + bad + base_bytes[(place + 1) * size:]
                words, index = base_words.copy(), place
                words[place] = 0
            err, got, status = _decode(nlx, ctx, grp, data, raw, device=place == 64)
            assert err is not None and err.code == E_INVAL, (name, place)
            assert "point %d:" % index in str(err), (name, place, str(err))
            want = np.zeros(len(words), dtype=np.uint32)
            want[index] = want_status
            assert np.array_equal(status, want), (name, place, status[index])
            assert np.array_equal(got, words), (name, place)                 # the bad point zero, the good ones still right
    expected = {gb.BAD_FLAG, gb.RANGE, gb.BAD_INFINITY, gb.OFF_CURVE} | ({gb.NOT_IN_SUBGROUP} if g2 else set())
    assert seen == expected
    # two bad points: the message names the lower one, the status words both
    kinds = _malformed(grp, raw)
    data = base_bytes[:3 * size] + kinds[0][1] + base_bytes[4 * size:40 * size] + kinds[-1][1] + base_bytes[41 * size:]
    err, got, status = _decode(nlx, ctx, grp, data, raw)
    assert err is not None and "point 3:" in str(err)
    assert sorted(np.nonzero(status)[0]) == [3, 40] and status[3] == grp.decode(kinds[0][1], raw)[0] and status[40] == grp.decode(kinds[-1][1], raw)[0]


@pytest.mark.parametrize("g2", (False, True), ids=("g1", "g2"))
def test_eight_x_with_a_root_and_eight_without(nlx, ctx, groups, g2):
    """the first eight seeded x for which the model finds no y and the first eight for which it finds one, both flags"""
    grp = groups[g2]
    rng = random.Random("roots-%d" % g2)
    with_root, without = [], []
    while len(with_root) < 8 or len(without) < 8:
        if g2:
            x = (rng.randrange(Q), rng.randrange(Q))
            y = gb.f2_sqrt(gb.f2_add(gb.f2_mul(gb.f2_mul(x, x), x), gb.B2))
        else:
            x = rng.randrange(Q)
            y = gb.fq_sqrt(x ** 3 + 3)
        which = without if y is None else with_root
        if len(which) < 8:
            which.append(x)
    xs = [x for pair in zip(with_root, without) for x in pair]
    for flag in (2, 3):
        data = b"".join(_with_flag(grp.encode((x, (0, 0) if g2 else 0), True)[:grp.size[False]], flag) for x in xs)
        size = grp.size[False]
        model = [grp.decode(data[i * size:(i + 1) * size], False, False) if g2 else grp.decode(data[i * size:(i + 1) * size], False) for i in range(16)]
        assert [st for st, _ in model] == [gb.OK, gb.OFF_CURVE] * 8
        err, got, status = _decode(nlx, ctx, grp, data, False, subgroup=False)
        assert err is not None and err.code == E_INVAL and "point 1:" in str(err)
        assert list(status) == [st for st, _ in model]
        assert np.array_equal(got, grp.pack([p for _, p in model]))
        assert all(gb.fq_largest(p[1]) == (flag == 3) for _, p in model if p is not None) if not g2 else True


def test_no_subgroup_flag(nlx, ctx, groups):
    grp = groups[True]
    p = _twist_x_with_root(random.Random(77), True)
    assert gb.g2_on_curve(p) and not gb.g2_in_subgroup(p)
    for raw in (False, True):
        data = grp.encode(p, raw) + grp.encode(grp.gen, raw)
        err, got, status = _decode(nlx, ctx, grp, data, raw, subgroup=False)
        assert err is None and np.array_equal(got, grp.pack([p, grp.gen])) and not status.any()
        err, got, status = _decode(nlx, ctx, grp, data, raw)
        assert err is not None and err.code == E_INVAL and "point 0:" in str(err) and "subgroup" in str(err)
        assert list(status) == [gb.NOT_IN_SUBGROUP, gb.OK] and np.array_equal(got, grp.pack([None, grp.gen]))


def test_flags_counts_and_refusals(nlx, ctx, groups):
    dll = nlx.lib.dll
    grp = groups[False]
    words = grp.pack(grp.seeded[:2])
    out = np.zeros(64, dtype=np.uint8)
    both, neither = 1 | 2, 0
    for flags in (both, neither, 8 | 1, 4 | 1):                               # NO_SUBGROUP belongs to g2_decode alone
        assert dll.nlx_bn254_g1_encode(ctx.handle, words.ctypes.data, 2, flags, out.ctypes.data) == E_RANGE
        assert dll.nlx_bn254_g1_decode(ctx.handle, out.ctypes.data, 2, flags, words.ctypes.data, None) == E_RANGE
    assert dll.nlx_bn254_g2_decode(ctx.handle, out.ctypes.data, 1, 4 | 1 | 2, words.ctypes.data, None) == E_RANGE
    assert not out.any()
    # n = 0: NLX_OK, nothing is touched, NULL pointers are fine
    assert dll.nlx_bn254_g1_encode(ctx.handle, None, 0, 1, None) == 0 and dll.nlx_bn254_g2_decode(ctx.handle, None, 0, 2, None, None) == 0
    assert nlx.bn254_g1_encode(ctx, np.zeros((0, 8), dtype=np.uint64)) == b"" and nlx.bn254_g2_decode(ctx, b"").shape == (0, 16)
    assert dll.nlx_bn254_g1_encode(ctx.handle, None, 2, 1, out.ctypes.data) == E_INVAL
    # input and output must not overlap
    buf = np.zeros(16, dtype=np.uint64)
    assert dll.nlx_bn254_g1_encode(ctx.handle, buf.ctypes.data, 2, 1, buf.ctypes.data + 64) == E_INVAL
    assert b"overlap" in dll.nlx_last_error(ctx.handle)
    # encode refuses a coordinate that is not below q, naming the index; the other points' bytes are written
    bad = grp.pack(grp.seeded[:5])
    bad[3, 4:8] = np.array([(Q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    out = np.full(5 * 32, 0xEE, dtype=np.uint8)
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_g1_encode(ctx, bad, out=out)
    assert e.value.code == E_RANGE and "point 3:" in str(e.value)
    assert out.tobytes() == grp.bytes_of(grp.seeded[:3], False) + bytes(32) + grp.bytes_of(grp.seeded[4:5], False)
    # a device pointer that is not 16-byte aligned (a slice that starts inside a file's bytes) is served as well
    import torch
    data = grp.bytes_of(grp.seeded[:65], False)
    dev = torch.frombuffer(bytearray(b"\x00" * 4 + data), dtype=torch.uint8).to("cuda:0")[4:]
    assert dev.data_ptr() % 16 == 4
    got = nlx.bn254_g1_decode(ctx, dev)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), grp.pack(grp.seeded[:65]))
    back = torch.zeros(4 + len(data), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()                     # the fill runs on torch's stream, the library on its own
    nlx.bn254_g1_encode(ctx, got, out=back[4:])
    assert back.cpu().numpy().tobytes() == b"\x00" * 4 + data
    # the kernel-timing names, units = points
    ctx.kernel_timing(True)
    nlx.bn254_g1_decode(ctx, data)
    calls, _, _ = ctx.kernel_stats("bn254_g1_decode")
    assert calls == 1 and ctx.kernel_units("bn254_g1_decode") == 65
    ctx.kernel_timing(False)
