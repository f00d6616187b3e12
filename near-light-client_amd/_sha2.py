"""What sha256_air.py and sha512_air.py share: everything about a SHA-2 compression AIR except the constraint program.

One `Sha2` object per hash - word size, round count, rounds per row and rotation amounts - gives the column map, the round
constants, padding, the plain-Python reference trace (tests only; the product path generates the trace on the GPU), the
binding fingerprint and a CPU round function; `Sha2Prover` is the device prover both AIR modules subclass.

A word is BITS = 32 H bits, committed as bits and added as H 32-bit halves chained by their carries (H = 1: one plain 32-bit
addition).  Column map of a row, SLOTS round slots first:

    oA = 0, oE = BITS, oW = 2 BITS, oCA = 3 BITS, oCE = oCA + 3 H, oCW = oCE + 3 H, oSW = oCW + 2 H, SLOT = oSW + H
    PA = SLOTS SLOT, PE = PA + 4 BITS, HIN = PE + 4 BITS, CY = HIN + 8 H, IS_FIRST = CY + 8 H

Nothing here touches the ctypes layer at import time (airgen.py imports the AIR modules without the built library).
"""
import hashlib
import math
import struct

import numpy as np

from .stark import Stark, StatementProver

GL = 0xFFFFFFFF00000001
M32 = 0xFFFFFFFF
ROWS_PER_BLOCK = 4


def _first_primes(count):
    primes, c = [], 2
    while len(primes) < count:
        if all(c % q for q in primes if q * q <= c):
            primes.append(c)
        c += 1
    return primes


def _icbrt(v):
    lo, hi = 0, 1 << ((v.bit_length() + 2) // 3 + 1)
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if mid * mid * mid <= v:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _ext_mul(x, y):
    return (x[0] * y[0] + 7 * x[1] * y[1]) % GL, (x[0] * y[1] + x[1] * y[0]) % GL


def _absorb(acc, gamma, elems):
    for v in elems:
        acc = _ext_mul(acc, gamma)
        acc = ((acc[0] + v) % GL, acc[1])
    return acc


class Sha2:
    def __init__(self, bits, rounds, slots, s0, s1, S0, S1):   # noqa: N803  s0 / s1: (rotate, rotate, shift); S0 / S1: three rotations
        self.BITS, self.ROUNDS, self.SLOTS, self.H = bits, rounds, slots, bits // 32
        self.MASK = (1 << bits) - 1
        self.rot = (s0, s1, S0, S1)
        self.name = "sha%d" % (8 * bits)
        self.dtype = np.uint32 if bits == 32 else np.uint64
        self.fmt = "I" if bits == 32 else "Q"
        h = self.H
        self.offsets = (0, bits, 2 * bits, 3 * bits, 3 * bits + 3 * h, 3 * bits + 6 * h, 3 * bits + 8 * h)   # oA oE oW oCA oCE oCW oSW
        self.SLOT = 3 * bits + 9 * h
        self.PA = slots * self.SLOT
        self.PE = self.PA + 4 * bits
        self.HIN = self.PE + 4 * bits
        self.CY = self.HIN + 8 * h
        self.IS_FIRST = self.CY + 8 * h
        self.N_COLS = self.IS_FIRST + 1
        # FIPS 180-4 §4.2.2-3 / §5.3.3-5: first BITS bits of the fractional parts of the cube / square roots of the first primes,
        # computed with integer arithmetic
        self.K = [_icbrt(q << (3 * bits)) & self.MASK for q in _first_primes(rounds)]
        self.IV = [math.isqrt(q << (2 * bits)) & self.MASK for q in _first_primes(8)]

    def halves(self, x):
        """a word -> its H 32-bit halves, low first"""
        return tuple((x >> (32 * h)) & M32 for h in range(self.H))

    def digest_halves(self, words):
        """eight digest words -> the 8 H public inputs (the halves of each word, low first)"""
        return np.array([v for w in words for v in self.halves(int(w))], dtype=np.uint64)

    def pad_message(self, msg):
        """FIPS 180-4 §5.1 padding -> list of 16-word blocks."""
        bb = 2 * self.BITS                                  # block bytes; the length field is bb / 8 bytes
        data = msg + b"\x80" + b"\x00" * ((bb - 1 - bb // 8 - len(msg)) % bb) + (len(msg) * 8).to_bytes(bb // 8, "big")
        assert len(data) % bb == 0
        return [list(struct.unpack(">16" + self.fmt, data[i:i + bb])) for i in range(0, len(data), bb)]

    def blocks_for_messages(self, messages, log_blocks=None):
        """The padded blocks of `messages`, preceded by as many empty messages as it takes to fill 2^log_blocks
        blocks - the filler goes FIRST so that the AIR's public output (the last block's chaining value) is the
        digest of the caller's last message.
        Returns (blocks [n_blocks,16] of the hash's word type, is_first uint8 [n_blocks], digest words uint64[8] of the last
        message)."""
        blocks, first = [], []
        for m in messages:
            pb = self.pad_message(m)
            blocks += pb
            first += [1] + [0] * (len(pb) - 1)
        need = max(1, len(blocks))
        lb = (need - 1).bit_length() if log_blocks is None else log_blocks
        if need > (1 << lb):
            raise ValueError("messages need %d blocks > 2^%d" % (need, lb))
        fill = (1 << lb) - len(blocks)
        blocks = self.pad_message(b"") * fill + blocks
        first = [1] * fill + first
        digest = struct.unpack(">8" + self.fmt, hashlib.new(self.name, messages[-1] if messages else b"").digest())
        return np.array(blocks, dtype=self.dtype), np.array(first, dtype=np.uint8), np.array(digest, dtype=np.uint64)

    def rotr(self, x, r):
        return ((x >> r) | (x << (self.BITS - r))) & self.MASK

    def s0(self, x):
        a, b, c = self.rot[0]
        return self.rotr(x, a) ^ self.rotr(x, b) ^ (x >> c)

    def s1(self, x):
        a, b, c = self.rot[1]
        return self.rotr(x, a) ^ self.rotr(x, b) ^ (x >> c)

    def round_terms(self, a1, a2, a3, e1, e2, e3):
        """(S1(e), Ch, S0(a), Maj) of a round"""
        (p, q, r), (u, v, w) = self.rot[2], self.rot[3]
        return (self.rotr(e1, u) ^ self.rotr(e1, v) ^ self.rotr(e1, w), (e1 & e2) ^ (~e1 & e3 & self.MASK),
                self.rotr(a1, p) ^ self.rotr(a1, q) ^ self.rotr(a1, r), (a1 & a2) ^ (a1 & a3) ^ (a2 & a3))

    def schedule(self, block):
        w = [int(x) for x in block]
        for i in range(16, self.ROUNDS):
            w.append((w[i - 16] + self.s0(w[i - 15]) + w[i - 7] + self.s1(w[i - 2])) & self.MASK)
        return w

    def add(self, terms):
        """sum of words mod 2^BITS as the AIR does it, half by half: (value, the carry out of every half)"""
        v, carries, c = 0, [], 0
        for h in range(self.H):
            s = sum((t >> (32 * h)) & M32 for t in terms) + c
            c = s >> 32
            v |= (s & M32) << (32 * h)
            carries.append(c)
        return v, carries

    def reference_trace(self, blocks, is_first):
        """(N_COLS, 4 * n_blocks) trace, plain Python.  Mirrors the column semantics documented in the AIR modules."""
        H, SLOTS, ROUNDS, BITS, SLOT = self.H, self.SLOTS, self.ROUNDS, self.BITS, self.SLOT   # noqa: N806
        oA, oE, oW, oCA, oCE, oCW, oSW = self.offsets                                          # noqa: N806
        nb = len(blocks)
        t = np.zeros((self.N_COLS, ROWS_PER_BLOCK * nb), dtype=np.uint64)

        def put_bits(base, row, v, cnt=BITS):
            for i in range(cnt):
                t[base + i, row] = (v >> i) & 1

        scheds = [self.schedule(b) for b in blocks]
        h = list(self.IV)
        for bi in range(nb):
            if is_first[bi] or bi == 0:
                h = list(self.IV)
            w = scheds[bi]
            ext = scheds[bi - 1][ROUNDS - 16:] + w            # ext[16 + t] = W_t; t < 0 reaches the previous block (cyclic)
            a = [h[3], h[2], h[1], h[0]]                      # a[t + 4], e[t + 4] for t = -4..ROUNDS-1
            e = [h[7], h[6], h[5], h[4]]
            ca, ce = [], []
            for r in range(ROUNDS):
                s1, ch, s0, mj = self.round_terms(a[-1], a[-2], a[-3], e[-1], e[-2], e[-3])
                t1 = [e[-4], s1, ch, self.K[r], w[r]]
                (va, cva), (ve, cve) = self.add(t1 + [s0, mj]), self.add([a[-4]] + t1)
                a.append(va)
                e.append(ve)
                ca.append(cva)
                ce.append(cve)
            for q in range(ROWS_PER_BLOCK):
                row = ROWS_PER_BLOCK * bi + q
                for j in range(SLOTS):
                    r = SLOTS * q + j
                    base = j * SLOT
                    put_bits(base + oA, row, a[r + 4])
                    put_bits(base + oE, row, e[r + 4])
                    put_bits(base + oW, row, w[r])
                    sw, cw = self.add([self.s1(ext[16 + r - 2]), ext[16 + r - 7], self.s0(ext[16 + r - 15]), ext[16 + r - 16]])
                    for hh in range(H):
                        put_bits(base + oCA + 3 * hh, row, ca[r][hh], 3)
                        put_bits(base + oCE + 3 * hh, row, ce[r][hh], 3)
                        put_bits(base + oCW + 2 * hh, row, cw[hh], 2)
                        t[base + oSW + hh, row] = self.halves(sw)[hh]
                for k in range(4):
                    put_bits(self.PA + BITS * k, row, a[SLOTS * q + 3 - k])
                    put_bits(self.PE + BITS * k, row, e[SLOTS * q + 3 - k])
                for k in range(8):
                    t[self.HIN + H * k:self.HIN + H * (k + 1), row] = self.halves(h[k])
                if q == 0:
                    t[self.IS_FIRST, row] = 1 if (is_first[bi] or bi == 0) else 0
            for k in range(8):
                h[k], cy = self.add([h[k], a[ROUNDS + 3 - k] if k < 4 else e[ROUNDS + 7 - k]])
                t[self.CY + H * k:self.CY + H * (k + 1), ROWS_PER_BLOCK * bi + 3] = cy
        return t, np.array(h, dtype=np.uint64)

    def block_outputs(self, blocks, is_first):
        """output chaining value of every block (the eight words the AIR absorbs on a block's last row)"""
        m = self.MASK
        outs, h = [], list(self.IV)
        for bi, blk in enumerate(blocks):
            if is_first[bi] or bi == 0:
                h = list(self.IV)
            w = self.schedule(blk)
            a, b, c, d, e, f, g, hh = h
            for r in range(self.ROUNDS):
                s1, ch, s0, mj = self.round_terms(a, b, c, e, f, g)
                t1 = (hh + s1 + ch + self.K[r] + w[r]) & m
                hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & m, c, b, a, (t1 + s0 + mj) & m
            h = [(x + y) & m for x, y in zip(h, (a, b, c, d, e, f, g, hh))]
            outs.append(list(h))
        return outs

    def _block_elements(self, blocks, is_first):
        """per block: (the 1 + 16 H elements absorbed on its first row, the 8 H absorbed on its last)"""
        for bi, (blk, out) in enumerate(zip(blocks, self.block_outputs(blocks, is_first))):
            yield ([1 if (is_first[bi] or bi == 0) else 0] + [v for x in blk for v in self.halves(int(x))],
                   [v for x in out for v in self.halves(x)])

    def fingerprint(self, blocks, is_first, gamma):
        """What the proof's round value must be for these padded blocks (blocks_for_messages): Horner in F_p^2 over, block by
        block, the message-start flag, the 16 message words and the 8 output chaining words, every word as its halves (low
        first) - the relying party's side of the binding."""
        acc = (0, 0)
        for head, tail in self._block_elements(blocks, is_first):
            acc = _absorb(acc, gamma, head + tail)
        return acc

    def binding_columns(self, blocks, is_first, gamma):
        """Round-1 accumulator columns (2, 4 n_blocks) and the total, plain Python (tests and the oracle path)."""
        out = np.zeros((2, ROWS_PER_BLOCK * len(blocks)), dtype=np.uint64)
        acc = (0, 0)
        for bi, (head, tail) in enumerate(self._block_elements(blocks, is_first)):
            for q in range(ROWS_PER_BLOCK):
                out[0, 4 * bi + q], out[1, 4 * bi + q] = acc
                acc = _absorb(acc, gamma, head if q == 0 else (tail if q == 3 else []))
        return out, acc

    def cpu_rounds(self, blocks, is_first, trace):
        """round function for a CPU prover of this AIR (tests, the bench's cpu_baseline): round 0 = the given trace, round 1 =
        the binding accumulator and its total for the gamma the prover drew"""
        def fn(rnd, known):
            if rnd == 0:
                return trace
            cols, total = self.binding_columns(blocks, is_first, known[:2])
            return cols, list(total)
        return fn


class Sha2Prover(StatementProver):
    """Proves one SHA-2 hash of a batch of messages on one GPU: trace generation (nlx_sha*_trace) straight into HBM, the binding
    accumulator (nlx_sha*_bind_round) once the prover has drawn gamma, and the two-round STARK (nlx_stark_prove_rounds) on the
    device-resident columns.  2^log_blocks compression blocks per proof.  A subclass names its Sha2 object, its AIR builder and
    its two entry points of the library."""
    sha2 = build_air = trace_fn = bind_fn = None

    def __init__(self, ctx, log_blocks, config=None, segment_nodes=None, step_tag=None):
        if log_blocks < 2:
            raise ValueError("at least four blocks per proof (a block is four trace rows, a STARK at least sixteen)")
        air = self.build_air(tagged=step_tag is not None)
        if segment_nodes is not None:
            air.segment_nodes = segment_nodes
        super().__init__(ctx, Stark(air, log_blocks + 2, config), step_tag)
        self.log_blocks = log_blocks
        self._trace = self._acc = None

    def generate_trace(self, blocks, is_first):
        """Returns (device round-0 trace tensor [N_COLS, n] int64, digest words uint64[8])."""
        import torch
        from ._lib import dll
        blocks = np.ascontiguousarray(blocks, dtype=self.sha2.dtype)
        is_first = np.ascontiguousarray(is_first, dtype=np.uint8)
        if blocks.shape != (1 << self.log_blocks, 16) or is_first.shape != (1 << self.log_blocks,):
            raise ValueError("expected 2^%d blocks" % self.log_blocks)
        n = ROWS_PER_BLOCK << self.log_blocks
        if self._trace is None:
            self._trace = torch.empty((self.sha2.N_COLS, n), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
            self._acc = torch.empty((2, n), dtype=torch.int64, device=self._trace.device)
        digest = np.zeros(8, dtype=np.uint64)
        self.ctx.check(getattr(dll, self.trace_fn)(self.ctx.handle, blocks.ctypes.data, is_first.ctypes.data, self.log_blocks,
                                                   self._trace.data_ptr(), digest.ctypes.data))
        return self._trace, digest

    def round1(self, known):
        """The binding accumulator for gamma = known[0:2] (device columns) and its total, the proof's round value."""
        from ._lib import dll
        gamma = np.array([int(known[0]), int(known[1])], dtype=np.uint64)
        total = np.zeros(2, dtype=np.uint64)
        self.ctx.check(getattr(dll, self.bind_fn)(self.ctx.handle, self._trace.data_ptr(), self.log_blocks, gamma.ctypes.data,
                                                  self._acc.data_ptr(), total.ctypes.data))
        self.last_total = (int(total[0]), int(total[1]))
        return self._acc, [int(total[0]), int(total[1])]

    def prove_trace(self, public_inputs):
        """The proof for the trace generate_trace() left on the device (public inputs: the last digest's halves)."""
        return self._prove(self._trace, public_inputs)

    def check_trace(self, public_inputs, challenges=None):
        """A stark.TraceReport for the trace generate_trace() left on the device: the rounds prove_trace() would run, checked
        against the AIR instead of proved (StarkProver.check_rounds)."""
        return self._check(self._trace, public_inputs, challenges)

    def prove(self, messages):
        """Returns (proof bytes, digest words of the last message in the batch)."""
        blocks, first, want = self.sha2.blocks_for_messages(messages, self.log_blocks)
        _, digest = self.generate_trace(blocks, first)
        assert np.array_equal(digest, want)  # the GPU's chaining value is the real digest
        return self.prove_trace(self.sha2.digest_halves(digest)), digest

    def close(self):
        super().close()
        self._trace = self._acc = None
