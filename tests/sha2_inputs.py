"""Raw compression blocks for the SHA-2 trace and binding-round tests (tests/test_sha2_reference.py, tests/test_gpu_sha2_trace.py,
tests/test_gpu_bind_round.py, tests/golden/gen_sha2_reference_digests.py): words nobody padded, aimed at the trace kernels'
edges rather than at messages."""
import hashlib

import numpy as np

MESSAGES = {"sha256": [b"abc", bytes(range(100)), b"", b"x" * 55, b"y" * 56, b"z" * 64],       # tests/test_sha256_air.py
            "sha512": [b"abc", bytes(range(150)), b"", b"x" * 111, b"y" * 112, b"z" * 128]}    # tests/test_sha512_air.py
MESSAGES_LOG_BLOCKS = 4
# (0, 0) makes every Horner step vanish, (1, 0) turns the fingerprint into a plain sum; the last has both words >= p
GAMMAS = [(0, 0), (1, 0), ((1 << 64) - 1, 0xFFFFFFFF00000001 + 5)]
GAMMA = (0x0123456789abcdef, 0x0fedcba987654321)


def raw_blocks(bits, log_blocks, flags="mixed"):
    """(blocks [2^log_blocks, 16] uint32 / uint64, is_first uint8): seeded random words and flags, then
      block 1 all-ones words and block 2 all-zero words (the largest and the smallest carries),
      flags == "mixed": is_first[0] = 0 (block 0 starts a message all the same), one message over blocks 62..66 (a chain walked
        across the 64-block workgroup boundary), the last block not a message start;
      flags == "ones" / "zeros": every flag 1 / 0 (zeros: one lane walks every block).
    Overrides that need blocks the size does not have are dropped."""
    nb = 1 << log_blocks
    rng = np.random.default_rng(20261020 + bits + log_blocks)
    blocks = rng.integers(0, (1 << bits) - 1, size=(nb, 16), dtype=np.uint64, endpoint=True).astype(np.uint32 if bits == 32 else np.uint64)
    first = rng.integers(0, 2, size=nb).astype(np.uint8)
    if nb > 2:
        blocks[1], blocks[2] = (1 << bits) - 1, 0
    if flags == "mixed":
        first[0] = 0
        if nb > 67:
            first[62:68] = [1, 0, 0, 0, 0, 1]
        first[nb - 1] = 0
    else:
        first[:] = 1 if flags == "ones" else 0
    return blocks, first


_REFERENCE = {}


def reference(nlx, name, log_blocks, flags="mixed"):
    """(AIR module, blocks, is_first, reference trace, its final chaining value) of raw_blocks, computed once per session and
    shared: nobody writes to the arrays"""
    key = (name, log_blocks, flags)
    if key not in _REFERENCE:
        mod = getattr(nlx, name + "_air")
        blocks, first = raw_blocks(32 if name == "sha256" else 64, log_blocks, flags)
        trace, hout = mod.reference_trace(blocks, first)
        for a in (blocks, first, trace, hout):
            a.setflags(write=False)
        _REFERENCE[key] = (mod, blocks, first, trace, hout)
    return _REFERENCE[key]


def device_trace(nlx, ctx, name, blocks, first, log_blocks):
    """(trace, digest) from nlx_sha256_trace / nlx_sha512_trace, called directly (the provers take log_blocks >= 2 only); the
    output buffer starts out as a pattern no column holds"""
    mod = getattr(nlx, name + "_air")
    trace = np.full((mod.N_COLS, 4 << log_blocks), 0xDEADDEADDEADDEAD, dtype=np.uint64)
    digest = np.zeros(8, dtype=np.uint64)
    ctx.check(getattr(nlx._lib.dll, "nlx_%s_trace" % name)(ctx.handle, blocks.ctypes.data, first.ctypes.data, log_blocks,
                                                           trace.ctypes.data, digest.ctypes.data))
    return trace, digest


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
    return h.hexdigest()


def reference_digests(mod, blocks, first, gammas):
    """SHA-256 over the bytes of what an AIR module's Python reference computes: the trace, its final chaining value, and per gamma
    the binding columns followed by the total"""
    trace, hout = mod.reference_trace(blocks, first)
    out = {"reference_trace": _sha(trace), "final_chaining_value": _sha(hout)}
    for g in gammas:
        cols, total = mod.binding_columns(blocks, first, g)
        out["binding_columns gamma=(%#x, %#x)" % g] = _sha(cols, np.array([int(v) for v in total], dtype=np.uint64))
    return out


def reference_cases(mod, name):
    """{case name: digests} of tests/golden/sha2_reference_digests.json: the test file's messages at their log_blocks, and the raw
    blocks at log_blocks = 2"""
    blocks, first, _ = mod.blocks_for_messages(MESSAGES[name], MESSAGES_LOG_BLOCKS)
    raw, raw_first = raw_blocks(32 if name == "sha256" else 64, 2)
    return {"messages log_blocks=%d" % MESSAGES_LOG_BLOCKS: reference_digests(mod, blocks, first, [GAMMA]),
            "raw_blocks log_blocks=2": reference_digests(mod, raw, raw_first, [GAMMA] + GAMMAS)}
