"""CPU: nlx_bn254_hash_to_field (the library's own SHA-256, expand_message_xmd and reduction mod r; csrc/sha256_host.hpp,
csrc/bn254_plonk_prove.hip) against the big-integer model tools/gnark_bsb22_model.py hash_to_field (hashlib).  No GPU, no
context: the entry is host code."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bsb22_model as gm  # noqa: E402

# the SHA-256 padding boundaries, shifted by the 64-byte zero prefix of expand_message_xmd (and by its 3 + len(dst) + 1 byte tail)
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 1000]
DSTS = [b"BSB22-Plonk", b"QUUX-V01-CS02-with-expander-SHA256-128-a-second-and-longer-tag"]


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("length", LENGTHS)
def test_hash_to_field_equals_model(nlx, length, dst):
    rng = random.Random(1000 * len(dst) + length)
    msg = bytes(rng.randrange(256) for _ in range(length))
    want = gm.hash_to_field(msg, dst)
    assert nlx.bn254_plonk.hash_to_field_native(msg, dst) == want
    assert nlx.bn254_plonk.hash_to_field(msg, dst) == want          # the binding's hashlib version, the model's twin
    # the words are an fr.Element: the Montgomery residue, below r
    out = np.zeros(4, dtype=np.uint64)
    assert nlx.lib.dll.nlx_bn254_hash_to_field(msg, len(msg), dst, len(dst), out.ctypes.data) == 0
    words = sum(int(out[i]) << (64 * i) for i in range(4))
    assert words < gm.R and words == want * (1 << 256) % gm.R


def test_refusals(nlx):
    out = np.zeros(4, dtype=np.uint64)
    dll = nlx.lib.dll
    assert dll.nlx_bn254_hash_to_field(b"x", 1, b"d", 1, None) == -1
    assert dll.nlx_bn254_hash_to_field(None, 1, b"d", 1, out.ctypes.data) == -1
    assert dll.nlx_bn254_hash_to_field(b"x", 1, bytes(256), 256, out.ctypes.data) == -4     # DST_prime holds the length in one byte
    assert dll.nlx_bn254_hash_to_field(None, 0, None, 0, out.ctypes.data) == 0
    assert nlx.bn254_plonk.hash_to_field_native(b"", b"") == gm.hash_to_field(b"", b"")
