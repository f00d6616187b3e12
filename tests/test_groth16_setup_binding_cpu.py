"""CPU: the Python side of the Groth16 setup (near-light-client_amd/bn254_groth16.py Trapdoor, Setup, _SetupDesc) before the library is
called: the descriptor's ctypes layout equals the C struct's (include/nlx.h, through the host compiler), the trapdoor's words, and
the shapes the binding refuses itself."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_setup_desc_layout_equals_the_header(nlx, tmp_path):
    g16 = nlx.bn254_groth16
    fields = [name for name, _ in g16._SetupDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlx.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(nlx_bn254_groth16_setup_desc, %s));\n' % f for f in fields)
                   + '    printf("%zu\\n", sizeof(nlx_bn254_groth16_setup_desc));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # the header is C
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(g16._SetupDesc, f).offset for f in fields] + [ctypes.sizeof(g16._SetupDesc)]
    assert (g16.SETUP_G1_A, g16.SETUP_INFINITY_A, g16.SETUP_IC, g16.SETUP_PEDERSEN_G_ROOT_SIGMA_NEG) == (0, 5, 15, 17)


def test_trapdoor(nlx):
    g16 = nlx.bn254_groth16
    R = g16.R
    a, b = g16.Trapdoor.random(), g16.Trapdoor.random()
    for td in (a, b):
        assert all(1 <= getattr(td, k) < R for k in ("tau", "alpha", "beta", "gamma", "delta", "sigma"))
    assert a.tau != b.tau and g16.Trapdoor(1, 2, 3, 4, 5).sigma is None
    assert not g16._trapdoor_words(0).any()
    assert g16.fr_unpack(g16._trapdoor_words(7)[None]) == [7]
    raw = g16._trapdoor_words(R)                                          # not a residue: the words go as they are, for the library to refuse
    assert sum(int(raw[w]) << (64 * w) for w in range(4)) == R
    with pytest.raises(nlx.NlxError):
        g16._trapdoor_words(1 << 256)


def test_shapes_the_binding_refuses(nlx):
    g16 = nlx.bn254_groth16
    td = g16.Trapdoor(2, 3, 4, 5, 6)
    coeffs = np.zeros((1, 4), dtype=np.uint64)
    for row_ptr, wire, coeff_id in (([0, 1, 4], [0, 1, 2], [0, 0, 0]), ([0, 1, 3], [0, 1, 2], [0, 0]), ([0, 1, 2, 3], [0, 1, 2], [0, 0, 0])):
        m = (np.asarray(row_ptr, dtype=np.uint64), np.asarray(wire, dtype=np.uint32), np.asarray(coeff_id, dtype=np.uint32))
        with pytest.raises(ValueError, match="matrix A"):
            g16.Setup(None, 1, 3, 1, 2, {"A": m, "B": m, "C": m, "coeffs": coeffs}, td)
    m = (np.array([0, 1, 3], dtype=np.uint64), np.array([0, 1, 2], dtype=np.uint32), np.zeros(3, dtype=np.uint32))
    with pytest.raises(ValueError, match="sigma"):
        g16.Setup(None, 1, 3, 1, 2, {"A": m, "B": m, "C": m, "coeffs": coeffs}, td, commitments=[dict(private=[1], public=[0], wire=2)])
    with pytest.raises(ValueError):
        g16.Setup(None, 1, 3, 1, 2, {"A": m, "B": m, "C": m, "coeffs": np.zeros((1, 5), dtype=np.uint64)}, td)
