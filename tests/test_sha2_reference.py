"""The plain-Python references of the two SHA-2 AIRs are pinned: what reference_trace and binding_columns compute on the inputs of
tests/sha2_inputs.py hashes to what tests/golden/sha2_reference_digests.json recorded (tests/golden/gen_sha2_reference_digests.py,
run on the commit named in the file).  The GPU tests compare the device against these references."""
import json
import os

import numpy as np
import pytest

import sha2_inputs as inputs
from conftest import P, ROOT


@pytest.mark.parametrize("name", ["sha256", "sha512"])
def test_reference_values_are_the_recorded_ones(nlx, name):
    with open(os.path.join(ROOT, "tests", "golden", "sha2_reference_digests.json")) as f:
        want = json.load(f)[name]
    got = inputs.reference_cases(getattr(nlx, name + "_air"), name)
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], case


@pytest.mark.parametrize("name", ["sha256", "sha512"])
def test_reference_reduces_gamma(nlx, name):
    """a gamma whose words are at or above p (what nlx_*_bind_round reduces on entry) gives the columns, the total and the
    fingerprint of its reduced form"""
    mod = getattr(nlx, name + "_air")
    blocks, first = inputs.raw_blocks(32 if name == "sha256" else 64, 2)
    gamma = inputs.GAMMAS[2]
    reduced = (gamma[0] % P, gamma[1] % P)
    assert min(gamma) >= P and reduced != gamma
    cols, total = mod.binding_columns(blocks, first, gamma)
    want_cols, want_total = mod.binding_columns(blocks, first, reduced)
    assert np.array_equal(cols, want_cols) and tuple(total) == tuple(want_total)
    assert mod.fingerprint(blocks, first, gamma) == mod.fingerprint(blocks, first, reduced) == tuple(total)
