"""nlx_sha256_trace / nlx_sha512_trace on raw blocks (tests/sha2_inputs.py): the device trace equals reference_trace bit for bit
and the device digest the reference's final chaining value, at one block (row 0's schedule looks back into its own block), at
four, and at 128 blocks = 512 rows - two workgroups of the trace kernel and two of the chain kernel."""
import numpy as np
import pytest

import sha2_inputs as inputs


@pytest.mark.gpu
@pytest.mark.parametrize("log_blocks,flags", [(0, "mixed"), (2, "mixed"), (7, "mixed"), (7, "ones"), (7, "zeros")])
@pytest.mark.parametrize("name", ["sha256", "sha512"])
def test_device_trace_equals_reference(nlx, ctx, name, log_blocks, flags):
    mod, blocks, first, want, hout = inputs.reference(nlx, name, log_blocks, flags)
    got, digest = inputs.device_trace(nlx, ctx, name, blocks, first, log_blocks)
    assert got.shape == want.shape == (mod.N_COLS, 4 << log_blocks)
    if not np.array_equal(got, want):
        col, row = np.argwhere(got != want)[0]
        pytest.fail("%s trace differs from the reference first at column %d row %d: %#x, expected %#x"
                    % (name, col, row, int(got[col, row]), int(want[col, row])))
    assert digest.tolist() == hout.tolist()
