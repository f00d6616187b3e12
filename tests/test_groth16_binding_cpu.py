"""CPU: the Groth16 binding refuses buffers of the wrong shape before the library sees them (near-light-client_amd/bn254_groth16.py) - the
library reads what the descriptor's counts say and cannot see where a caller's buffer ends.  Numpy arrays and tensors alike."""
import numpy as np
import pytest


def test_buffers_of_the_wrong_shape_raise(nlx):
    import torch
    buf = nlx.bn254_groth16._buf
    good = np.zeros((5, 8), dtype=np.uint64)
    assert buf(good, np.uint64, 8)[2] == 5 and buf(torch.zeros((5, 8), dtype=torch.int64), np.uint64, 8)[2] == 5
    assert buf(np.zeros(8, dtype=np.uint64), np.uint64, size=8)[2] == 8 and buf(None, np.uint64, 8) == (None, None, 0)
    for make in (lambda shape: np.zeros(shape, dtype=np.uint64), lambda shape: torch.zeros(shape, dtype=torch.int64)):
        with pytest.raises(ValueError):
            buf(make((5, 8)), np.uint64, 16)          # a G1 array where G2 points are expected
        with pytest.raises(ValueError):
            buf(make((20,)), np.uint64, 4)            # a flat witness
        with pytest.raises(ValueError):
            buf(make((5, 4)), np.uint64, 0)           # a matrix where a one-dimensional array is expected
        with pytest.raises(ValueError):
            buf(make((16,)), np.uint64, size=8)       # sixteen words where a G1 point is expected
    with pytest.raises(TypeError):
        buf(torch.zeros((5, 4), dtype=torch.int32), np.uint64, 4)
    with pytest.raises(TypeError):
        buf(torch.zeros((5, 4), dtype=torch.float64), np.uint64, 4)
    with pytest.raises(TypeError):
        buf(torch.zeros((4, 5), dtype=torch.int64).t(), np.uint64, 4)   # not contiguous


def _key_args(row_ptr, wire, coeff_id, n_constraints=2, n_wires=3):
    """ProvingKey's arguments for a key of two constraints on three wires whose three matrices are (row_ptr, wire, coeff_id)"""
    g1, g2 = np.zeros((n_wires, 8), dtype=np.uint64), np.zeros((n_wires, 16), dtype=np.uint64)
    mask, p1, p2 = np.zeros(n_wires, dtype=np.uint8), np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    m = (np.asarray(row_ptr, dtype=np.uint64), np.asarray(wire, dtype=np.uint32), np.asarray(coeff_id, dtype=np.uint32))
    r1cs = {"A": m, "B": m, "C": m, "coeffs": np.zeros((1, 4), dtype=np.uint64)}
    return (1, n_wires, 1, n_constraints, g1, g1, g2, g1[1:], g1[:1], mask, mask, p1, p1, p1, p2, p2), r1cs


def test_row_pointers_that_disagree_with_the_terms_raise(nlx):
    """the library finds a matrix's number of terms in row_ptr's last entry: the binding refuses a row_ptr that ends past the
    wire / coeff_id arrays, or has another length than n_constraints + 1, before the library is called (ctx is never touched)"""
    Key = nlx.bn254_groth16.ProvingKey
    for row_ptr, wire, coeff_id in (([0, 1, 4], [0, 1, 2], [0, 0, 0]),      # ends at 4, three terms
                                    ([0, 1, 3], [0, 1, 2], [0, 0]),         # wire and coeff_id of different lengths
                                    ([0, 1, 2, 3], [0, 1, 2], [0, 0, 0]),   # three rows' offsets for two constraints
                                    ([0, 3], [0, 1, 2], [0, 0, 0])):        # one row's offsets for two constraints
        args, r1cs = _key_args(row_ptr, wire, coeff_id)
        with pytest.raises(ValueError, match="matrix A"):
            Key(None, *args, r1cs=r1cs)
    import torch
    args, r1cs = _key_args([0, 1, 4], [0, 1, 2], [0, 0, 0])
    r1cs["A"] = tuple(torch.from_numpy(a.astype(np.int64 if a.dtype == np.uint64 else np.int32)) for a in r1cs["A"])
    with pytest.raises(ValueError, match="row_ptr ends at 4"):
        Key(None, *args, r1cs=r1cs)
