"""The three binding rounds called directly: nlx_sha256_bind_round and nlx_sha512_bind_round on the device trace of raw blocks
(tests/sha2_inputs.py) and nlx_ed25519_bind_round on a synthetic round-0 array equal the Python binding_columns in both columns,
exactly, and their totals equal the fingerprint - for gamma = 0, gamma = 1 and a gamma whose two words are at or above p."""
import numpy as np
import pytest

import sha2_inputs as inputs


def _bind_round(nlx, ctx, entry, trace, log_units, n, gamma):
    acc = np.full((2, n), 0xDEADDEADDEADDEAD, dtype=np.uint64)
    g, total = np.array(gamma, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    ctx.check(getattr(nlx._lib.dll, entry)(ctx.handle, trace.ctypes.data, log_units, g.ctypes.data, acc.ctypes.data, total.ctypes.data))
    return acc, (int(total[0]), int(total[1]))


def _compare(got, want, gamma):
    if not np.array_equal(got, want):
        col, row = np.argwhere(got != want)[0]
        pytest.fail("gamma %r: accumulator column %d differs first at row %d: %#x, expected %#x"
                    % (gamma, col, row, int(got[col, row]), int(want[col, row])))


@pytest.mark.gpu
@pytest.mark.parametrize("log_blocks", [0, 2, 7])
@pytest.mark.parametrize("name", ["sha256", "sha512"])
def test_sha2_bind_round_equals_binding_columns(nlx, ctx, name, log_blocks):
    mod = getattr(nlx, name + "_air")
    blocks, first = inputs.raw_blocks(32 if name == "sha256" else 64, log_blocks)
    trace, _ = inputs.device_trace(nlx, ctx, name, blocks, first, log_blocks)
    for gamma in inputs.GAMMAS:
        got, total = _bind_round(nlx, ctx, "nlx_%s_bind_round" % name, trace, log_blocks, 4 << log_blocks, gamma)
        want, want_total = mod.binding_columns(blocks, first, gamma)
        _compare(got, want, gamma)
        assert total == tuple(want_total) == mod.fingerprint(blocks, first, gamma), gamma


@pytest.mark.gpu
@pytest.mark.parametrize("log_slots", [0, 2])
def test_ed25519_bind_round_equals_binding_columns(nlx, ctx, log_slots):
    E = nlx.ed25519_air  # noqa: N806
    n = E.ROWS << log_slots
    rng = np.random.default_rng(25519 + log_slots)
    # E.N_COLS0 columns are what the entry reads (a prover's array goes on with multiplicity columns the entry never stages); only
    # what the fingerprint reads is filled
    t0 = np.zeros((E.N_COLS0, n), dtype=np.uint64)
    # the bound columns are per-slot columns (the AIR holds them constant over a slot's rows): the slot kernel reads them on the
    # slot's first row, the rows kernel and the Python reference on the row that absorbs them
    for base in (E.AY, E.RY, E.SW, E.DW, E.DW + 16):
        t0[base:base + 16] = np.repeat(rng.integers(0, 1 << 16, size=(16, 1 << log_slots), dtype=np.uint64), E.ROWS, axis=1)
    for col in (E.SGA, E.SGR, E.ACT):
        t0[col] = np.repeat(rng.integers(0, 2, size=1 << log_slots, dtype=np.uint64), E.ROWS)
    for gamma in inputs.GAMMAS:
        got, total = _bind_round(nlx, ctx, "nlx_ed25519_bind_round", t0, log_slots, n, gamma)
        want, want_total = E.binding_columns(t0, gamma)
        _compare(got, want, gamma)
        assert total == tuple(want_total), gamma
