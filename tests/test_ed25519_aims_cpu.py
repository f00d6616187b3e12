"""CPU tests on the aimed Ed25519 slots (tests/ed25519_aims.py): the aims hit what they claim; the row code the GPU runs, built
for the host under the address and undefined-behaviour sanitizers, equals the Python reference at every list size and refuses
every false statement; fe25519_fast.hpp (the scan's arithmetic, host and device) function by function against Python integers
at the edges of p and of its limb bounds.  The device side of the same checks is tests/test_gpu_ed25519_aims.py."""
import os
import subprocess

import numpy as np
import pytest

import ed25519_aims as aims
from conftest import ROOT
from test_ed25519_air import slot_line

P = aims.P


def build_native(tmp_path_factory, name):
    """tests/native/<name>.cpp as a stand-alone program under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "near-light-client_amd", "csrc"), os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def edcheck(tmp_path_factory):
    return build_native(tmp_path_factory, "ed25519_host_check")


@pytest.fixture(scope="module")
def fecheck(tmp_path_factory):
    return build_native(tmp_path_factory, "fe25519_fast_check")


def test_the_aims_hit_what_they_claim(nlx):
    E = nlx.ed25519_air
    sl = aims.slots(nlx)
    assert len(sl) == 16 and [len(names) for _, _, names in aims.SIZES] == [1, 2, 4, 8, 16, 32, 1]
    # the lists end on an active slot (1, 16) and on an inactive one (2, 4, 8): row 0 of slot 0 sees both flags of its predecessor
    assert [sl[names[-1]][6] for _, _, names in aims.SIZES[:5]] == [1, 0, 0, 0, 1]
    for name, s in sl.items():
        assert (name.startswith("off_") or name == "idle") == (s[6] == 0), name
    rows = {n: aims.reference_rows(nlx, n) for n in aims.ORDER}     # an active slot that is not a true statement raises here
    idle = rows["idle"]
    assert not idle[E.SIN:E.SIN + 16].any() and np.array_equal(idle[E.SIN + 16:E.SIN + 32], idle[E.SIN + 32:E.SIN + 48])
    assert not idle[E.SB].any() and not idle[E.HB].any()
    assert not rows["s_zero"][E.SB].any() and rows["s_zero"][E.HB].any() and sl["s_zero"][4] == 0
    for n in ("h_zero", "d_zero", "off_zero_pt_hzero"):
        assert not rows[n][E.HB].any() and rows[n][E.SB].any(), n
    ext = rows["off_extremes"]
    assert int(ext[E.AY + 15, 0]) == 0x7FFF and int(ext[E.SGA, 0]) == 1 and int(ext[E.QW + 16, 0]) != 0
    assert not rows["d_zero"][E.DW:E.DW + 32].any() and (rows["d_max"][E.DW:E.DW + 32] == 0xFFFF).all()
    assert sl["s_lm1"][4] == E.L_ORDER - 1 and sl["r_identity"][2:4] == (0, 1) and sl["a_identity"][:2] == (0, 1)
    assert sl["a_order2"][:2] == (0, P - 1) and sl["a_order2"][5] % E.L_ORDER % 2 == 0
    # S and h are below L < 2^253: rows 0 .. 2 (bits 255 .. 253) hold the pair (0, 0) in every slot, and bit 252 is set only in
    # a scalar within 2^125 of L.  So "a slot's first row" is row 3 for S (S = L - 1 sets it, nothing aimed at sets h's) and all
    # four pairs can first occur on row 4 (bit 251), the first bit free in both scalars; the last row is bit 0.
    pairs = {r: {(int(t[E.SB, r]), int(t[E.HB, r])) for t in rows.values()} for r in (0, 1, 2, 3, 4, E.ROWS - 1)}
    assert pairs[0] == pairs[1] == pairs[2] == {(0, 0)}
    assert pairs[3] == {(0, 0), (1, 0)}
    assert pairs[4] == pairs[E.ROWS - 1] == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the false statements have no witness, and the reference says so
    for what, replaced, reported in aims.false_statements(nlx):
        assert reported == min(replaced)
        for bad in replaced.values():
            with pytest.raises(AssertionError):
                E.reference_slot(*bad)


def test_reference_cache_hands_out_copies(nlx):
    """the list at 2^5 holds every slot twice, behind two different predecessors: their row 0 differs, the rest does not"""
    E = nlx.ed25519_air
    _, _, names = aims.SIZES[5]
    t = aims.reference(nlx, names)
    k0, k1 = 1, 30                                            # off_extremes behind random0 and behind s_zero
    assert names[k0] == names[k1] == "off_extremes" and names[k0 - 1] != names[k1 - 1]
    a, b = t[:, 256 * k0:256 * k0 + 256], t[:, 256 * k1:256 * k1 + 256]
    assert np.array_equal(a[:, 1:], b[:, 1:]) and not np.array_equal(a[E.AUX_B:E.AUX_B + 16, 0], b[E.AUX_B:E.AUX_B + 16, 0])
    assert np.array_equal(t[:, :256 * 16][:, 256:], aims.reference(nlx, aims.ORDER)[:, 256:])


@pytest.mark.parametrize("label,log_slots,names", aims.SIZES, ids=[s[0] for s in aims.SIZES])
def test_host_row_code_equals_reference(nlx, edcheck, tmp_path, label, log_slots, names):
    E = nlx.ed25519_air
    want = aims.reference(nlx, names)
    out = str(tmp_path / "trace.bin")
    text = "\n".join(slot_line(s) for s in aims.slot_list(nlx, names)) + "\n"
    subprocess.run([edcheck, out], input=text, text=True, check=True)
    got = np.fromfile(out, dtype=np.uint64).reshape(E.N_COLS0, -1)
    diff = aims.first_difference(nlx, got, want, names)
    assert diff is None, "host-built row code differs from the reference at " + diff


def test_host_row_code_refuses_every_false_statement(nlx, edcheck, tmp_path):
    for what, replaced, _ in aims.false_statements(nlx):
        text = "\n".join(slot_line(s) for s in aims.with_replaced(nlx, replaced)) + "\n"
        assert subprocess.run([edcheck, str(tmp_path / "bad.bin")], input=text, text=True).returncode == 5, what


def run_fe(fecheck, lines):
    r = subprocess.run([fecheck], input="\n".join(lines) + "\n", text=True, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def fe_line(*values):
    return " ".join(str(x) for v in values for x in v)


def test_fe25519_freeze_against_integers(fecheck):
    ops = aims.freeze_operands()
    assert len(ops) >= 7 * 41 * 2
    for v, got in zip(ops, run_fe(fecheck, ["F " + fe_line(v) for v in ops])):
        assert int(got[0], 16) == aims.value(v) % P, v


def test_fe25519_mul_against_integers_and_its_limb_bound(fecheck):
    ops = aims.mul_operands()
    for (a, b), got in zip(ops, run_fe(fecheck, ["M " + fe_line(a, b) for a, b in ops])):
        limbs = [int(x) for x in got[:10]]
        want = aims.value(a) * aims.value(b) % P
        assert int(got[10], 16) == want and aims.value(limbs) % P == want, (a, b)
        aims.assert_mul_limbs_in_bound(limbs, (a, b))


def test_fe25519_from_limbs16_against_integers(fecheck):
    ops = aims.from_limbs16_operands()
    for x, got in zip(ops, run_fe(fecheck, ["L %064x" % x for x in ops])):
        limbs = [int(v) for v in got]
        assert len(limbs) == 10 and all(0 <= v < (1 << 26) for v in limbs) and aims.value(limbs) == x, hex(x)


def test_fe25519_sums_against_integers(fecheck):
    ops = aims.sum_operands()
    for (a, b, c, d), got in zip(ops, run_fe(fecheck, ["S " + fe_line(a, b, c, d) for a, b, c, d in ops])):
        want = ([w + x + y + z for w, x, y, z in zip(a, b, c, d)], [w - x - y - z for w, x, y, z in zip(a, b, c, d)],
                [2 * (w + x) for w, x in zip(a, b)], [-(w + x) - (y + z) for w, x, y, z in zip(a, b, c, d)])
        assert len(got) == 44
        for k, limbs in enumerate(want):
            assert [int(v) for v in got[11 * k:11 * k + 10]] == limbs and max(abs(v) for v in limbs) <= aims.B28
            assert int(got[11 * k + 10], 16) == aims.value(limbs) % P, (k, a, b, c, d)
