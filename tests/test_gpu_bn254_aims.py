"""GPU: the BN254 scalar-field chain (csrc/bn254_plonk.hip, csrc/bn254.hip) and the nine-limb field under it (csrc/bn254_f29.hpp)
on the aimed inputs of tests/bn254_aims.py, every comparison exact and against Python integers (oracle/bn254_py.py and the models
in bn254_aims - never device output against device output):

  * nlx_bn254_f29_ops: every function of the header at the operands of the host check, both moduli, and x32;
  * nlx_bn254_plonk_grand_product at the sizes where its launches change, with zero denominators and numerators (1 / 0 := 0), at
    challenges 0, 1, r - 1, and its refusal of challenges that are not residues;
  * nlx_bn254_plonk_quotient with chosen values at chosen points of the coset (tests/test_bn254_aims_cpu.py proves they are there);
  * nlx_bn254_kzg_open, nlx_bn254_fr_lincomb, nlx_bn254_groth16_quotient and the NTT at edge values and at the sizes whose
    paths no other test runs (2^11: the tiled reordering with m = 1; 2^14, 2^15: the coset power table past hi[1])."""
import ctypes
import random

import numpy as np
import pytest

import bn254_aims as aims

pytestmark = pytest.mark.gpu

bn = aims.bn
R = aims.R
SHIFT, K1, K2 = 5, 5, 25
NLX_E_RANGE = -4
EDGE = (0, 1, R - 1)


# ---- the field functions on the device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f29_cases():
    return aims.f29_cases(random.Random(29))


def _f29_run(nlx, ctx, cases):
    """cases of one modulus -> per case (value, limbs normalised) of the case's own function"""
    a = np.array([aims.to_limbs(c[2]) for c in cases], dtype=np.uint32)
    b = np.array([aims.to_limbs(c[3]) for c in cases], dtype=np.uint32)
    out = nlx.bn254_f29_ops(ctx, cases[0][0], a, b)
    assert out.shape == (len(cases), len(nlx.BN254_F29_OPS), 9)
    return [aims.from_limbs(out[i, nlx.BN254_F29_OPS.index(c[1])]) for i, c in enumerate(cases)]


@pytest.mark.parametrize("modulus", ["q", "r"])
def test_f29_field_code_on_the_device(nlx, ctx, f29_cases, modulus):
    """the host check's cases and assertions (tests/test_bn254_model.py) on the device: value, bound and limb normalisation of
    every function, at 1, 63, 64, 65 cases and the full list (one lane per case, blocks of 64)"""
    cases = [c for c in f29_cases if c[0] == modulus]
    assert len(cases) >= 2000 and (modulus == "q" or sum(c[1] == "x32" for c in cases) >= 5)
    for count in (1, 63, 64, 65, len(cases)):
        for case, (got, normalised) in zip(cases[-count:], _f29_run(nlx, ctx, cases[-count:])):
            aims.f29_check(case, got, normalised)
        if count < len(cases):                   # and from the front of the list: other functions on the first lanes
            for case, (got, normalised) in zip(cases[:count], _f29_run(nlx, ctx, cases[:count])):
                aims.f29_check(case, got, normalised)
    assert nlx.bn254_f29_ops(ctx, modulus, np.zeros((0, 9), np.uint32), np.zeros((0, 9), np.uint32)).shape[0] == 0
    one = np.zeros((1, 9), np.uint32)
    assert nlx.lib.dll.nlx_bn254_f29_ops(ctx.handle, 2, one.ctypes.data, one.ctypes.data, 1, np.zeros(99, np.uint32).ctypes.data) == NLX_E_RANGE


# ---- the grand product --------------------------------------------------------------------------------------------------------------
_witnesses = {}


def _witness(log_n):
    """one satisfying witness per size, computed once and left unchanged: (p, beta, gamma)"""
    if log_n not in _witnesses:
        rng = random.Random(500 + log_n)
        beta, gamma = rng.randrange(R), rng.randrange(R)
        _witnesses[log_n] = (bn.plonk_witness(log_n, rng, K1, K2, beta, gamma), beta, gamma)
    return _witnesses[log_n]


def _grand_product(nlx, ctx, p, beta, gamma):
    n = len(p["l"])
    z = np.zeros((n, 4), dtype=np.uint64)
    closes = nlx.bn254_plonk.grand_product(ctx, n.bit_length() - 1, *[aims.pack_mont(p[k]) for k in ("l", "r", "o", "s1", "s2", "s3")],
                                           beta, gamma, K1, K2, z)
    return aims.unpack_mont(z), closes


def _assert_gp(nlx, ctx, p, beta, gamma, what):
    want_z, want_closes = aims.grand_product_model(p, beta, gamma, K1, K2)
    z, closes = _grand_product(nlx, ctx, p, beta, gamma)
    diff = [i for i in range(len(z)) if z[i] != want_z[i]]
    print("%s: first differing row %s of %d, closes %s (model %s)" % (what, diff[0] if diff else None, len(z), closes, want_closes))
    assert not diff, "%s: z differs from the model first in row %d (%d rows differ)" % (what, diff[0], len(diff))
    assert closes == want_closes, what
    return want_z, want_closes


@pytest.mark.parametrize("log_n", [1, 2, 6, 7, 12, 13])
def test_grand_product_sizes(nlx, ctx, log_n):
    """below one run of 64 rows, exactly one run, two runs, one full block of 64 runs (two scan levels), two blocks (three scan
    levels): z and closes equal the row formula on a satisfying witness and with s1 / s2 swapped"""
    p, beta, gamma = _witness(log_n)
    z, closes = _assert_gp(nlx, ctx, p, beta, gamma, "2^%d" % log_n)
    assert closes and z == p["z"]
    _, closes = _assert_gp(nlx, ctx, dict(p, s1=p["s2"], s2=p["s1"]), beta, gamma, "2^%d, s1 / s2 swapped" % log_n)
    assert not closes


@pytest.mark.parametrize("log_n", [7, 13])
def test_grand_product_zero_denominators_and_numerators(nlx, ctx, log_n):
    """1 / 0 := 0: a row whose denominator vanishes gives the ratio 0 and leaves every other row of its run exact; z equals the
    model in every row and the product does not close"""
    p, beta, gamma = _witness(log_n)
    for name, q, den_rows, num_rows in aims.gp_zero_cases(p, beta, gamma, K1, K2):
        z, closes = _assert_gp(nlx, ctx, q, beta, gamma, "2^%d, %s (denominator 0 in rows %s, numerator 0 in rows %s)" % (log_n, name, den_rows, num_rows))
        first = min(den_rows + num_rows)
        assert not closes and all(z[:first + 1]) and not any(z[first + 1:])


@pytest.mark.parametrize("beta", EDGE)
@pytest.mark.parametrize("gamma", [0, R - 1])
def test_grand_product_edge_challenges(nlx, ctx, beta, gamma):
    """beta in {0, 1, r - 1}, gamma in {0, r - 1} on wires that hold 0, 1 and r - 1: with beta = gamma = 0 a zero wire is a zero
    denominator (and numerator); with beta = 0 every other ratio is 1"""
    p, _, _ = _witness(7)
    q = dict(p, l=list(p["l"]), r=list(p["r"]), o=list(p["o"]))
    q["l"][5], q["r"][70], q["o"][127] = 0, 0, 0
    q["l"][9], q["r"][9], q["o"][9] = 1, R - 1, 1
    q["r"][64] = 1
    if beta == 0 and gamma == 0:
        assert aims.gp_factors(q, 5, pow(bn.root_of_unity(7), 5, R), beta, gamma, K1, K2) == (0, 0)
    _assert_gp(nlx, ctx, q, beta, gamma, "beta %s gamma %s" % (beta if beta < 2 else "r-1", gamma if gamma < 2 else "r-1"))


def test_grand_product_refuses_challenges_that_are_not_residues(nlx, ctx):
    """a challenge or shift not below r is no fr.Element: NLX_E_RANGE, as the quotient chain answers; the context works afterwards"""
    p, beta, gamma = _witness(2)
    arrays = [aims.pack_mont(p[k]) for k in ("l", "r", "o", "s1", "s2", "s3")]
    good = [aims.pack([bn.to_montgomery(x)])[0] for x in (beta, gamma, K1, K2)]
    z = np.zeros((4, 4), dtype=np.uint64)
    closes = ctypes.c_int32(-7)
    call = lambda sc: nlx.lib.dll.nlx_bn254_plonk_grand_product(ctx.handle, 2, *[a.ctypes.data for a in arrays], *[s.ctypes.data for s in sc],   # noqa: E731
                                                                z.ctypes.data, ctypes.byref(closes))
    for pos in range(4):
        for bad in (R, R + 3, (1 << 256) - 1):
            sc = list(good)
            sc[pos] = aims.pack([bad])[0]
            assert call(sc) == NLX_E_RANGE and closes.value == -7 and not z.any()
    assert call(good) == 0 and closes.value == 1 and aims.unpack_mont(z) == p["z"]


# ---- the quotient at aimed points ------------------------------------------------------------------------------------------------------
def _quotient(nlx, ctx, on_h, variant, sc, blinding):
    packed = {name: aims.pack_mont(v) for name, v in on_h.items() if name in aims.THIRTEEN}
    kw = {}
    if variant == "blinded":
        kw["blinding"] = [bn.to_montgomery(x) for x in blinding]
    if variant == "commit":
        kw.update(qcp=[aims.pack_mont(on_h["qcp0"])], pi2=[aims.pack_mont(on_h["pi20"])])
    t, ok = nlx.bn254_plonk_quotient(ctx, packed, *[bn.to_montgomery(x) for x in sc], **kw)
    return aims.unpack_mont(t.reshape(-1, 4)), ok


def _assert_quotient(nlx, ctx, aim, variant, c, log_n, alpha, beta, gamma, blinding):
    on_h, _, k0 = aims.quotient_inputs(aim, variant, c, log_n, SHIFT, K1, K2, beta, gamma)
    want, want_ok = aims.quotient_model(on_h, variant, 1 << log_n, SHIFT, K1, K2, alpha, beta, gamma, blinding)
    got, ok = _quotient(nlx, ctx, on_h, variant, (SHIFT, K1, K2, alpha, beta, gamma), blinding)
    assert got == want, (aim, variant, c, k0)
    assert ok == want_ok, (aim, variant, c, k0)


@pytest.mark.parametrize("variant", ["plain", "pi", "blinded", "commit"])
@pytest.mark.parametrize("log_n", [3, 6])
def test_quotient_at_aimed_points(nlx, ctx, log_n, variant):
    """every aim at one position of every class of the 4n coset (the other positions hold the aimed words in rotation): t and
    high_chunk_is_zero equal the model the existing test of the variant uses.  The aimed witnesses do not satisfy the circuit."""
    rng = random.Random(600 + log_n)
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    blinding = [rng.randrange(R) for _ in range(9)]
    for c in range(4):
        for aim in aims.QUOTIENT_AIMS:
            _assert_quotient(nlx, ctx, aim, variant, c, log_n, alpha, beta, gamma, blinding)


@pytest.mark.parametrize("alpha", EDGE)
@pytest.mark.parametrize("log_n", [3, 6])
def test_quotient_edge_challenges(nlx, ctx, log_n, alpha):
    """alpha, beta, gamma each in {0, 1, r - 1}, the aim and the class moving with the combination"""
    j = 0
    for beta in EDGE:
        for gamma in EDGE:
            aim = aims.QUOTIENT_AIMS[(3 * j + EDGE.index(alpha)) % len(aims.QUOTIENT_AIMS)]
            _assert_quotient(nlx, ctx, aim, "pi" if j % 2 else "plain", j % 4, log_n, alpha, beta, gamma, None)
            j += 1


# ---- KZG opening and linear combination ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 64, 65, 4097])
def test_kzg_open_edge_points_and_coefficients(nlx, ctx, m):
    """zeta in {0, 1, r - 1, a root}; coefficients all words r - 1, all values r - 1 (p(-1) = 0 for even m: a root), all 0, only
    the top one non-zero (0 is a root)"""
    rng = random.Random(700 + m)
    root = rng.randrange(2, R)
    q = [rng.randrange(R) for _ in range(m - 1)]
    with_root = [(a - root * b) % R for a, b in zip([0] + q, q + [0])]          # (X - root) q(X)
    polys = {"words r-1": [aims.V_RM1] * m, "values r-1": [R - 1] * m, "zero": [0] * m, "top only": [0] * (m - 1) + [R - 1], "with a root": with_root}
    roots = 0
    for name, coeffs in polys.items():
        words = aims.pack_mont(coeffs)
        for zeta in EDGE + (root,):
            want_y, want_q = bn.kzg_open(coeffs, zeta)
            y, quot, _ = nlx.bn254_kzg_open(ctx, words, bn.to_montgomery(zeta))
            assert aims.unpack_mont(y[None]) == [want_y], (name, zeta)
            assert aims.unpack_mont(quot) == want_q, (name, zeta)
            roots += want_y == 0 and any(coeffs)
    assert aims.unpack_mont(aims.pack_mont(with_root)) == with_root and bn.kzg_open(with_root, root) == (0, q)
    assert roots >= (3 if m % 2 == 0 else 2)


@pytest.mark.parametrize("m", [1, 257])
def test_lincomb_sixteen_terms_of_r_minus_one(nlx, ctx, m):
    """the largest sum the accumulator meets: 16 terms, every scalar and every element r - 1 (as words and as values)"""
    for v in (aims.V_RM1, R - 1):
        polys = [aims.pack_mont([v] * m) for _ in range(16)]
        out = np.zeros((m, 4), dtype=np.uint64)
        nlx.bn254_plonk.lincomb(ctx, polys, [v] * 16, out)
        assert aims.unpack_mont(out) == [16 * v * v % R] * m
    cols = [[aims.aim_value(t + i) for i in range(m)] for t in range(16)]
    scal = [aims.aim_value(3 * t) for t in range(16)]
    out = np.zeros((m, 4), dtype=np.uint64)
    nlx.bn254_plonk.lincomb(ctx, [aims.pack_mont(c) for c in cols], scal, out)
    assert aims.unpack_mont(out) == [sum(s * c[i] for s, c in zip(scal, cols)) % R for i in range(m)]


# ---- Groth16's quotient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 9])
def test_groth16_quotient_edge_values(nlx, ctx, log_n):
    n = 1 << log_n
    for v in (R - 1, aims.V_RM1):
        for name, (a, b, c) in {"a = b = r-1, c free": ([v] * n, [v] * n, [aims.aim_value(i) for i in range(n)]),
                                "c = a b: every numerator zero": ([v] * n, [v] * n, [v * v % R] * n),
                                "a = 0, c all r-1": ([0] * n, [v] * n, [v] * n)}.items():
            want = bn.groth16_quotient(a, b, c)
            got = aims.unpack_mont(nlx.bn254_plonk.groth16_quotient(ctx, aims.pack_mont(a), aims.pack_mont(b), aims.pack_mont(c)))
            assert got == want, name
            assert any(want) == ("numerator zero" not in name)


# ---- the NTT at the sizes and values no other test reaches ---------------------------------------------------------------------------------
def _bitrev(v):
    n = len(v)
    bits = n.bit_length() - 1
    return [v[int(format(i, "0%db" % bits)[::-1], 2)] for i in range(n)] if bits else list(v)


@pytest.mark.parametrize("shift_kind", ["5", "random"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [11, 14, 15])
def test_ntt_on_cosets_at_edge_columns(nlx, ctx, log_n, inverse, shift_kind):
    """forward and inverse on the coset of 5 and of a random shift, in both decimations (DIF: bit-reversed out, DIT: bit-reversed
    in) and both element forms, against the recursive big-integer transform.  The transform is linear, so the same integer
    columns serve both forms (as canonical integers and as Montgomery words, the shift in the form of the data)."""
    rng = random.Random(800 + log_n)
    n = 1 << log_n
    shift = 5 if shift_kind == "5" else rng.randrange(2, R)
    single = [0] * n
    single[(4096 + 1) % n] = 1
    cols = [[R - 1] * n, [0] * n, single, [aims.WORD_AIMS[i % 10][1] for i in range(n)]]
    want = []
    for col in cols:
        if not any(col):
            want.append(col)
        elif not inverse:
            s, scaled = 1, []
            for v in col:
                scaled.append(v * s % R)
                s = s * shift % R
            want.append(bn.ntt(scaled))
        else:
            sinv, s, out = pow(shift, R - 2, R), 1, []
            for v in bn.ntt(col, inverse=True):
                out.append(v * s % R)
                s = s * sinv % R
            want.append(out)
    natural = np.stack([aims.pack(col) for col in cols])
    reversed_in = np.stack([aims.pack(_bitrev(col)) for col in cols])
    for montgomery in (False, True):
        sh = bn.to_montgomery(shift) if montgomery else shift
        dif = nlx.bn254_ntt(ctx, natural, inverse=inverse, montgomery=montgomery, coset_shift=sh, bitrev_out=True)
        dit = nlx.bn254_ntt(ctx, reversed_in, inverse=inverse, montgomery=montgomery, coset_shift=sh, bitrev_in=True)
        for j in range(len(cols)):
            assert aims.unpack(dit[j]) == want[j], (j, montgomery, "DIT")
            assert _bitrev(aims.unpack(dif[j])) == want[j], (j, montgomery, "DIF")
