"""GPU: gnark's plonk.Setup on the device (nlx_bn254_plonk_setup, _setup_read, _setup_key, _setup_wires, nlx_bn254_kzg_srs;
csrc/bn254_plonk_setup.hip, near-light-client_amd/bn254_plonk.py Setup / kzg_srs) against the big-integer
model tools/gnark_plonk_setup_model.py on the circuits of tests/bn254_plonk_setup_cases.py, which
tests/test_gnark_plonk_setup_model_cpu.py pins to the frozen models.  Every comparison is exact.  Parity with gnark-produced
keys stays unpinned."""
import ctypes
import random

import numpy as np
import pytest

import bn254_plonk_check_model as check_model
import bn254_plonk_setup_cases as cases

pytestmark = pytest.mark.gpu

gm, bn, R, sm = check_model.gm, check_model.bn, check_model.R, cases.sm
E_INVAL, E_RANGE = -1, -4
ACCEPT, ALGEBRAIC = 0, 4
VK_ORDER = ("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk")


@pytest.fixture(scope="module")
def setups(nlx, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = nlx.bn254_plonk.Setup(ctx, **cases.case(name).args())
        return made[name]
    yield get
    for s in made.values():
        s.close()


def _mont_words(nlx, values):
    return nlx.bn254_pack([[bn.to_montgomery(v) for v in values]])[0]


def _ints(nlx, tensor):
    """an (n, 4) device tensor of fr.Element words as integers"""
    words = tensor.cpu().numpy().view(np.uint64)
    return [nlx.bn254_plonk._from_words_mont(w) for w in words]


def _verdict(v):
    return int(v.accepted), int(v.reason), int(v.index)


def _flat(cells):
    return cells[0] + cells[1] + cells[2]


# ---- the arrays ----
@pytest.mark.parametrize("name", cases.SMALL)
def test_every_array_equals_the_models(nlx, setups, name):
    c, s = cases.case(name), setups(name)
    m = c.model()
    where = m.classes()
    assert s.info() == {"n": m.n, "log_n": m.log_n, "k": c.k, "rows_used": m.used, "variables_used": len(where),
                        "longest_class": max(len(p) for p in where.values())}
    got = s.values()
    assert sorted(got) == sorted(m.values)
    for key, want in m.values.items():
        assert got[key] == want, key
    assert s.read("cells").tolist() == _flat(m.cells)
    assert s.read("permutation").tolist() == m.perm
    assert s.read("sigma_cells").tolist() == m.sigma_cells()
    assert s.commitment_info() == m.info
    assert np.array_equal(s.read("s2", device="cuda:0").cpu().numpy().view(np.uint64), s.read("s2"))
    assert s.read("permutation", device="cuda:0").cpu().tolist() == m.perm
    with pytest.raises(nlx.NlxError) as e:
        s.read("qcp%d" % c.k)
    assert e.value.code == E_RANGE and "unknown array" in str(e.value)


def test_worked_case_and_the_smallest_domain(nlx, ctx):
    P = nlx.bn254_plonk
    w = cases.worked_case()
    s = P.Setup(ctx, 4, 1, [(1, 2, 3, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0)], [0, 1, R - 1])      # log_n = 0: three rows -> 2^3
    assert s.log_n == 3 and s.read("permutation").tolist() == w.perm
    assert all(s.read("permutation")[p] == q for p, q in cases.WORKED_PERM.items())
    s.close()
    c = cases.case("n1000_k1")
    s = P.Setup(ctx, **dict(c.args(), log_n=0))
    assert s.info()["log_n"] == 10
    s.close()
    s = P.Setup(ctx, 1, 0, [], [])                       # no row at all: padding only, one class of 24 cells
    assert s.info() == {"n": 8, "log_n": 3, "k": 0, "rows_used": 0, "variables_used": 1, "longest_class": 24}
    assert s.read("permutation").tolist() == [23] + list(range(23))
    s.close()


def test_2_14_rows_above_the_table_split(nlx, setups):
    c, s = cases.case("s14"), setups("s14")
    m = c.model()
    assert s.read("permutation").tolist() == m.perm
    assert s.read("sigma_cells").tolist() == m.sigma_cells()
    for name in ("s1", "s2", "s3"):
        assert np.array_equal(s.read(name), _mont_words(nlx, m.values[name])), name
    assert np.array_equal(s.read("ql")[:5], _mont_words(nlx, m.values["ql"][:5]))


def test_2_16_more_variables_than_one_digit_pass(nlx, setups):
    c, s = cases.case("s16"), setups("s16")
    m = sm.Setup(c.n_variables, c.n_public, c.constraints, c.coeffs, c.k1, c.k2, c.sets, c.log_n, with_sigma=False)
    perm = s.read("permutation").tolist()
    assert perm == m.perm
    rng = random.Random(16)
    sigma = [s.read(name) for name in ("s1", "s2", "s3")]
    for p in [0, m.n - 1, 3 * m.n - 1] + [rng.randrange(3 * m.n) for _ in range(61)]:
        want = sm.sigma_value(m.perm[p], m.log_n, c.k1, c.k2)
        assert np.array_equal(sigma[p // m.n][p % m.n], _mont_words(nlx, [want])[0]), p
    assert s.info()["variables_used"] == len(m.classes())


# ---- the key ----
@pytest.mark.parametrize("name", ["n32_k2", "n1000_k1"])
def test_key_commitments_equal_the_models_through_the_trapdoor(nlx, ctx, setups, name):
    P = nlx.bn254_plonk
    c, s = cases.case(name), setups(name)
    m = c.model()
    tau = random.Random(name).randrange(1, R)
    g1, _, _ = P.kzg_srs(ctx, tau, m.n + 3, device="cuda:0")
    key = s.key(g1)
    names = list(VK_ORDER) + ["qcp%d" % j for j in range(c.k)]
    want = [bn.g1_mul(bn.eval_poly(bn.ntt(m.values[x], inverse=True), tau), bn.G1) for x in names]
    assert np.array_equal(key.key_commitments(), nlx.bn254_g1_pack(want))
    assert key.info()["n"] == m.n and key.info()["k"] == c.k and key.bsb22 == m.info and key.proof_bytes == 552 + 64 * c.k
    key.close()


@pytest.mark.parametrize("coset", [False, True])
@pytest.mark.parametrize("name", ["n256", "n1000_k1"])
def test_proof_bytes_equal_a_key_from_the_models_host_values(nlx, ctx, setups, name, coset):
    """k = 0 and k = 1: the same witness and blinding on the setup's key and on a ResidentKey built the old way"""
    P = nlx.bn254_plonk
    c, s = cases.case(name), setups(name)
    m = c.model()
    rng = random.Random(name + str(coset))
    tau = rng.randrange(1, R)
    blind, cblind = [rng.randrange(R) for _ in range(9)], [rng.randrange(R) for _ in range(2 * c.k)]
    g1, _, _ = P.kzg_srs(ctx, tau, m.n + 3)
    key = s.key(g1, coset=coset)
    old = P.ResidentKey(ctx, m.values, g1, c.k1, c.k2, commitments=m.info, coset=coset)
    assert key.info() == old.info()
    assert np.array_equal(key.key_commitments(), old.key_commitments())
    witness = lambda cs: m.wires(c.complete(cs))
    got = P.prove_resident(key, public_inputs=c.public_inputs, blinding=blind, commit_blinding=cblind, witness=witness)
    want = P.prove_resident(old, public_inputs=c.public_inputs, blinding=blind, commit_blinding=cblind, witness=witness)
    assert got == want and len(got) == 552 + 64 * c.k
    key.close()
    old.close()


@pytest.mark.parametrize("name", ["n1024", "n1000_k1", "n4096"])
def test_end_to_end_on_the_device(nlx, ctx, name):
    """kzg_srs -> setup -> key -> wires(values) -> prove_resident -> VerifyingKey.from_resident(..).verify.  The rejections: a
    changed public input changes gamma and PI(zeta), a foreign key changes the digests the transcript binds - either way the
    algebraic relation fails before any pairing, the verdict tests/test_gpu_bn254_plonk_verify.py sees for a changed input."""
    P = nlx.bn254_plonk
    c = cases.case(name)
    rng = random.Random(name)
    tau = rng.randrange(1, R)
    g1, g2, g2_tau = P.kzg_srs(ctx, tau, c.n + 3, device="cuda:0")
    key, s = P.setup(ctx, c.n_variables, c.n_public, c.constraints, c.coeffs, g1, commitments=c.sets)
    assert s.log_n == c.log_n
    pubs = c.public_inputs
    if c.k:
        def witness(cs):
            return tuple(_ints(nlx, t) for t in s.wires(c.complete(cs)))
        proof = P.prove_resident(key, public_inputs=pubs, witness=witness)
    else:
        l, r, o = s.wires(c.complete())
        proof = P.prove_resident(key, l, r, o, pubs)
    vk = P.VerifyingKey.from_resident(key, g2, g2_tau, c.n_public)
    assert _verdict(vk.verify(proof, pubs)) == (1, ACCEPT, 0)
    assert _verdict(vk.verify(proof, [(pubs[0] + 1) % R] + pubs[1:])) == (0, ALGEBRAIC, 0)
    foreign_constraints, _ = cases.one_cell_changed(c)
    key2, s2 = P.setup(ctx, c.n_variables, c.n_public, foreign_constraints, c.coeffs, g1, commitments=c.sets)
    vk2 = P.VerifyingKey.from_resident(key2, g2, g2_tau, c.n_public)
    assert not np.array_equal(key2.key_commitments()[:3], key.key_commitments()[:3])
    assert np.array_equal(key2.key_commitments()[3:], key.key_commitments()[3:])        # one cell: only the permutation differs
    assert _verdict(vk2.verify(proof, pubs)) == (0, ALGEBRAIC, 0)
    for x in (vk, vk2, key, key2, s, s2):
        x.close()


# ---- the witness checker on the setup's key ----
@pytest.mark.parametrize("name", ["n256", "n1000_k1"])
def test_check_resident_on_the_setups_key(nlx, ctx, setups, name):
    P = nlx.bn254_plonk
    c, s = cases.case(name), setups(name)
    m = c.model()
    rng = random.Random("check" + name)
    tau = rng.randrange(1, R)
    cblind = [rng.randrange(R) for _ in range(2 * c.k)]
    (l, r, o), _, _, _, cs = gm.solve(cases.AsInstance(c), None, cblind, tau)
    g1, _, _ = P.kzg_srs(ctx, tau, m.n + 3)
    ctx.kernel_timing(True)
    key = s.key(g1)
    rep = P.check_resident(key, l, r, o, c.public_inputs, cblind if c.k else None)
    assert rep.satisfied == 1 and rep.checked == (7 if c.k else 3)
    assert rep.cache_bytes == 12 * m.n                                    # on the FIRST report: the cells came with the key
    # one cell changed: the copy the checker names is the model's permutation (this pins the direction)
    p = next(p for p in range(m.n, 3 * m.n) if m.perm[p] != p and m.perm[p] != m.perm.index(p))      # a class of three or more
    bad = [list(col) for col in (l, r, o)]
    bad[p // m.n][p % m.n] = (bad[p // m.n][p % m.n] + 1) % R
    rep = P.check_resident(key, bad[0], bad[1], bad[2], c.public_inputs, what=check_model.CHECK_COPIES)
    want = check_model.check(m.values, bad[0], bad[1], bad[2], c.public_inputs, None, m.info, c.k1, c.k2, what=check_model.CHECK_COPIES)
    got = rep.as_dict()
    assert got.pop("cache_bytes") == 12 * m.n and got == want
    at = rep.copy_wire * m.n + rep.copy_row
    assert rep.copy_cells_bad == 2 and rep.copy_to_wire * m.n + rep.copy_to_row == m.perm[at]
    assert ctx.kernel_stats("bn254_plonk_sigma_decode")[0] == 0 and ctx.kernel_stats("bn254_plonk_check_copies")[0] == 2
    # the same wires on a key_create key: the same reports, apart from that history
    old = P.ResidentKey(ctx, m.values, g1, c.k1, c.k2, commitments=m.info)
    rep2 = P.check_resident(old, bad[0], bad[1], bad[2], c.public_inputs, what=check_model.CHECK_COPIES)
    got2 = rep2.as_dict()
    assert got2.pop("cache_bytes") == 12 * m.n and got2 == want and rep2.message == rep.message
    assert ctx.kernel_stats("bn254_plonk_sigma_decode")[0] == 1           # that key had to decode
    rep3 = P.check_resident(old, l, r, o, c.public_inputs, cblind if c.k else None)
    assert rep3.satisfied == 1
    ctx.kernel_timing(False)
    key.close()
    old.close()


# ---- the gather ----
@pytest.mark.parametrize("name", ["n32_k2", "n256"])
def test_wires_equal_the_models_gather(nlx, ctx, setups, name):
    import torch
    c, s = cases.case(name), setups(name)
    m = c.model()
    values = c.complete([11 + j for j in range(c.k)])
    want = [_mont_words(nlx, col) for col in m.wires(values)]
    words = _mont_words(nlx, values)
    dev = torch.from_numpy(words.view(np.int64)).to("cuda:0")
    for source in (values, words, dev):
        got = s.wires(source)
        for col in range(3):
            assert np.array_equal(got[col].cpu().numpy().view(np.uint64), want[col]), col
    with pytest.raises(ValueError):
        s.wires(values[:-1])


# ---- the SRS ----
def test_kzg_srs_equals_the_models(nlx, ctx):
    P = nlx.bn254_plonk
    tau = random.Random(5).randrange(1, R)
    _, want_g2, want_g2_tau = sm.kzg_srs(tau, 1)
    for n in (1, 2, 3, 259):
        g1, g2, g2_tau = P.kzg_srs(ctx, tau, n)
        assert np.array_equal(g1, nlx.bn254_g1_pack(bn.kzg_srs(tau, n))), n
        assert np.array_equal(g2, nlx.bn254_g2_pack([want_g2])[0]) and np.array_equal(g2_tau, nlx.bn254_g2_pack([want_g2_tau])[0])
    n = (1 << 16) + 3
    g1, _, _ = P.kzg_srs(ctx, tau, n, device="cuda:0")
    g1 = g1.cpu().numpy().view(np.uint64)
    rng = random.Random(6)
    for i in [0, 1, n - 1, 1 << 16] + [rng.randrange(n) for _ in range(12)]:
        assert np.array_equal(g1[i], nlx.bn254_g1_pack([bn.g1_mul(pow(tau, i, R), bn.G1)])[0]), i
    g1, g2, g2_tau = P.kzg_srs(ctx, 1, 70)
    assert np.array_equal(g1, np.repeat(nlx.bn254_g1_pack([bn.G1]), 70, axis=0)) and np.array_equal(g2, g2_tau)


# ---- refusals: the stated code, the cause and the index named, nothing left allocated ----
def _refused(nlx, ctx, code, needle, **args):
    before = ctx.memory()[1]
    with pytest.raises(nlx.NlxError) as e:
        nlx.bn254_plonk.Setup(ctx, **args)
    assert e.value.code == code and needle in str(e.value), str(e.value)
    assert ctx.memory()[1] == before


def test_setup_refusals(nlx, ctx):
    c = cases.case("n32_k2")
    base = c.args()
    cons = c.constraints
    edit = lambda i, at, v: cons[:i] + [cons[i][:at] + (v,) + cons[i][at + 1:]] + cons[i + 1:]
    rng = lambda needle, **over: _refused(nlx, ctx, E_RANGE, needle, **dict(base, **over))
    rng("flags", flags=0)
    rng("flags", flags=3)
    rng("log_n", log_n=2)
    rng("log_n", log_n=27)
    rng("log_n = 4 is too small", log_n=4)
    rng("n_variables = 0", n_variables=0)
    rng("n_variables = 1", n_variables=1)                                 # below n_public = 2
    rng("constraint 3, xb: variable %d of %d" % (c.n_variables, c.n_variables), constraints=edit(3, 1, c.n_variables))
    rng("constraint 0, xa: variable", constraints=edit(0, 0, c.n_variables + 5))
    rng("constraint 25, xc: variable", constraints=edit(25, 2, 0xFFFFFFFF))
    rng("constraint 2, qm: coefficient %d of %d" % (len(c.coeffs), len(c.coeffs)), constraints=edit(2, 5, len(c.coeffs)))
    rng("constraint 7, qk: coefficient", constraints=edit(7, 7, len(c.coeffs)))
    rng("coefficient 1 is not below r", coeffs=[c.coeffs[0], R] + c.coeffs[2:])
    rng("k1 is not below r", k1=R)
    rng("k2 is not below r", k2=R + 1)
    rng("coset_shift is not below r", coset_shift=(1 << 256) - 1)
    sets = lambda j, **over: [dict(x, **over) if i == j else x for i, x in enumerate(c.sets)]
    rng("n_commit", commitments=c.sets * 3)
    rng("commitment 1: committed constraint %d of %d" % (len(cons), len(cons)), commitments=sets(1, committed=[3, len(cons)]))
    rng("commitment 0: its constraint %d of %d" % (len(cons), len(cons)), commitments=sets(0, constraint=len(cons)))
    rng("commitment 1: the committed constraints do not ascend at 4", commitments=sets(1, committed=[2, 4, 4]))
    rng("commitment 0: the committed constraints do not ascend at 1", commitments=sets(0, committed=[5, 1]))
    big = cases.case("n1000_k1")
    _refused(nlx, ctx, E_RANGE, "log_n = 9 is too small", **dict(big.args(), log_n=9))


def test_null_arguments_and_wires_and_srs_refusals(nlx, ctx):
    P, dll = nlx.bn254_plonk, nlx.lib.dll
    one = np.zeros(1, dtype=np.uint32)
    coeffs = np.zeros((1, 4), dtype=np.uint64)
    scalars = [P._element_words(x) for x in (5, 25, 5)]

    def desc(**over):
        d = P._PlonkSetupDesc()
        d.log_n, d.flags, d.n_variables, d.n_public, d.n_constraints, d.n_coeffs = 3, 1, 2, 1, 1, 1
        for name in ("xa", "xb", "xc", "ql", "qr", "qm", "qo", "qk"):
            setattr(d, name, one.ctypes.data)
        d.coeffs = coeffs.ctypes.data
        d.k1, d.k2, d.coset_shift = (x.ctypes.data for x in scalars)
        for name, v in over.items():
            setattr(d, name, v)
        return d

    def call(d, code, needle):
        before = ctx.memory()[1]
        h = ctypes.c_void_p()
        assert dll.nlx_bn254_plonk_setup(ctx.handle, ctypes.byref(d), ctypes.byref(h)) == code and not h.value
        assert needle in dll.nlx_last_error(ctx.handle).decode(), dll.nlx_last_error(ctx.handle).decode()
        assert ctx.memory()[1] == before

    for name in ("xa", "xc", "ql", "qk", "coeffs", "k1", "coset_shift"):
        call(desc(**{name: None}), E_INVAL, name)
    call(desc(n_commit=1), E_INVAL, "n_committed")
    h = ctypes.c_void_p()
    assert dll.nlx_bn254_plonk_setup(ctx.handle, None, ctypes.byref(h)) == E_INVAL
    assert dll.nlx_bn254_plonk_setup(ctx.handle, ctypes.byref(desc()), ctypes.byref(h)) == 0 and h.value       # the descriptor itself is fine
    before = ctx.memory()[1]
    out = np.zeros((3, 8, 4), dtype=np.uint64)
    assert dll.nlx_bn254_plonk_setup_wires(ctx.handle, h, None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data) == E_INVAL
    assert dll.nlx_bn254_plonk_setup_wires(ctx.handle, h, coeffs.ctypes.data, None, out[1].ctypes.data, out[2].ctypes.data) == E_INVAL
    key = ctypes.c_void_p()
    small = np.zeros((10, 8), dtype=np.uint64)
    assert dll.nlx_bn254_plonk_setup_key(h, small.ctypes.data, 10, 0, ctypes.byref(key)) == E_RANGE and not key.value      # n + 3 = 11 points
    assert dll.nlx_bn254_plonk_setup_key(h, small.ctypes.data, 11, 2, ctypes.byref(key)) == E_RANGE
    assert ctx.memory()[1] == before
    dll.nlx_bn254_plonk_setup_destroy(h)
    # the SRS
    g1, g2 = np.zeros((4, 8), dtype=np.uint64), np.zeros((2, 16), dtype=np.uint64)
    for tau, n, code, needle in ((0, 4, E_RANGE, "tau is zero"), (R, 4, E_RANGE, "not below r"), (7, 0, E_RANGE, "n = 0"),
                                 (7, (1 << 27) + 1, E_RANGE, "2^27"), (None, 4, E_INVAL, "NULL")):
        before = ctx.memory()[1]
        t = P._element_words(tau) if tau is not None else None
        assert dll.nlx_bn254_kzg_srs(ctx.handle, t.ctypes.data if t is not None else None, n, g1.ctypes.data, g2.ctypes.data) == code
        assert needle in dll.nlx_last_error(ctx.handle).decode() and ctx.memory()[1] == before and not g1.any()
    assert dll.nlx_bn254_kzg_srs(ctx.handle, P._element_words(7).ctypes.data, 4, None, None) == E_INVAL
