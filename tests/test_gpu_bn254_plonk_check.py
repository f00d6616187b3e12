"""GPU: nlx_bn254_plonk_check_witness (csrc/bn254_plonk_check.hip, near-light-client_amd/bn254_plonk.py check_resident; DESIGN.md
section 35) against the big-integer yardstick tests/bn254_plonk_check_model.py, which tests/test_bn254_plonk_check_model_cpu.py
pins to the frozen models.  Sizes where the kernels can go wrong: 2^3 (less than a wave), 2^6 (one wave), 2^7 (two waves), 2^9
(more than one 256-lane block), 2^10; keys with k = 0 (n_pi 0 and 3) and k = 1, 2 (n_pi 2), with and without the coset values."""
import ctypes

import numpy as np
import pytest

import bn254_plonk_check_model as model
from test_gpu_bn254_plonk_resident import _power_srs

pytestmark = pytest.mark.gpu

gm, bn, R = model.gm, model.bn, model.R
NLX_E_INVAL, NLX_E_RANGE = -1, -4
SIZES = [3, 6, 7, 9, 10]
SHAPES = [(0, 0), (0, 3), (1, 2), (2, 2)]   # (k, n_pi)
GATES, COPIES, COMMITS, ALL = model.CHECK_GATES, model.CHECK_COPIES, model.CHECK_COMMITS, model.CHECK_ALL


class Rig:
    """a case of the yardstick with its resident keys (made on first use, kept for the module)"""

    def __init__(self, nlx, ctx, case):
        self.nlx, self.ctx, self.case, self.keys = nlx, ctx, case, {}
        self.srs = nlx.bn254_g1_pack(_power_srs(case.tau, case.n + 3))

    def key(self, coset=False, values=None, k2=None):
        if values is not None or k2 is not None:
            return self.nlx.bn254_plonk.ResidentKey(self.ctx, values or self.case.values, self.srs, self.case.k1, k2 or self.case.k2,
                                                    commitments=self.case.info, coset=coset)
        if coset not in self.keys:
            self.keys[coset] = self.key(coset, values=self.case.values)
        return self.keys[coset]

    def check(self, wires=None, pubs=None, cblind=None, what=ALL, coset=False, key=None):
        c = self.case
        wires = c.wires if wires is None else wires
        return self.nlx.bn254_plonk.check_resident(key or self.key(coset), wires[0], wires[1], wires[2], c.pubs if pubs is None else pubs,
                                                   (c.cblind if cblind is None else cblind) if c.k else None, what)

    def proves(self, wires=None, pubs=None, cblind=None, coset=False):
        """does prove_resident accept the same arguments?  (-> the bytes, or None for ValueError)"""
        c = self.case
        wires = c.wires if wires is None else wires
        try:
            return self.nlx.bn254_plonk.prove_resident(self.key(coset), wires[0], wires[1], wires[2], c.pubs if pubs is None else pubs, c.blind,
                                                       (c.cblind if cblind is None else cblind) if c.k else None)
        except ValueError:
            return None


@pytest.fixture(scope="module")
def rigs(nlx, ctx):
    made = {}

    def get(log_n, k, n_pi):
        if (log_n, k, n_pi) not in made:
            made[log_n, k, n_pi] = Rig(nlx, ctx, model.Case(log_n, k, n_pi))
        return made[log_n, k, n_pi]
    yield get
    for rig in made.values():
        for key in rig.keys.values():
            key.close()


def _same(rep, want, n=None, cached=None):
    got = rep.as_dict()
    cache = got.pop("cache_bytes")
    assert got == want, {f: (got[f], want[f]) for f in want if got[f] != want[f]}
    if cached is not None:
        assert cache == (12 * n if cached else 0)
    assert bool(rep) == bool(want["satisfied"])
    if not want["satisfied"]:
        assert rep.message.startswith("the witness does not satisfy the circuit") and "\n" not in rep.message and str(rep) == rep.message
        with pytest.raises(ValueError):
            rep.raise_if_unsatisfied()


@pytest.mark.parametrize("coset", [False, True])
@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", SIZES)
def test_satisfied_witnesses(rigs, log_n, k, n_pi, coset):
    rig = rigs(log_n, k, n_pi)
    for what in (ALL, GATES, COPIES, GATES | COPIES, COMMITS, GATES | COMMITS):
        rep = rig.check(what=what, coset=coset)
        want = rig.case.check(what=what)
        assert rep.satisfied == 1 and rep.checked == (what if k else what & 3) and rep.raise_if_unsatisfied() is rep
        assert (rep.gate_rows_bad, rep.copy_cells_bad, rep.commits_bad) == (0, 0, 0)
        assert rep.gate_rows_skipped == (k if what & GATES and not what & COMMITS else 0)
        _same(rep, want)


def _low_free_row(case):
    """the lowest row without a role in a commitment that holds neither aimed cell"""
    return next(i for i in range(case.n) if i not in (case.gate_only[1], case.copy_only[1])
                and not any(i == c["row"] or i in c["committed"] for c in case.info))


def _aimed(case):
    """name -> (wires, pubs, cblind): single changes aimed at the kernels' edges and at each kind of finding"""
    n, w = case.n, case.wires
    bump = lambda c, i, d=1: model.mutated(case, (c, i, (w[c][i] + d) % R))
    out = {"l_row0": (bump(0, 0), None, None), "r_last_row": (bump(1, n - 1), None, None), "o_middle": (bump(2, n // 2), None, None),
           "l_last_row": (bump(0, n - 1), None, None), "o_row0": (bump(2, 0), None, None)}
    c, i = case.copy_only       # another value swapped in, nothing refitted: its row has qo = 0
    out["copy_no_gate"] = (model.mutated(case, (c, i, w[0][0] if w[0][0] != w[c][i] else 1)), None, None)
    c, i = case.gate_only       # the cell is its own cycle
    out["gate_no_copy"] = (bump(c, i), None, None)
    if case.n_pi:
        out["wrong_public_input"] = (None, [(case.pubs[0] + 1) % R] + case.pubs[1:], None)
        out["wrong_last_public_input"] = (None, case.pubs[:-1] + [(case.pubs[-1] + 5) % R], None)
    if case.k:
        out["committed_value_changed"] = (bump(0, case.info[0]["committed"][0]), None, None)
        out["wrong_commitment_row"] = (bump(0, case.info[-1]["row"]), None, None)
        out["wrong_commit_blinding"] = (None, None, [(x + 1) % R for x in case.cblind])
    # "first": two bad rows / two broken copies, the lower one is named
    two = bump(2, case.gate_only[1])
    lo = _low_free_row(case)
    two[2][lo] = (two[2][lo] + 1) % R
    out["two_bad_rows"] = (two, None, None)
    return out


def _run_case(rig, name, wires, pubs, cblind, coset):
    case = rig.case
    want = case.check(wires, pubs, cblind)
    assert want["satisfied"] == 0, name
    rep = rig.check(wires, pubs, cblind, coset=coset)
    _same(rep, want)
    # the contract: CHECK_ALL is satisfied exactly when the prover accepts the same arguments
    assert rig.proves(wires, pubs, cblind, coset=coset) is None, name
    return rep


@pytest.mark.parametrize("coset", [False, True])
@pytest.mark.parametrize("k,n_pi", SHAPES)
@pytest.mark.parametrize("log_n", SIZES)
def test_aimed_mutations_equal_the_yardstick_and_the_prover_refuses(rigs, log_n, k, n_pi, coset):
    rig = rigs(log_n, k, n_pi)
    case = rig.case
    seen = {}
    for name, (wires, pubs, cblind) in _aimed(case).items():
        seen[name] = _run_case(rig, name, wires, pubs, cblind, coset)
    rep = seen["copy_no_gate"]
    assert (rep.gate_rows_bad, rep.copy_cells_bad) == (0, 2) and "copy:" in rep.message
    rep = seen["gate_no_copy"]
    assert (rep.gate_rows_bad, rep.copy_cells_bad, rep.gate_row) == (1, 0, case.gate_only[1]) and "row %d:" % rep.gate_row in rep.message
    rep = seen["two_bad_rows"]
    assert (rep.gate_rows_bad, rep.gate_row) == (2, _low_free_row(case)) and _low_free_row(case) < case.gate_only[1]
    if case.n_pi:
        assert (seen["wrong_public_input"].gate_rows_bad, seen["wrong_public_input"].gate_row) == (1, 0)
    if k:
        assert seen["committed_value_changed"].commits_bad >= 1 and "Bsb22 commitment" in seen["committed_value_changed"].message
        rep = seen["wrong_commitment_row"]
        assert (rep.commits_bad, rep.commit_index, rep.commit_row) == (1, k - 1, case.info[-1]["row"])
        assert seen["wrong_commit_blinding"].commits_bad == k
    # and the good witness still proves: the bytes do not depend on the checks that ran in between
    assert rig.proves(coset=coset) is not None


def test_two_broken_copies_name_the_lower_cell(rigs):
    rig = rigs(7, 0, 0)
    case = rig.case
    cells = model.decode_sigma(case.values, case.k1, case.k2)

    def cycle(cell):
        out, at = [], cell
        while at not in out:
            out.append(at)
            at = cells[at[0]][at[1]]
        return out
    a = case.copy_only
    b = next((c, i) for i in range(case.n - 1, -1, -1) for c in range(3) if cells[c][i] != (c, i) and (c, i) not in cycle(a))
    wires = model.mutated(case, (a[0], a[1], 1))
    wires[b[0]][b[1]] = 2
    want = case.check(wires)
    rep = rig.check(wires)
    _same(rep, want)
    # each changed cell and the cell before it in its cycle
    bad = {a, cycle(a)[-1], b, cycle(b)[-1]}
    assert rep.copy_cells_bad == 4 and (rep.copy_row, rep.copy_wire) == min((i, c) for c, i in bad)
    assert rig.proves(wires) is None


@pytest.mark.parametrize("coset", [False, True])
def test_golden_mutations_equal_the_yardstick(rigs, coset):
    records = model.load_golden()
    assert len(records) == 40
    for g in records:
        rig = rigs(g["log_n"], g["k"], g["n_pi"])
        wires = model.mutated(rig.case, (g["wire"], g["row"], int(g["value"], 16)))
        want = {f: (int(v, 16) if isinstance(v, str) else v) for f, v in g["report"].items()}
        _same(rig.check(wires, coset=coset), want)
        assert rig.proves(wires, coset=coset) is None


@pytest.mark.parametrize("k,n_pi", [(0, 3), (2, 2)])
def test_proof_bytes_and_buffers_are_untouched(nlx, rigs, k, n_pi):
    import torch
    rig = rigs(9, k, n_pi)
    case = rig.case
    before = rig.proves()
    assert before is not None
    host = [list(c) for c in case.wires]
    dev = [torch.from_numpy(nlx.bn254_pack([[bn.to_montgomery(v) for v in c]])[0].view(np.int64)).cuda() for c in case.wires]
    kept = [d.clone() for d in dev]
    P = nlx.bn254_plonk
    cb = case.cblind if k else None
    bad = model.mutated(case, (1, 5, 12345))
    bad_dev = [d.clone() for d in dev]
    bad_dev[1][5] = torch.from_numpy(nlx.batch._fr_words(bn.to_montgomery(12345)).view(np.int64)).cuda()
    bad_kept = [d.clone() for d in bad_dev]
    for what in (ALL, GATES, COPIES):
        rep = P.check_resident(rig.key(), dev[0], dev[1], dev[2], case.pubs, cb, what)
        assert rep.satisfied == 1
        _same(P.check_resident(rig.key(), bad_dev[0], bad_dev[1], bad_dev[2], case.pubs, cb, what), case.check(bad, what=what))
    assert rig.proves(bad) is None
    with pytest.raises(ValueError):
        P.prove_resident(rig.key(), bad_dev[0], bad_dev[1], bad_dev[2], case.pubs, case.blind, cb)
    assert all(torch.equal(a, b) for a, b in zip(dev, kept)) and all(torch.equal(a, b) for a, b in zip(bad_dev, bad_kept))
    assert rig.check(host).satisfied == 1 and host == case.wires
    assert rig.proves() == before
    assert P.prove_resident(rig.key(), dev[0], dev[1], dev[2], case.pubs, case.blind, cb) == before
    if k:   # the callable form, driven through the hint as prove_resident drives it
        calls = []

        def witness(cs):
            calls.append(len(cs))
            return case.inst.complete(cs)
        rep = P.check_resident(rig.key(), public_inputs=case.pubs, commit_blinding=case.cblind, witness=witness)
        assert rep.satisfied == 1 and calls == list(range(k + 1))


@pytest.mark.parametrize("k,n_pi", [(0, 0), (1, 2)])
def test_cache(rigs, k, n_pi):
    rig = rigs(6, k, n_pi)
    case, n = rig.case, rig.case.n
    key = rig.key(values=case.values)     # a key of its own: nothing checked yet
    bad = model.mutated(case, (0, 3, 77))
    try:
        info = key.info()
        _same(rig.check(bad, what=GATES | COMMITS, key=key), case.check(bad, what=GATES | COMMITS), n, cached=False)
        _same(rig.check(what=GATES, key=key), case.check(what=GATES), n, cached=False)
        first = rig.check(bad, what=COPIES, key=key)
        _same(first, case.check(bad, what=COPIES), n, cached=True)
        again = rig.check(bad, what=COPIES, key=key)
        assert bytes(again) == bytes(first) and again.message == first.message
        _same(rig.check(bad, what=GATES, key=key), case.check(bad, what=GATES), n, cached=True)
        _same(rig.check(bad, key=key), case.check(bad), n, cached=True)
        assert rig.proves(bad) is None
        assert key.info() == info          # key_info keeps its five words
    finally:
        key.close()


@pytest.mark.parametrize("k,n_pi", [(0, 3), (1, 2)])
def test_a_later_gates_and_copies_check_takes_less_time_than_one_proof(nlx, rigs, k, n_pi):
    """The one condition the entry is held to, at the largest size of this file: wires on the device, the
    synchronous calls' wall time, the median of 5 after 2 warm-ups on a key that has been checked before."""
    import statistics
    import time

    import torch
    rig = rigs(10, k, n_pi)
    case, key, P = rig.case, rig.key(), nlx.bn254_plonk
    dev = [torch.from_numpy(nlx.bn254_pack([[bn.to_montgomery(v) for v in c]])[0].view(np.int64)).cuda() for c in case.wires]
    cb = case.cblind if k else None

    def median_ms(fn):
        times = []
        for i in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times[2:])
    check_ms = median_ms(lambda: P.check_resident(key, dev[0], dev[1], dev[2], case.pubs, cb, GATES | COPIES).raise_if_unsatisfied())
    prove_ms = median_ms(lambda: P.prove_resident(key, dev[0], dev[1], dev[2], case.pubs, case.blind, cb))
    print("2^10 gates, k = %d: a later gates | copies check %.3f ms, one proof %.3f ms" % (k, check_ms, prove_ms))
    assert check_ms < prove_ms


def _raw(nlx, ctx, key, wires, pubs, cblind, what, report=True, null=()):
    B = nlx.batch
    words = lambda xs: np.stack([B._fr_words(bn.to_montgomery(x) if x < R else x) for x in xs]) if xs is not None and len(xs) else None
    w = [nlx.bn254_pack([[bn.to_montgomery(v) for v in c]])[0] for c in wires]
    pw, cw = words(pubs), words(cblind)
    rep = nlx.bn254_plonk.WitnessReport()
    ctypes.memset(ctypes.byref(rep), 0xA5, ctypes.sizeof(rep))
    ptrs = [None if i in null else w[i].ctypes.data for i in range(3)]
    rc = nlx.lib.dll.nlx_bn254_plonk_check_witness(ctx.handle, None if "key" in null else key.handle, ptrs[0], ptrs[1], ptrs[2],
                                                   pw.ctypes.data if pw is not None else None, len(pubs or ()), cw.ctypes.data if cw is not None else None,
                                                   what, ctypes.byref(rep) if report else None)
    return rc, rep


def test_arguments(nlx, ctx, rigs):
    rig = rigs(6, 2, 2)
    case, n = rig.case, rig.case.n
    key = rig.key()
    last = lambda: nlx.lib.dll.nlx_last_error(ctx.handle).decode()
    zeroed = lambda rep: bytes(rep) == bytes(ctypes.sizeof(rep))
    assert ctypes.sizeof(nlx.bn254_plonk.WitnessReport) == 232
    rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, case.cblind, ALL)
    assert rc == 0 and rep.satisfied == 1 and rep.checked == 7 and rep.commit_pad_ == 0
    for null in ((0,), (1,), (2,), ("key",)):
        rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, case.cblind, ALL, null=null)
        assert rc == NLX_E_INVAL and zeroed(rep) and "NULL" in last()
    assert _raw(nlx, ctx, key, case.wires, case.pubs, case.cblind, ALL, report=False)[0] == NLX_E_INVAL
    for what in (0, 8, 15):
        rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, case.cblind, what)
        assert rc == NLX_E_INVAL and zeroed(rep) and "what" in last()
    rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, None, ALL)
    assert rc == NLX_E_INVAL and zeroed(rep) and "blinding" in last()
    rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, None, GATES | COPIES)       # no COMMITS: no blinding needed
    assert rc == 0 and rep.satisfied == 1 and rep.checked == 3 and rep.gate_rows_skipped == 2
    rc, rep = _raw(nlx, ctx, key, case.wires, [R, case.pubs[1]], case.cblind, ALL)
    assert rc == NLX_E_RANGE and zeroed(rep)
    rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, [R + 1] + case.cblind[1:], ALL)
    assert rc == NLX_E_RANGE and zeroed(rep)
    # a key without commitments drops COMMITS and wants no blinding
    plain = rigs(6, 0, 3)
    rc, rep = _raw(nlx, ctx, plain.key(), plain.case.wires, plain.case.pubs, None, ALL)
    assert rc == 0 and rep.satisfied == 1 and rep.checked == 3
    rc, rep = _raw(nlx, ctx, plain.key(), plain.case.wires, plain.case.pubs, None, COMMITS)
    assert rc == 0 and rep.satisfied == 1 and rep.checked == 0
    # a sigma entry outside the three cosets: NLX_E_INVAL with its position, nothing cached, the next good call works
    values = dict(case.values, s2=list(case.values["s2"]))
    values["s2"][41] = 7           # 7^n is none of 1, 5^n, 25^n at n = 64
    assert pow(7, n, R) not in (1, pow(5, n, R), pow(25, n, R))
    broken = rig.key(values=values)
    try:
        for _ in range(2):
            rc, rep = _raw(nlx, ctx, broken, case.wires, case.pubs, case.cblind, COPIES)
            assert rc == NLX_E_INVAL and zeroed(rep) and "s2" in last() and "row 41" in last()
        rc, rep = _raw(nlx, ctx, broken, case.wires, case.pubs, case.cblind, GATES | COMMITS)
        assert rc == 0 and rep.satisfied == 1 and rep.cache_bytes == 0
    finally:
        broken.close()
    # a key whose cosets coincide
    same = rig.key(k2=case.k1)
    try:
        rc, rep = _raw(nlx, ctx, same, case.wires, case.pubs, case.cblind, COPIES)
        assert rc == NLX_E_INVAL and zeroed(rep) and "k1^n" in last()
        rc, rep = _raw(nlx, ctx, same, case.wires, case.pubs, case.cblind, GATES | COMMITS)
        assert rc == 0 and rep.cache_bytes == 0
    finally:
        same.close()
    rc, rep = _raw(nlx, ctx, key, case.wires, case.pubs, case.cblind, ALL)
    assert rc == 0 and rep.satisfied == 1 and rep.cache_bytes == 12 * n
    with pytest.raises(ValueError):
        nlx.bn254_plonk.check_resident(key, case.wires[0], case.wires[1], case.wires[2], case.pubs, None, ALL)
    with pytest.raises(ValueError):
        nlx.bn254_plonk.check_resident(key, case.wires[0], case.wires[1], None, case.pubs, case.cblind)
