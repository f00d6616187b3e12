"""Row f.4: a whole (unblinded) PLONK proof over BN254 on the GPU, assembled from the C-ABI pieces - the host-side mirror of
what gnark's backend/plonk/bn254 `Prove` orchestrates for the recursive wrap (Go, not in /root/reference; succinct.json:7-8
names the entry point that runs it).  The five rounds of the published protocol (Gabizon-Williamson-Ciobotaru), each round's
heavy step one library call on device-resident polynomials:

  1. [a] [b] [c]                      FFTInverse (nlx_bn254_ntt_batch) + three MSMs (nlx_bn254_msm_g1)
  2. beta, gamma -> z, [z]            nlx_bn254_plonk_grand_product + FFTInverse + MSM
  3. alpha -> t, [t_lo] [t_mid] [t_hi]  nlx_bn254_plonk_quotient + three MSMs
  4. zeta -> six evaluations          nlx_bn254_kzg_open (value only)
  5. v -> [W_zeta], [W_zeta_omega]    nlx_bn254_fr_lincomb (the linearisation polynomial and the batch in ONE combination of
                                      fifteen polynomials), nlx_bn254_kzg_open twice (synthetic division + MSM)

What this is not: gnark's byte format, blinding, its fiat-shamir labels (the transcript below is this repo's own SHA-256
chain) or the wrapper circuit - a maintainer wires the same calls into gnark's rounds.  Parity: the
proof's nine points and six scalars equal the big-integer model's (oracle/bn254_py.py plonk_prove_model) and the model's
verifier accepts them (tests/test_gpu_bn254_plonk.py)."""
import ctypes
import hashlib

import numpy as np

from . import batch as B

R = B.BN254_R
_MONT = (1 << 256) % R
_MONT_INV = pow(_MONT, R - 2, R)


def _to_mont(x):
    return int(x) * _MONT % R


def _from_words_mont(w):
    return sum(int(w[k]) << (64 * k) for k in range(4)) * _MONT_INV % R


def root_of_unity(log_n):
    return pow(pow(5, (R - 1) >> 28, R), 1 << (28 - log_n), R)


class Transcript:
    """SHA-256 chain over 32-byte big-endian integers; a challenge is the chain value mod r (this repo's convention)."""

    def __init__(self, label=b"nlx-plonk-bn254"):
        self.state = hashlib.sha256(label).digest()

    def absorb_int(self, x):
        self.state = hashlib.sha256(self.state + int(x).to_bytes(32, "big")).digest()

    def absorb_point(self, words):
        pt = B.bn254_g1_unpack(words)
        x, y = (0, 0) if pt is None else pt
        self.absorb_int(x)
        self.absorb_int(y)

    def challenge(self, label):
        self.state = hashlib.sha256(self.state + label).digest()
        return int.from_bytes(self.state, "big") % R


class ProvingKey:
    """The preprocessed circuit on the device: the eight fixed polynomials by values on H and by coefficients, their
    commitments, the SRS.  Everything is fr.Element / G1Affine words (Montgomery) in torch int64 tensors."""

    NAMES = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")

    def __init__(self, ctx, values, srs, k1, k2, device="cuda:0", commitments=()):
        """values: dict name -> n integers (canonical, values on H); srs: (>= n, 8) G1Affine words (array or device tensor).
        commitments: one dict per Bsb22 commitment, in commitment order - "committed": the rows whose L wire it covers, "row":
        its commitment row i_j, "last_row": the key-wide second blinding row (gnark: the last constraint) - with the selector
        of commitment j as values["qcp<j>"] (1 on the committed rows, 0 elsewhere).  The selectors are kept like the other fixed
        polynomials: qcp_values, qcp_coeffs (k, n, 4) and qcp_commitments.  Two names that must not be confused: the
        parameter `commitments` describes the circuit's Bsb22 commitments and is kept as self.bsb22; the attribute
        self.commitments is, as before, the dict of the fixed polynomials' KZG commitments by name."""
        import torch
        self.ctx, self.device = ctx, device
        self.n = len(values["ql"])
        self.log_n = self.n.bit_length() - 1
        self.k1, self.k2 = int(k1), int(k2)
        self.srs = srs if hasattr(srs, "data_ptr") else torch.from_numpy(np.ascontiguousarray(srs, dtype=np.uint64).view(np.int64)).to(device)
        packed = B.bn254_pack([[_to_mont(x) for x in values[k]] for k in self.NAMES])
        self.values = torch.from_numpy(packed.view(np.int64)).to(device)                      # (8, n, 4)
        self.coeffs = B.bn254_ntt(ctx, self.values.clone(), inverse=True, montgomery=True)     # in place on the clone
        self.commitments = {k: B.bn254_msm_g1(ctx, self.srs[:self.n], self.coeffs[i], montgomery=True) for i, k in enumerate(self.NAMES)}
        self.bsb22 = [{"committed": sorted(int(i) for i in c["committed"]), "row": int(c["row"]), "last_row": int(c["last_row"])} for c in commitments]
        self.qcp_values = self.qcp_coeffs = None
        self.qcp_commitments = []
        if self.bsb22:
            if len(self.bsb22) > 4:
                raise ValueError("at most four Bsb22 commitments")
            qcp = []
            for j, c in enumerate(self.bsb22):
                q = [int(x) % R for x in values["qcp%d" % j]]
                qcp.append(q)
                if c["last_row"] != self.bsb22[0]["last_row"] or not all(0 <= i < self.n for i in c["committed"] + [c["row"], c["last_row"]]):
                    raise ValueError("commitment %d: rows outside H, or a last_row that differs from the key's" % j)
                if len(q) != self.n or [i for i in range(self.n) if q[i]] != c["committed"] or any(q[i] != 1 for i in c["committed"]):
                    raise ValueError("qcp%d is not 1 on the committed rows and 0 elsewhere" % j)
            packed = B.bn254_pack([[_to_mont(x) for x in q] for q in qcp])
            self.qcp_values = torch.from_numpy(packed.view(np.int64)).to(device)              # (k, n, 4)
            self.qcp_coeffs = B.bn254_ntt(ctx, self.qcp_values.clone(), inverse=True, montgomery=True)
            self.qcp_commitments = [B.bn254_msm_g1(ctx, self.srs[:self.n], self.qcp_coeffs[j], montgomery=True) for j in range(len(self.bsb22))]

    def value(self, name):
        return self.values[self.NAMES.index(name)]

    def coeff(self, name):
        return self.coeffs[self.NAMES.index(name)]


def prove(pk, l, r, o, public_inputs=()):
    """l, r, o: the wire values on H - n canonical integers each, or (n, 4) device tensors of fr.Element words (Montgomery).
    Returns the proof: nine G1Affine word arrays and six integers, under the keys of the model's proof dict.
    This is the UNBLINDED paper-shaped proof under this repo's own transcript; it has no public-input polynomial - a statement
    with public inputs is proved with prove_gnark (gnark's transcript, blinding, batched opening and byte format)."""
    import torch
    if len(public_inputs):
        raise ValueError("prove() constrains no public inputs (it has no public-input polynomial): use prove_gnark")
    ctx, n, log_n = pk.ctx, pk.n, pk.log_n
    w = root_of_unity(log_n)
    commit = lambda c: B.bn254_msm_g1(ctx, pk.srs[:c.shape[0]], c, montgomery=True)
    tr = Transcript()
    tr.absorb_int(n)
    for x in public_inputs:
        tr.absorb_int(x)
    for k in pk.NAMES:
        tr.absorb_point(pk.commitments[k])
    # round 1
    if hasattr(l, "data_ptr"):   # already fr.Element words on the device: (n, 4) tensors
        wires = torch.stack([l, r, o])
    else:
        wires = torch.from_numpy(B.bn254_pack([[_to_mont(x) for x in col] for col in (l, r, o)]).view(np.int64)).to(pk.device)   # (3, n, 4)
    wire_coeffs = B.bn254_ntt(ctx, wires.clone(), inverse=True, montgomery=True)
    proof = {"a": commit(wire_coeffs[0]), "b": commit(wire_coeffs[1]), "c": commit(wire_coeffs[2])}
    for k in "abc":
        tr.absorb_point(proof[k])
    beta, gamma = tr.challenge(b"beta"), tr.challenge(b"gamma")
    # round 2
    z = torch.empty((n, 4), dtype=torch.int64, device=pk.device)
    if not grand_product(ctx, log_n, wires[0], wires[1], wires[2], pk.value("s1"), pk.value("s2"), pk.value("s3"), beta, gamma, pk.k1, pk.k2, z):
        raise ValueError("the wires do not respect the circuit's copy constraints (the grand product does not close)")
    z_coeffs = B.bn254_ntt(ctx, z.clone().reshape(1, n, 4), inverse=True, montgomery=True)[0]
    proof["z"] = commit(z_coeffs)
    tr.absorb_point(proof["z"])
    alpha = tr.challenge(b"alpha")
    # round 3
    polys = {k: pk.value(k) for k in pk.NAMES}
    polys.update(l=wires[0], r=wires[1], o=wires[2], z=z)
    t = torch.empty((3, n, 4), dtype=torch.int64, device=pk.device)
    _, ok = B.bn254_plonk_quotient(ctx, polys, *[_to_mont(x) for x in (pk.k1, pk.k1, pk.k2, alpha, beta, gamma)], out=t)
    if not ok:
        raise ValueError("the witness does not satisfy the circuit (the quotient has a fourth chunk)")
    for i, name in enumerate(("t_lo", "t_mid", "t_hi")):
        proof[name] = commit(t[i])
        tr.absorb_point(proof[name])
    zeta = tr.challenge(b"zeta")
    # round 4
    at = lambda c, point: _from_words_mont(B.bn254_kzg_open(ctx, c, _to_mont(point), want_quotient=False)[0])
    ev = {"a": at(wire_coeffs[0], zeta), "b": at(wire_coeffs[1], zeta), "c": at(wire_coeffs[2], zeta),
          "s1": at(pk.coeff("s1"), zeta), "s2": at(pk.coeff("s2"), zeta), "zw": at(z_coeffs, zeta * w % R)}
    for k in ("a", "b", "c", "s1", "s2", "zw"):
        tr.absorb_int(ev[k])
    v = tr.challenge(b"v")
    # round 5: F = r + v a + v^2 b + v^3 c + v^4 s1 + v^5 s2 as ONE combination; its opening at zeta is W_zeta
    sc = linearisation_scalars(ev, n, zeta, alpha, beta, gamma, pk.k1, pk.k2, v)
    terms = {"qm": pk.coeff("qm"), "ql": pk.coeff("ql"), "qr": pk.coeff("qr"), "qo": pk.coeff("qo"), "qk": pk.coeff("qk"), "z": z_coeffs,
             "s3": pk.coeff("s3"), "t_lo": t[0], "t_mid": t[1], "t_hi": t[2], "a": wire_coeffs[0], "b": wire_coeffs[1], "c": wire_coeffs[2],
             "s1": pk.coeff("s1"), "s2": pk.coeff("s2")}
    f = torch.empty((n, 4), dtype=torch.int64, device=pk.device)
    lincomb(ctx, [terms[k] for k in sc], [sc[k] for k in sc], f)
    proof["w_zeta"] = B.bn254_kzg_open(ctx, f, _to_mont(zeta), srs=pk.srs, want_quotient=False)[2]
    proof["w_zeta_omega"] = B.bn254_kzg_open(ctx, z_coeffs, _to_mont(zeta * w % R), srs=pk.srs, want_quotient=False)[2]
    proof["evals"] = ev
    return proof


def linearisation_scalars(ev, n, zeta, alpha, beta, gamma, k1, k2, v):
    """coefficients of the fifteen polynomials in F(X) (the published round 5, constants dropped: they do not reach a quotient)"""
    zh = (pow(zeta, n, R) - 1) % R
    l1 = zh * pow(n * (zeta - 1) % R, R - 2, R) % R
    a, b, c, s1, s2, zw = (ev[k] for k in ("a", "b", "c", "s1", "s2", "zw"))
    zn = pow(zeta, n, R)
    return {"qm": a * b % R, "ql": a, "qr": b, "qo": c, "qk": 1,
            "z": (alpha * (a + beta * zeta + gamma) % R * (b + beta * k1 * zeta + gamma) % R * (c + beta * k2 * zeta + gamma) + alpha * alpha % R * l1) % R,
            "s3": (-alpha * (a + beta * s1 + gamma) % R * (b + beta * s2 + gamma) % R * beta % R * zw) % R,
            "t_lo": (-zh) % R, "t_mid": (-zh * zn) % R, "t_hi": (-zh * zn % R * zn) % R,
            "a": v, "b": v * v % R, "c": pow(v, 3, R), "s1": pow(v, 4, R), "s2": pow(v, 5, R)}


def grand_product(ctx, log_n, l, r, o, s1, s2, s3, beta, gamma, k1, k2, z_out):
    """nlx_bn254_plonk_grand_product on device tensors / host arrays of fr.Element words; scalars: canonical integers.
    Returns whether the product closes."""
    import ctypes
    from ._lib import dll
    keep = [B._fr_words(_to_mont(x)) for x in (beta, gamma, k1, k2)]
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    closes = ctypes.c_int32()
    ctx.check(dll.nlx_bn254_plonk_grand_product(ctx.handle, log_n, ptr(l), ptr(r), ptr(o), ptr(s1), ptr(s2), ptr(s3),
                                                keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data,
                                                ptr(z_out), ctypes.byref(closes)))
    return bool(closes.value)


def lincomb(ctx, polys, scalars, out):
    """out = sum_t scalars[t] polys[t] (nlx_bn254_fr_lincomb): polys device tensors / host arrays (m, 4), scalars canonical integers"""
    import ctypes
    from ._lib import dll
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    m = polys[0].shape[0]
    arr = (ctypes.c_void_p * len(polys))(*[ptr(p) for p in polys])
    sc = np.stack([B._fr_words(_to_mont(s)) for s in scalars])
    ctx.check(dll.nlx_bn254_fr_lincomb(ctx.handle, m, len(polys), arr, sc.ctypes.data, ptr(out)))
    return out


def groth16_quotient(ctx, a, b, c, coset_shift=5):
    """nlx_bn254_groth16_quotient: a, b, c = values of A w, B w, C w on H ((n, 4) arrays or device tensors of fr.Element words);
    returns h's n coefficients as a host array (n, 4)."""
    from ._lib import dll
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else np.ascontiguousarray(x, dtype=np.uint64).ctypes.data
    n = a.shape[0]
    keep = [x if hasattr(x, "data_ptr") else np.ascontiguousarray(x, dtype=np.uint64) for x in (a, b, c)]
    sh = B._fr_words(_to_mont(coset_shift))
    out = np.zeros((n, 4), dtype=np.uint64)
    ctx.check(dll.nlx_bn254_groth16_quotient(ctx.handle, n.bit_length() - 1, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), sh.ctypes.data, out.ctypes.data))
    return out


# ---- the proof in gnark's shape: its fiat-shamir, its blinding, its batched opening, its bytes (round 4) ----------------------
# The host-side mirror of gnark backend/plonk/bn254 Prove (Go, not in /root/reference; succinct.json:7-8 names the entry point
# that runs it), restated from its published structure [U: from memory, no gnark-produced vector exists here]; every heavy
# step is one library call on device-resident polynomials.  Bsb22 commitments (api.Commit: what the wrapper circuit's range
# checks go through) are part of it: tools/gnark_bsb22_model.py states their rules one by one and is the model for keys that
# have them (tests/test_gpu_bn254_bsb22.py).  oracle/bn254_py.py gnark_plonk_prove_model restates the same
# protocol on big integers (tests only); tests/test_gpu_bn254_plonk.py compares the BYTES and runs the model's verifier.
Q = B.BN254_Q


def fr_bytes(x):
    return (int(x) % R).to_bytes(32, "big")


def g1_marshal(words):
    """G1Affine.Marshal(): x || y, big-endian (what the transcript binds)"""
    pt = B.bn254_g1_unpack(words)
    if pt is None:
        return bytes([0x40]) + bytes(63)
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def g1_compress(words):
    """G1Affine.Bytes(): x with 0b10 / 0b11 in the top two bits for the smaller / larger y, 0b01 for infinity (Proof.WriteTo)"""
    pt = B.bn254_g1_unpack(words)
    if pt is None:
        return bytes([0x40]) + bytes(31)
    b = bytearray(pt[0].to_bytes(32, "big"))
    b[0] |= 0xC0 if pt[1] > (Q - 1) // 2 else 0x80
    return bytes(b)


class FiatShamir:
    """gnark-crypto fiatshamir.Transcript over SHA-256: named challenges in a fixed order; challenge i hashes its name, the raw
    bytes of challenge i - 1 and whatever was bound to it"""

    def __init__(self, *names):
        self.names, self.bound, self.raw = names, {k: [] for k in names}, {}

    def bind(self, name, data):
        self.bound[name].append(bytes(data))

    def challenge(self, name):
        i = self.names.index(name)
        h = hashlib.sha256(name.encode())
        if i:
            h.update(self.raw[self.names[i - 1]])
        for b in self.bound[name]:
            h.update(b)
        self.raw[name] = h.digest()
        return int.from_bytes(self.raw[name], "big") % R


def _words_to_int(t):
    return sum((int(v) & 0xFFFFFFFFFFFFFFFF) << (64 * k) for k, v in enumerate(t.tolist()))


def _blinded(torch, coeffs, n, b):
    """coefficients (n, 4) on the device + (b[0] + b[1] X + ...)(X^n - 1): a tensor of n + len(b) coefficients; only 2 len(b)
    of them change, patched through the host (fr.Element words are Montgomery residues)"""
    out = torch.zeros((n + len(b), 4), dtype=torch.int64, device=coeffs.device)
    out[:n] = coeffs
    for i, bi in enumerate(b):
        for idx, sign in ((i, -1), (n + i, 1)):
            cur = _words_to_int(out[idx].cpu()) * _MONT_INV % R
            val = _to_mont((cur + sign * bi) % R)
            out[idx] = torch.from_numpy(B._fr_words(val).view(np.int64)).to(coeffs.device)
    return out


BSB22_DST = b"BSB22-Plonk"


def hash_to_field(msg, dst=BSB22_DST):
    """gnark-crypto fr.Hash(msg, dst, 1)[0]: RFC 9380 expand_message_xmd over SHA-256 to 48 bytes, read big-endian, mod r.  How
    a Bsb22 commitment comes back into the circuit: c_j = hash_to_field([PI2_j].Marshal())."""
    dst_prime = bytes(dst) + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + bytes(msg) + (48).to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b1 = hashlib.sha256(b0 + b"\x01" + dst_prime).digest()
    b2 = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dst_prime).digest()
    return int.from_bytes((b1 + b2)[:48], "big") % R


def prove_gnark(pk, l=None, r=None, o=None, public_inputs=(), blinding=None, commit_blinding=None, witness=None):
    """l, r, o: the wire values on H (n canonical integers each).  public_inputs: the values of the public-input polynomial on
    the first points of H (the circuit's qk leaves them out, as gnark's does).  blinding: nine scalars (l 2, r 2, o 2, z 3) -
    random when None; a test passes them to compare bytes with the model.  The SRS must hold n + 3 points.
    A key with k Bsb22 commitments (ProvingKey(commitments=...)): commitment j's polynomial pi2_j takes the L values on its
    committed rows and two blinding scalars (commit_blinding[2 j] on its commitment row, then commit_blinding[2 j + 1] on
    last_row; 2 k scalars, random when None), [PI2_j] is its KZG commitment and c_j = hash_to_field([PI2_j].Marshal()) is the
    value the circuit expects on the L wire of the commitment row.  Committed values may depend on earlier c_j: pass
    witness = a callable that receives [c_0 .. c_{j-1}] and returns (l, r, o) - it is called once per commitment and once
    with all k values for the final wires - or pass full l, r, o when every c_j is known already.  ValueError if in the end
    l[i_j] != c_j or a committed value differs from what was committed.
    Returns the proof's bytes (gnark Proof.WriteTo layout)."""
    import secrets
    import torch
    ctx, n, log_n = pk.ctx, pk.n, pk.log_n
    w, u, dev = root_of_unity(log_n), pk.k1, pk.device
    if pk.srs.shape[0] < n + 3:
        raise ValueError("the SRS must hold n + 3 points (blinded polynomials have up to n + 3 coefficients)")
    if (witness is None) == (l is None) or (witness is None and (r is None or o is None)):
        raise ValueError("pass the wires l, r, o or a callable witness(cs) -> (l, r, o)")
    b = [secrets.randbelow(R) for _ in range(9)] if blinding is None else [int(x) % R for x in blinding]
    commit = lambda c: B.bn254_msm_g1(ctx, pk.srs[:c.shape[0]], c.contiguous(), montgomery=True)
    at = lambda c, point: _from_words_mont(B.bn254_kzg_open(ctx, c.contiguous(), _to_mont(point), want_quotient=False)[0])
    to_dev = lambda cols: torch.from_numpy(B.bn254_pack([[_to_mont(x) for x in col] for col in cols]).view(np.int64)).to(dev)
    # round 0: the Bsb22 commitments, in order; the witness is completed between them
    k = len(pk.bsb22)
    cb = [secrets.randbelow(R) for _ in range(2 * k)] if commit_blinding is None else [int(x) % R for x in commit_blinding]
    if len(cb) != 2 * k:
        raise ValueError("two blinding scalars per Bsb22 commitment")
    cs, committed, pi2_values, pi2_coeffs, pi2c = [], [], [], [], []
    for j, info in enumerate(pk.bsb22):
        lj = l if witness is None else witness(list(cs))[0]
        committed.append([int(lj[i]) % R for i in info["committed"]])
        # pi2_j on H: the committed L values, a blinding scalar on the commitment row, THEN one on last_row (the second
        # assignment stands if the two coincide), zero elsewhere - only these entries cross to the device
        entries = dict(zip(info["committed"], committed[j]))
        entries[info["row"]] = cb[2 * j]
        entries[info["last_row"]] = cb[2 * j + 1]
        v = torch.zeros((1, n, 4), dtype=torch.int64, device=dev)
        v[0, torch.tensor(list(entries), dtype=torch.int64, device=dev)] = to_dev([list(entries.values())])[0]
        pi2_values.append(v)
        pi2_coeffs.append(B.bn254_ntt(ctx, v.clone(), inverse=True, montgomery=True)[0])
        pi2c.append(commit(pi2_coeffs[j]))
        cs.append(hash_to_field(g1_marshal(pi2c[j])))
    if witness is not None:
        l, r, o = witness(list(cs))
    for j, info in enumerate(pk.bsb22):
        if int(l[info["row"]]) % R != cs[j]:
            raise ValueError("Bsb22 commitment %d: the L wire of its commitment row is not the hash of the commitment" % j)
        if [int(l[i]) % R for i in info["committed"]] != committed[j]:
            raise ValueError("Bsb22 commitment %d: a committed value was changed after the commitment" % j)
    fs = FiatShamir("gamma", "beta", "alpha", "zeta")
    for name in ("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk"):
        fs.bind("gamma", g1_marshal(pk.commitments[name]))
    for c in pk.qcp_commitments:
        fs.bind("gamma", g1_marshal(c))
    for x in public_inputs:
        fs.bind("gamma", fr_bytes(x))
    # round 1: blinded wires
    wires = to_dev((l, r, o))   # (3, n, 4)
    wire_coeffs = B.bn254_ntt(ctx, wires.clone(), inverse=True, montgomery=True)
    bl = [_blinded(torch, wire_coeffs[i], n, b[2 * i:2 * i + 2]) for i in range(3)]
    lro = [commit(c) for c in bl]
    for c in lro:
        fs.bind("gamma", g1_marshal(c))
    gamma = fs.challenge("gamma")
    beta = fs.challenge("beta")
    # round 2: the grand product, blinded
    z = torch.empty((n, 4), dtype=torch.int64, device=dev)
    if not grand_product(ctx, log_n, wires[0], wires[1], wires[2], pk.value("s1"), pk.value("s2"), pk.value("s3"), beta, gamma, pk.k1, pk.k2, z):
        raise ValueError("the wires do not respect the circuit's copy constraints (the grand product does not close)")
    blz = _blinded(torch, B.bn254_ntt(ctx, z.clone().reshape(1, n, 4), inverse=True, montgomery=True)[0], n, b[6:9])
    zc = commit(blz)
    for c in pi2c:
        fs.bind("alpha", g1_marshal(c))
    fs.bind("alpha", g1_marshal(zc))
    alpha = fs.challenge("alpha")
    # round 3: the quotient of the BLINDED polynomials (nlx_bn254_plonk_quotient patches the coefficients it derives from the
    # values on H), all 4 n coefficients, cut into h1 h2 h3 of n + 2
    polys = {name: pk.value(name) for name in pk.NAMES}
    polys.update(l=wires[0], r=wires[1], o=wires[2], z=z)
    if len(public_inputs) or k:
        pi = [int(x) % R for x in public_inputs] + [0] * (n - len(public_inputs))
        for j, info in enumerate(pk.bsb22):
            pi[info["row"]] = cs[j]           # PI(w^i_j) = c_j: the commitment row reads - l + c_j = 0
        polys["pi"] = to_dev([pi])[0]
    h4 = torch.empty((4 * n, 4), dtype=torch.int64, device=dev)
    _, ok = B.bn254_plonk_quotient(ctx, polys, *[_to_mont(x) for x in (u, pk.k1, pk.k2, alpha, beta, gamma)], out=h4,
                                   blinding=[_to_mont(x) for x in b],
                                   qcp=[pk.qcp_values[j] for j in range(k)] if k else None, pi2=[v[0] for v in pi2_values] if k else None)
    if not ok:
        raise ValueError("the witness does not satisfy the circuit (the quotient has more than 3 n + 6 coefficients)")
    hs = [h4[0:n + 2], h4[n + 2:2 * n + 4], h4[2 * n + 4:3 * n + 6]]
    hc = [commit(c) for c in hs]
    for c in hc:
        fs.bind("zeta", g1_marshal(c))
    zeta = fs.challenge("zeta")
    # round 4: evaluations, z at w zeta on its own
    lz, rz, oz = (at(c, zeta) for c in bl)
    s1z, s2z = at(pk.coeff("s1"), zeta), at(pk.coeff("s2"), zeta)
    yw, _, zshift = B.bn254_kzg_open(ctx, blz, _to_mont(zeta * w % R), srs=pk.srs, want_quotient=False)
    zw = _from_words_mont(yw)
    # round 5: the linearised polynomial, foldedH, ONE batched opening at zeta
    zh = (pow(zeta, n, R) - 1) % R
    l1 = zh * pow(n * (zeta - 1) % R, R - 2, R) % R
    a_ = (lz + beta * zeta + gamma) * (rz + beta * pk.k1 * zeta + gamma) % R * (oz + beta * pk.k2 * zeta + gamma) % R
    b_ = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) % R
    m = n + 3

    def padded(c):
        if c.shape[0] == m:
            return c
        out = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        out[:c.shape[0]] = c
        return out
    lin = torch.empty((m, 4), dtype=torch.int64, device=dev)
    qcpz = [at(pk.qcp_coeffs[j], zeta) for j in range(k)]
    lincomb(ctx, [padded(pk.coeff(name)) for name in ("qm", "ql", "qr", "qo", "qk")] + [blz, padded(pk.coeff("s3"))] + [padded(pi2_coeffs[j]) for j in range(k)],
            [lz * rz % R, lz, rz, oz, 1, (alpha * a_ + alpha * alpha % R * l1) % R, (-alpha * b_ % R * beta % R * zw) % R] + qcpz, lin)
    zn2 = pow(zeta, n + 2, R)
    folded_h = torch.empty((n + 2, 4), dtype=torch.int64, device=dev)
    lincomb(ctx, [c.contiguous() for c in hs], [1, zn2, zn2 * zn2 % R], folded_h)
    batch = [padded(folded_h), lin, padded(bl[0]), padded(bl[1]), padded(bl[2]), padded(pk.coeff("s1")), padded(pk.coeff("s2"))]
    batch += [padded(pk.qcp_coeffs[j]) for j in range(k)]
    digests = [commit(folded_h), commit(lin)] + lro + [pk.commitments["s1"], pk.commitments["s2"]] + pk.qcp_commitments
    claimed = [at(batch[0], zeta), at(lin, zeta), lz, rz, oz, s1z, s2z] + qcpz
    fg = FiatShamir("gamma")
    fg.bind("gamma", fr_bytes(zeta))
    for d in digests:
        fg.bind("gamma", g1_marshal(d))
    for v in claimed:
        fg.bind("gamma", fr_bytes(v))
    gp = fg.challenge("gamma")
    folded = torch.empty((m, 4), dtype=torch.int64, device=dev)
    lincomb(ctx, batch, [pow(gp, i, R) for i in range(len(batch))], folded)
    bh = B.bn254_kzg_open(ctx, folded, _to_mont(zeta), srs=pk.srs, want_quotient=False)[2]
    out = b"".join(g1_compress(c) for c in lro) + g1_compress(zc) + b"".join(g1_compress(c) for c in hc)
    out += k.to_bytes(4, "big") + b"".join(g1_compress(c) for c in pi2c)      # Bsb22Commitments
    out += g1_compress(bh) + len(claimed).to_bytes(4, "big") + b"".join(fr_bytes(v) for v in claimed)
    return out + g1_compress(zshift) + fr_bytes(zw)


# ---- the same proof from a key resident in HBM, behind the C ABI (nlx_bn254_plonk_key_create / _commit / _prove) ------------
# What prove_gnark orchestrates above - transcript, blinding patches, the Bsb22 round, the linearisation scalars, the batched
# opening, Proof.WriteTo - runs inside the library (csrc/bn254_plonk_prove.hip); this is the binding.
class _PlonkKeyDesc(ctypes.Structure):
    """nlx_bn254_plonk_key_desc (include/nlx.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("flags", ctypes.c_uint32)] + [(k, ctypes.c_void_p) for k in (
        "ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "k1", "k2", "coset_shift", "srs")] + [
        ("n_srs", ctypes.c_uint64), ("n_commit", ctypes.c_uint32), ("qcp", ctypes.POINTER(ctypes.c_void_p)), ("n_committed", ctypes.c_void_p),
        ("committed_rows", ctypes.c_void_p), ("commit_rows", ctypes.c_void_p), ("last_row", ctypes.c_uint32)]


NLX_BN254_PLONK_KEY_COSET = 0x400


def _wire_words(col):
    """a wire column for the C ABI: an (n, 4) device tensor / uint64 array as it is, integers packed as fr.Element words"""
    if hasattr(col, "data_ptr"):
        return col.contiguous()
    if isinstance(col, np.ndarray) and col.dtype == np.uint64:
        return np.ascontiguousarray(col)
    return B.bn254_pack([[_to_mont(x) for x in col]])[0]


def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


class ResidentKey:
    """ProvingKey's arguments, kept by the library: coefficients, commitments, the converted SRS (and, with coset=True, the fixed
    polynomials' values on the quotient's coset) stay in HBM across proofs.  values may hold integer lists, (n, 4) uint64 arrays
    or device tensors of fr.Element words."""

    NAMES = ProvingKey.NAMES

    def __init__(self, ctx, values, srs, k1, k2, commitments=(), coset=False, coset_shift=None):
        import ctypes
        from ._lib import dll
        self.ctx, self.handle = ctx, None
        first = values["ql"]
        self.n = first.shape[0] if hasattr(first, "shape") else len(first)
        self.log_n = self.n.bit_length() - 1
        self.k1, self.k2 = int(k1), int(k2)
        self.bsb22 = [{"committed": [int(i) for i in c["committed"]], "row": int(c["row"]), "last_row": int(c["last_row"])} for c in commitments]
        k = self.k = len(self.bsb22)
        if k > 4:
            raise ValueError("at most four Bsb22 commitments")
        if any(c["last_row"] != self.bsb22[0]["last_row"] for c in self.bsb22):
            raise ValueError("a last_row that differs from the key's")
        keep = {name: _wire_words(values[name]) for name in self.NAMES}
        qcp = [_wire_words(values["qcp%d" % j]) for j in range(k)]
        srs = srs if hasattr(srs, "data_ptr") else np.ascontiguousarray(srs, dtype=np.uint64)
        sc = [B._fr_words(_to_mont(x)) for x in (self.k1, self.k2, self.k1 if coset_shift is None else coset_shift)]
        d = _PlonkKeyDesc()
        d.log_n, d.flags = self.log_n, 1 | (NLX_BN254_PLONK_KEY_COSET if coset else 0)
        for name in self.NAMES:
            setattr(d, name, _ptr(keep[name]))
        d.k1, d.k2, d.coset_shift = (x.ctypes.data for x in sc)
        d.srs, d.n_srs, d.n_commit = _ptr(srs), srs.shape[0], k
        arr = (ctypes.c_void_p * max(k, 1))(*[_ptr(q) for q in qcp])
        counts = np.array([len(c["committed"]) for c in self.bsb22], dtype=np.uint64)
        rows = np.array([i for c in self.bsb22 for i in c["committed"]], dtype=np.int64)
        crows = np.array([c["row"] for c in self.bsb22], dtype=np.int64)
        if k and (rows.min(initial=0) < 0 or rows.max(initial=0) >= 1 << 32 or crows.min() < 0 or crows.max() >= 1 << 32 or not 0 <= self.bsb22[0]["last_row"] < 1 << 32):
            raise ValueError("rows outside H")
        rows, crows = rows.astype(np.uint32), crows.astype(np.uint32)
        if k:
            d.qcp = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
            d.n_committed, d.committed_rows, d.commit_rows = counts.ctypes.data, rows.ctypes.data, crows.ctypes.data
            d.last_row = self.bsb22[0]["last_row"]
        h = ctypes.c_void_p()
        rc = dll.nlx_bn254_plonk_key_create(ctx.handle, ctypes.byref(d), ctypes.byref(h))
        if rc:
            _raise(ctx, rc)
        self.handle = h
        ctx._adopt(self)
        self.proof_bytes = dll.nlx_bn254_plonk_proof_bytes(h)

    @classmethod
    def _from_handle(cls, ctx, handle, log_n, k1, k2, commitments=()):
        """adopt a key the library built itself (nlx_bn254_plonk_setup_key)"""
        from ._lib import dll
        self = cls.__new__(cls)
        self.ctx, self.handle = ctx, handle
        self.log_n, self.n, self.k1, self.k2 = int(log_n), 1 << int(log_n), int(k1), int(k2)
        self.bsb22 = [{"committed": [int(i) for i in c["committed"]], "row": int(c["row"]), "last_row": int(c["last_row"])} for c in commitments]
        self.k = len(self.bsb22)
        ctx._adopt(self)
        self.proof_bytes = dll.nlx_bn254_plonk_proof_bytes(handle)
        return self

    def info(self):
        """dict: resident bytes, n, k, the committed rows of all sets, whether the coset values are resident"""
        from ._lib import dll
        out = np.zeros(5, dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_plonk_key_info(self.handle, out.ctypes.data))
        return {"resident_bytes": int(out[0]), "n": int(out[1]), "k": int(out[2]), "committed_rows": int(out[3]), "coset": bool(out[4])}

    def key_commitments(self):
        """(8 + k, 8) G1Affine words in the transcript's order: s1 s2 s3 ql qr qm qo qk qcp_0 .."""
        from ._lib import dll
        out = np.zeros((8 + self.k, 8), dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_plonk_key_commitments(self.handle, out.ctypes.data))
        return out

    def close(self):
        if self.handle and self.ctx.handle:
            from ._lib import dll
            dll.nlx_bn254_plonk_key_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _raise(ctx, rc):
    """NLX_E_INVAL from the prover is a statement about the caller's witness or key: ValueError, as prove_gnark raises"""
    from ._lib import NlxError, dll
    err = NlxError(rc, dll.nlx_last_error(ctx.handle).decode())
    if rc == -1:
        raise ValueError(str(err)) from err
    raise err


def commit_resident(key, j, l, blinding):
    """The solver's hint of commitment j (nlx_bn254_plonk_commit): l = the L wire as far as it is solved, blinding = two
    scalars.  Returns ([PI2_j] as G1Affine words, c_j as an integer)."""
    from ._lib import dll
    lw = _wire_words(l)
    b = np.stack([B._fr_words(_to_mont(int(x) % R)) for x in blinding])
    if b.shape[0] != 2:
        raise ValueError("two blinding scalars per Bsb22 commitment")
    point, c = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rc = dll.nlx_bn254_plonk_commit(key.ctx.handle, key.handle, j, _ptr(lw), b.ctypes.data, point.ctypes.data, c.ctypes.data)
    if rc:
        _raise(key.ctx, rc)
    return point, _from_words_mont(c)


def prove_resident(key, l=None, r=None, o=None, public_inputs=(), blinding=None, commit_blinding=None, witness=None):
    """prove_gnark's contract on a ResidentKey: the same arguments (wires also as (n, 4) device tensors of fr.Element words), the
    same bytes, ValueError where prove_gnark raises it.  One library call per proof, and one per commitment when the witness is
    a callable (the hint)."""
    import ctypes
    import secrets
    from ._lib import dll
    k = key.k
    if (witness is None) == (l is None) or (witness is None and (r is None or o is None)):
        raise ValueError("pass the wires l, r, o or a callable witness(cs) -> (l, r, o)")
    b = [secrets.randbelow(R) for _ in range(9)] if blinding is None else [int(x) % R for x in blinding]
    if len(b) != 9:
        raise ValueError("nine blinding scalars")
    cb = [secrets.randbelow(R) for _ in range(2 * k)] if commit_blinding is None else [int(x) % R for x in commit_blinding]
    if len(cb) != 2 * k:
        raise ValueError("two blinding scalars per Bsb22 commitment")
    committed = []
    if witness is not None:
        cs = []
        for j, info in enumerate(key.bsb22):
            lj = witness(list(cs))[0]
            committed.append([int(lj[i]) % R for i in info["committed"]])
            cs.append(commit_resident(key, j, lj, cb[2 * j:2 * j + 2])[1])
        l, r, o = witness(list(cs))
        for j, info in enumerate(key.bsb22):
            if [int(l[i]) % R for i in info["committed"]] != committed[j]:
                raise ValueError("Bsb22 commitment %d: a committed value was changed after the commitment" % j)
    wires = [_wire_words(c) for c in (l, r, o)]
    pubs = np.stack([B._fr_words(_to_mont(int(x) % R)) for x in public_inputs]) if len(public_inputs) else None
    bw = np.stack([B._fr_words(_to_mont(x)) for x in b])
    cbw = np.stack([B._fr_words(_to_mont(x)) for x in cb]) if k else None
    out = np.zeros(key.proof_bytes, dtype=np.uint8)
    got = ctypes.c_size_t()
    rc = dll.nlx_bn254_plonk_prove(key.ctx.handle, key.handle, _ptr(wires[0]), _ptr(wires[1]), _ptr(wires[2]),
                                   pubs.ctypes.data if pubs is not None else None, len(public_inputs), bw.ctypes.data,
                                   cbw.ctypes.data if k else None, out.ctypes.data, out.nbytes, ctypes.byref(got))
    if rc:
        _raise(key.ctx, rc)
    return out[:got.value].tobytes()


# ---- the witness checker of the resident prover (csrc/bn254_plonk_check.hip) ----
CHECK_GATES, CHECK_COPIES, CHECK_COMMITS, CHECK_ALL = 1, 2, 4, 7


class WitnessReport(ctypes.Structure):
    """nlx_bn254_plonk_witness_report (include/nlx.h): what nlx_bn254_plonk_check_witness found; `message` is the library's
    line.  Field elements are four canonical words: value("gate_value") gives the integer."""
    _fields_ = [("checked", ctypes.c_uint32), ("satisfied", ctypes.c_uint32),
                ("gate_rows_bad", ctypes.c_uint64), ("gate_rows_skipped", ctypes.c_uint32), ("gate_row", ctypes.c_uint32),
                ("gate_value", ctypes.c_uint64 * 4),
                ("copy_cells_bad", ctypes.c_uint64), ("copy_row", ctypes.c_uint32), ("copy_wire", ctypes.c_uint32),
                ("copy_to_row", ctypes.c_uint32), ("copy_to_wire", ctypes.c_uint32), ("copy_value", ctypes.c_uint64 * 4),
                ("copy_to_value", ctypes.c_uint64 * 4),
                ("commits_bad", ctypes.c_uint32), ("commit_index", ctypes.c_uint32), ("commit_row", ctypes.c_uint32),
                ("commit_pad_", ctypes.c_uint32), ("commit_have", ctypes.c_uint64 * 4), ("commit_want", ctypes.c_uint64 * 4),
                ("cache_bytes", ctypes.c_uint64)]
    message = ""

    def value(self, name):
        return sum(int(w) << (64 * i) for i, w in enumerate(getattr(self, name)))

    def as_dict(self):
        """every field but the padding, field elements as integers"""
        return {name: (self.value(name) if name.endswith(("_value", "_have", "_want")) else int(getattr(self, name)))
                for name, _ in self._fields_ if name != "commit_pad_"}

    def __bool__(self):
        return self.satisfied == 1

    def __str__(self):
        return self.message if not self else "the witness satisfies the circuit (checked = %d)" % self.checked

    def raise_if_unsatisfied(self):
        if not self:
            raise ValueError(self.message)
        return self


def check_resident(key, l=None, r=None, o=None, public_inputs=(), commit_blinding=None, what=CHECK_ALL, witness=None):
    """nlx_bn254_plonk_check_witness on a ResidentKey: which row, which copy or which Bsb22 commitment the wires break.  The
    wires as prove_resident takes them: integer lists, (n, 4) device tensors of fr.Element words, or witness = a callable that
    receives [c_0 .. c_{j-1}] and returns (l, r, o), driven through commit_resident as prove_resident drives it (that form
    needs commit_blinding).  commit_blinding: the 2 k scalars the proof will use - required when `what` holds CHECK_COMMITS
    and the key carries commitments.  CHECK_ALL is satisfied exactly when prove_resident accepts the same arguments.
    Returns a WitnessReport (truthy when satisfied); bad arguments raise as prove_resident's do."""
    from ._lib import dll
    k = key.k
    if (witness is None) == (l is None) or (witness is None and (r is None or o is None)):
        raise ValueError("pass the wires l, r, o or a callable witness(cs) -> (l, r, o)")
    cb = None if commit_blinding is None else [int(x) % R for x in commit_blinding]
    if cb is not None and len(cb) != 2 * k:
        raise ValueError("two blinding scalars per Bsb22 commitment")
    if witness is not None:
        if k and cb is None:
            raise ValueError("a callable witness is completed through the commitments' hints: pass commit_blinding")
        cs = []
        for j in range(k):
            cs.append(commit_resident(key, j, witness(list(cs))[0], cb[2 * j:2 * j + 2])[1])
        l, r, o = witness(list(cs))
    wires = [_wire_words(c) for c in (l, r, o)]
    pubs = np.stack([B._fr_words(_to_mont(int(x) % R)) for x in public_inputs]) if len(public_inputs) else None
    cbw = np.stack([B._fr_words(_to_mont(x)) for x in cb]) if k and cb is not None else None
    rep = WitnessReport()
    rc = dll.nlx_bn254_plonk_check_witness(key.ctx.handle, key.handle, _ptr(wires[0]), _ptr(wires[1]), _ptr(wires[2]),
                                           pubs.ctypes.data if pubs is not None else None, len(public_inputs),
                                           cbw.ctypes.data if cbw is not None else None, int(what), ctypes.byref(rep))
    if rc:
        _raise(key.ctx, rc)
    if not rep:
        rep.message = dll.nlx_last_error(key.ctx.handle).decode()
    return rep


# ---- gnark's plonk.Setup on the device, from the constraints (csrc/bn254_plonk_setup.hip; the rules:
# tools/gnark_plonk_setup_model.py - recalled from gnark v0.9 and UNPINNED, parity with gnark-produced keys is not claimed) ----
SETUP_INFO_WORDS = 6
SETUP_ARRAYS = {"ql": 0, "qr": 1, "qm": 2, "qo": 3, "qk": 4, "s1": 5, "s2": 6, "s3": 7, "qcp0": 8, "qcp1": 9, "qcp2": 10, "qcp3": 11,
                "cells": 12, "permutation": 13, "sigma_cells": 14}


class _PlonkSetupDesc(ctypes.Structure):
    """nlx_bn254_plonk_setup_desc (include/nlx.h)"""
    _fields_ = ([("log_n", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_variables", ctypes.c_uint64), ("n_public", ctypes.c_uint64),
                 ("n_constraints", ctypes.c_uint64)]
                + [(k, ctypes.c_void_p) for k in ("xa", "xb", "xc", "ql", "qr", "qm", "qo", "qk", "coeffs")]
                + [("n_coeffs", ctypes.c_uint64)]
                + [(k, ctypes.c_void_p) for k in ("k1", "k2", "coset_shift")]
                + [("n_commit", ctypes.c_uint32), ("n_committed", ctypes.c_void_p), ("committed", ctypes.c_void_p),
                   ("commit_constraint", ctypes.c_void_p)])


def _element_words(x):
    """an integer as fr.Element words; r <= x < 2^256 is no residue: its words go as they are and the library refuses them"""
    x = int(x)
    if not 0 <= x < (1 << 256):
        raise ValueError("a field element does not fit four words")
    return B._fr_words(_to_mont(x) if x < R else x)


class Setup:
    """struct nlx_bn254_plonk_setup: gnark's plonk.Setup(spr, srs) from a sparse constraint system, resident on the device (owns
    the handle).  constraints: one (xa, xb, xc, ql, qr, qm, qo, qk) per constraint - three variable ids and five ids into
    `coeffs` - as a list or an (m, 8) array; coeffs: integers below r, or (c, 4) uint64 fr.Element words; commitments: one
    {"committed": ascending constraint indices, "constraint": the commitment's own constraint} per Bsb22 commitment; log_n = 0
    takes the smallest domain of at least 8 rows that holds n_public + m rows.  coset_shift defaults to k1 (gnark: k1 = u,
    k2 = u^2)."""

    def __init__(self, ctx, n_variables, n_public, constraints, coeffs, k1=5, k2=25, coset_shift=None, commitments=(), log_n=0, flags=1):
        from ._lib import dll
        self.ctx, self.handle = ctx, None
        self.n_variables, self.n_public, self.k1, self.k2 = int(n_variables), int(n_public), int(k1), int(k2)
        self.sets = [{"committed": [int(i) for i in c["committed"]], "constraint": int(c["constraint"])} for c in commitments]
        cons = np.ascontiguousarray(np.asarray(constraints, dtype=np.int64).reshape(-1, 8))
        if cons.size and (cons.min() < 0 or cons.max() >= 1 << 32):
            raise ValueError("variable and coefficient ids are 32-bit")
        cols = np.ascontiguousarray(cons.T.astype(np.uint32))          # (8, m): xa xb xc ql qr qm qo qk
        self.n_constraints = cons.shape[0]
        if isinstance(coeffs, np.ndarray) and coeffs.dtype == np.uint64:
            cw = np.ascontiguousarray(coeffs).reshape(-1, 4)
        else:
            cw = np.stack([_element_words(x) for x in coeffs]) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        sc = [_element_words(x) for x in (self.k1, self.k2, self.k1 if coset_shift is None else coset_shift)]
        d = _PlonkSetupDesc()
        d.log_n, d.flags = int(log_n), int(flags)
        d.n_variables, d.n_public, d.n_constraints = self.n_variables, self.n_public, self.n_constraints
        if self.n_constraints:
            for i, name in enumerate(("xa", "xb", "xc", "ql", "qr", "qm", "qo", "qk")):
                setattr(d, name, cols[i].ctypes.data)
        d.coeffs, d.n_coeffs = (cw.ctypes.data if len(cw) else None), len(cw)
        d.k1, d.k2, d.coset_shift = (x.ctypes.data for x in sc)
        d.n_commit = len(self.sets)
        ids = [i for c in self.sets for i in c["committed"]] + [c["constraint"] for c in self.sets]
        if any(not 0 <= i < 1 << 32 for i in ids):
            raise ValueError("constraint indices are 32-bit")
        counts = np.array([len(c["committed"]) for c in self.sets], dtype=np.uint64)
        committed = np.array([i for c in self.sets for i in c["committed"]] + [0], dtype=np.uint32)
        own = np.array([c["constraint"] for c in self.sets], dtype=np.uint32)
        if self.sets:
            d.n_committed, d.committed, d.commit_constraint = counts.ctypes.data, committed.ctypes.data, own.ctypes.data
        h = ctypes.c_void_p()
        ctx.check(dll.nlx_bn254_plonk_setup(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)
        i = self.info()
        self.n, self.log_n, self.k = i["n"], i["log_n"], i["k"]

    def info(self):
        """dict: n, log_n, k, the rows in use (n_public + constraints), the variables that occur, the longest class"""
        from ._lib import dll
        out = np.zeros(SETUP_INFO_WORDS, dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_plonk_setup_info(self.handle, out.ctypes.data))
        return {k: int(out[i]) for i, k in enumerate(("n", "log_n", "k", "rows_used", "variables_used", "longest_class"))}

    def read(self, name, device=None):
        """one array by name (SETUP_ARRAYS): a polynomial as (n, 4) fr.Element words, "cells" / "permutation" / "sigma_cells" as
        3 n uint32 - numpy, or with device="cuda:k" a device tensor (int64 / int32 bit patterns)"""
        from ._lib import dll
        which = SETUP_ARRAYS[name]
        poly = which < 12
        if device is not None:
            import torch
            out = torch.empty((self.n, 4) if poly else (3 * self.n,), dtype=torch.int64 if poly else torch.int32, device=device)
            self.ctx.check(dll.nlx_bn254_plonk_setup_read(self.handle, which, out.data_ptr()))
            return out
        out = np.zeros((self.n, 4) if poly else (3 * self.n,), dtype=np.uint64 if poly else np.uint32)
        self.ctx.check(dll.nlx_bn254_plonk_setup_read(self.handle, which, out.ctypes.data))
        return out

    def values(self):
        """the fixed polynomials by values on H as integers, in Instance.key_values()'s shape: ql .. s3, qcp0 .."""
        names = list(ResidentKey.NAMES) + ["qcp%d" % j for j in range(self.k)]
        return {name: [_from_words_mont(w) for w in self.read(name)] for name in names}

    def commitment_info(self):
        """the commitments as ResidentKey describes them: rows of H"""
        last = self.n_public + self.n_constraints - 1
        return [{"committed": [i + self.n_public for i in c["committed"]], "row": c["constraint"] + self.n_public, "last_row": last}
                for c in self.sets]

    def key(self, srs, coset=False):
        """nlx_bn254_plonk_setup_key: the ResidentKey of this setup, built from the device arrays, its permutation already
        decoded for the witness checker.  srs: (>= n + 3, 8) G1Affine words, numpy or a device tensor."""
        from ._lib import dll
        srs = srs if hasattr(srs, "data_ptr") else np.ascontiguousarray(srs, dtype=np.uint64)
        h = ctypes.c_void_p()
        rc = dll.nlx_bn254_plonk_setup_key(self.handle, _ptr(srs), srs.shape[0], NLX_BN254_PLONK_KEY_COSET if coset else 0, ctypes.byref(h))
        if rc:
            _raise(self.ctx, rc)
        return ResidentKey._from_handle(self.ctx, h, self.log_n, self.k1, self.k2, self.commitment_info())

    def wires(self, values, device="cuda:0"):
        """nlx_bn254_plonk_setup_wires, the solver's last step: the solved variable vector (n_variables integers, (n_variables, 4)
        fr.Element words or a device tensor of them) -> l, r, o as (n, 4) device tensors"""
        import torch
        from ._lib import dll
        v = _wire_words(values)
        if v.shape[0] != self.n_variables:
            raise ValueError("expected %d variable values" % self.n_variables)
        out = [torch.empty((self.n, 4), dtype=torch.int64, device=device) for _ in range(3)]
        self.ctx.check(dll.nlx_bn254_plonk_setup_wires(self.ctx.handle, self.handle, _ptr(v), *(t.data_ptr() for t in out)))
        return tuple(out)

    def solver(self, n_secret, hints=(), fuse=True):
        """nlx_bn254_plonk_solver_create: the witness solver of this constraint system (Solver).  Variables [0, n_public +
        n_secret) are the inputs; hints: ("inv_zero", before, x, y), ("n_bits", before, x, outs), ("quo_rem64", before, x, m, q, r)
        with `before` = the constraint in front of which the hint runs, non-descending; the commitments' hints are implied.
        fuse=False: one launch per level.  ValueError where the schedule refuses (the message names the constraint or hint)."""
        return Solver(self, n_secret, hints, fuse)

    def close(self):
        if self.handle and self.ctx.handle:
            from ._lib import dll
            dll.nlx_bn254_plonk_setup_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- gnark's witness solver on the device, by levels (csrc/bn254_plonk_solve.hip; the rules:
# tools/gnark_plonk_solve_model.py - recalled from gnark v0.9 and UNPINNED) ----
SOLVER_INFO_WORDS = 16
SOLVER_NO_FUSE = 0x800
SOLVER_FUSE = 1024
HINT_KINDS = {"inv_zero": 4, "n_bits": 5, "quo_rem64": 6}
SOLVE_KINDS = {0: "", 1: "DIV_ZERO", 2: "UNSATISFIED"}
SOLVER_INFO_NAMES = ("levels", "widest_level", "launches", "fused_runs", "checks", "solve_l", "solve_r", "solve_o", "inv_zero", "n_bits", "quo_rem64",
                     "commits", "constant_divisors", "value_divisors", "unassigned", "resident_bytes")


class _PlonkSolverDesc(ctypes.Structure):
    """nlx_bn254_plonk_solver_desc (include/nlx.h)"""
    _fields_ = ([("n_secret", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("n_hints", ctypes.c_uint32)]
                + [(k, ctypes.c_void_p) for k in ("hint_kind", "hint_before", "hint_param", "hint_in_off", "hint_out_off", "hint_in", "hint_out")])


class SolveReport(ctypes.Structure):
    """nlx_bn254_plonk_solve_report (include/nlx.h); `message` is the library's line, .value_int the canonical integer"""
    _fields_ = [("solved", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("constraint", ctypes.c_uint32), ("level", ctypes.c_uint32),
                ("value", ctypes.c_uint64 * 4), ("failures", ctypes.c_uint64), ("poisoned_variables", ctypes.c_uint64),
                ("levels_run", ctypes.c_uint32), ("launches", ctypes.c_uint32)]
    message = ""
    commit_points = None          # (k, 8) G1Affine words: the [PI2_j]

    @property
    def value_int(self):
        return sum(int(w) << (64 * i) for i, w in enumerate(self.value))

    @property
    def kind_name(self):
        return SOLVE_KINDS.get(int(self.kind), "?")

    def __bool__(self):
        return self.solved == 1

    def __str__(self):
        return self.message if not self else "solved: %d levels in %d launches" % (self.levels_run, self.launches)

    def raise_if_unsolved(self):
        if not self:
            raise ValueError(self.message)
        return self


class Solver:
    """struct nlx_bn254_plonk_solver (owns the handle); made by Setup.solver.  It keeps its own copies and is independent of the
    Setup once made; it belongs to the Setup's context."""

    def __init__(self, setup, n_secret, hints=(), fuse=True):
        from ._lib import dll
        ctx = self.ctx = setup.ctx
        self.handle = None
        self.n_variables, self.n_public, self.n_secret, self.n_constraints, self.k = setup.n_variables, setup.n_public, int(n_secret), setup.n_constraints, setup.k
        kinds, befores, params, ins, outs, in_off, out_off = [], [], [], [], [], [0], [0]
        for t in hints:
            kind = HINT_KINDS[t[0]]
            o = [t[3]] if kind == 4 else list(t[3]) if kind == 5 else [t[4], t[5]]
            m = int(t[3]) if kind == 6 else 0
            if not 0 <= m < 1 << 64:
                raise ValueError("quo_rem64 takes 1 <= m < 2^64")
            kinds.append(kind), befores.append(int(t[1])), params.append(m), ins.append(int(t[2])), outs.extend(int(v) for v in o)
            in_off.append(len(ins)), out_off.append(len(outs))
        if any(not 0 <= v < 1 << 32 for v in befores + ins + outs):
            raise ValueError("variable and constraint ids are 32-bit")
        keep = [np.array(kinds + [0], dtype=np.uint32), np.array(befores + [0], dtype=np.uint32), np.array(params + [0], dtype=np.uint64),
                np.array(in_off, dtype=np.uint64), np.array(out_off, dtype=np.uint64), np.array(ins + [0], dtype=np.uint32), np.array(outs + [0], dtype=np.uint32)]
        d = _PlonkSolverDesc()
        d.n_secret, d.flags, d.n_hints = self.n_secret, 1 | (0 if fuse else SOLVER_NO_FUSE), len(kinds)
        for name, a in zip(("hint_kind", "hint_before", "hint_param", "hint_in_off", "hint_out_off", "hint_in", "hint_out"), keep):
            setattr(d, name, a.ctypes.data)
        h = ctypes.c_void_p()
        rc = dll.nlx_bn254_plonk_solver_create(ctx.handle, setup.handle, ctypes.byref(d), ctypes.byref(h))
        if rc:
            _raise(ctx, rc)
        self.handle = h
        ctx._adopt(self)

    def info(self):
        """dict by SOLVER_INFO_NAMES: levels, the widest level, launches per solve, fused runs, items per form, constant and
        value-dependent divisors, variables left unassigned, resident bytes"""
        from ._lib import dll
        out = np.zeros(SOLVER_INFO_WORDS, dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_plonk_solver_info(self.handle, out.ctypes.data))
        return {k: int(out[i]) for i, k in enumerate(SOLVER_INFO_NAMES)}

    def read(self, name):
        """the schedule per constraint as uint32: "level" (0 where skipped), "form" (0 check, 1 2 3 solve L R O, 8 skipped),
        "assigns" (0xFFFFFFFF where none)"""
        from ._lib import dll
        out = np.zeros(self.n_constraints, dtype=np.uint32)
        self.ctx.check(dll.nlx_bn254_plonk_solver_read(self.handle, {"level": 0, "form": 1, "assigns": 2}[name], out.ctypes.data))
        return out

    def solve(self, inputs, key=None, commit_blinding=None, device="cuda:0"):
        """nlx_bn254_plonk_solver_solve: inputs = the n_public + n_secret given values (integers, (m, 4) fr.Element words or a
        device tensor of them); key: the ResidentKey, required exactly when the setup carries commitments; commit_blinding: the
        2 k scalars the proof will use.  -> (values, SolveReport): values as an (n_variables, 4) device tensor - what
        Setup.wires takes -, or a numpy array with device=None.  A failing witness still returns: see the report."""
        from ._lib import dll
        v = _wire_words(inputs)
        if v.shape[0] != self.n_public + self.n_secret:
            raise ValueError("expected %d input values" % (self.n_public + self.n_secret))
        k = self.k
        cb = None
        if commit_blinding is not None:
            if len(commit_blinding) != 2 * k:
                raise ValueError("two blinding scalars per Bsb22 commitment")
            cb = np.stack([B._fr_words(_to_mont(int(x) % R)) for x in commit_blinding]) if k else None
        if device is not None:
            import torch
            out = torch.empty((self.n_variables, 4), dtype=torch.int64, device=device)
        else:
            out = np.zeros((self.n_variables, 4), dtype=np.uint64)
        points = np.zeros((max(k, 1), 8), dtype=np.uint64)
        rep = SolveReport()
        rc = dll.nlx_bn254_plonk_solver_solve(self.ctx.handle, self.handle, _ptr(v), key.handle if key is not None else None,
                                              cb.ctypes.data if cb is not None else None, _ptr(out), points.ctypes.data, ctypes.addressof(rep))
        if rc:
            _raise(self.ctx, rc)
        rep.commit_points = points[:k]
        if not rep:
            rep.message = dll.nlx_last_error(self.ctx.handle).decode()
        return out, rep

    def close(self):
        if self.handle and self.ctx.handle:
            from ._lib import dll
            dll.nlx_bn254_plonk_solver_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kzg_srs(ctx, tau, n, device=None):
    """A TEST SRS from its trapdoor (nlx_bn254_kzg_srs; gnark-crypto kzg.NewSRS(n, tau)): ([tau^i]_1 for i < n as (n, 8) G1Affine
    words - numpy, or an int64 device tensor with device="cuda:k" -, [1]_2 and [tau]_2 as 16 words each).  Whoever knows tau
    forges openings."""
    from ._lib import dll
    t = _element_words(tau)
    g2 = np.zeros((2, 16), dtype=np.uint64)
    if device is not None:
        import torch
        g1 = torch.empty((int(n), 8), dtype=torch.int64, device=device)
        ctx.check(dll.nlx_bn254_kzg_srs(ctx.handle, t.ctypes.data, int(n), g1.data_ptr(), g2.ctypes.data))
    else:
        g1 = np.zeros((int(n), 8), dtype=np.uint64)
        ctx.check(dll.nlx_bn254_kzg_srs(ctx.handle, t.ctypes.data, int(n), g1.ctypes.data, g2.ctypes.data))
    return g1, g2[0], g2[1]


def srs_to_bytes(ctx, g1, g2_one, g2_tau, raw=False):
    """kzg.SRS.WriteTo (raw: WriteRawTo) of an SRS as kzg_srs returns it: the slice Pk.G1, Vk.G2[0], Vk.G2[1], Vk.G1 (= g1[0]); the
    points through the device codec, the slice in one call.  Layout: tools/gnark_bytes_model.py rule 9, recalled and unpinned."""
    from . import bn254_codec as C
    if hasattr(g1, "data_ptr"):
        first = g1[:1].cpu().numpy().view(np.uint64)
    else:
        g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 8)
        first = g1[:1]
    if not len(first):
        raise ValueError("an SRS holds at least one G1 point")
    g2 = np.stack([np.ascontiguousarray(g2_one, dtype=np.uint64).reshape(16), np.ascontiguousarray(g2_tau, dtype=np.uint64).reshape(16)])
    return C.slice_bytes(ctx, False, g1, raw) + C.bn254_g2_encode(ctx, g2, raw) + C.bn254_g1_encode(ctx, first, raw)


def srs_from_bytes(ctx, data, device=None):
    """kzg.SRS.ReadFrom: (g1, g2_0, g2_1), the tuple kzg_srs returns and setup takes - g1 numpy words, or an int64 device tensor
    with device="cuda:k".  The mode (compressed or raw) is read off the first point's flag bits.  Every point goes through the
    device codec (range, curve, for G2 the subgroup); NlxError (NLX_E_INVAL) names the section for short or trailing data and the
    section and index for a bad point."""
    from . import bn254_codec as C
    from ._lib import NlxError
    if len(data) >= 4 and not any(data[:4]):
        raise NlxError(C.NLX_E_INVAL, "Pk.G1 is empty")
    rd = C.Reader(ctx, data, C.container_is_raw(data, [("Pk.G1 count", 4)], "Pk.G1"), device)
    g1 = rd.points(False, "Pk.G1", device=True)
    g2_0, g2_1 = rd.point(True, "Vk.G2[0]"), rd.point(True, "Vk.G2[1]")
    vk_g1 = rd.point(False, "Vk.G1")
    rd.end("SRS")
    first = g1[0].cpu().numpy().view(np.uint64) if hasattr(g1, "data_ptr") else g1[0]
    if not np.array_equal(vk_g1, first):
        raise NlxError(C.NLX_E_INVAL, "Vk.G1 is not Pk.G1[0]")
    return g1, g2_0, g2_1


def setup(ctx, n_variables, n_public, constraints, coeffs, srs, k1=5, k2=25, coset_shift=None, commitments=(), log_n=0, coset=False):
    """gnark's plonk.Setup(spr, srs) in one call: (ResidentKey, Setup).  The Setup stays open for .wires(values) - the solver's
    last step - and .read(); close it when the witnesses are done.  The rules are recalled from gnark v0.9 and unpinned
    (tools/gnark_plonk_setup_model.py)."""
    s = Setup(ctx, n_variables, n_public, constraints, coeffs, k1, k2, coset_shift, commitments, log_n)
    try:
        return s.key(srs, coset), s
    except Exception:
        s.close()
        raise


def eval_many(ctx, polys, point):
    """nlx_bn254_fr_eval_many: up to 16 polynomials ((m_i, 4) uint64 arrays / device tensors of fr.Element words, coefficients in
    natural order, lengths may differ) at one point (a canonical integer) -> their values as canonical integers"""
    import ctypes
    from ._lib import dll
    keep = [p.contiguous() if hasattr(p, "data_ptr") else np.ascontiguousarray(p, dtype=np.uint64) for p in polys]
    arr = (ctypes.c_void_p * max(len(keep), 1))(*[_ptr(p) for p in keep])
    lens = np.array([p.shape[0] for p in keep], dtype=np.uint64)
    z = B._fr_words(_to_mont(int(point) % R))
    out = np.zeros((max(len(keep), 1), 4), dtype=np.uint64)
    ctx.check(dll.nlx_bn254_fr_eval_many(ctx.handle, len(keep), arr, lens.ctypes.data, z.ctypes.data, out.ctypes.data))
    return [_from_words_mont(w) for w in out[:len(keep)]]


def hash_to_field_native(msg, dst=BSB22_DST):
    """nlx_bn254_hash_to_field (host code of the library, no context): what hash_to_field above computes with hashlib"""
    from ._lib import dll
    msg, dst = bytes(msg), bytes(dst)
    out = np.zeros(4, dtype=np.uint64)
    rc = dll.nlx_bn254_hash_to_field(msg, len(msg), dst, len(dst), out.ctypes.data)
    if rc:
        raise ValueError("nlx_bn254_hash_to_field: error %d" % rc)
    return _from_words_mont(out)


# ---- the verifier (csrc/bn254_plonk_verify.hip; the model with real pairings is
# tools/gnark_plonk_verify_model.py) ----
VERIFY_ACCEPT, VERIFY_MALFORMED, VERIFY_PAIRING, VERIFY_ALGEBRAIC = 0, 1, 3, 4
_REASONS = {VERIFY_ACCEPT: "accepted", VERIFY_MALFORMED: "malformed", VERIFY_ALGEBRAIC: "the algebraic relation fails",
            VERIFY_PAIRING: "the pairing equation fails"}
_NLX_E_INVAL, _NLX_E_RANGE = -1, -4


class _PlonkVkDesc(ctypes.Structure):
    """nlx_bn254_plonk_vk_desc (include/nlx.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("n_public", ctypes.c_uint32), ("n_commit", ctypes.c_uint32)] + [(name, ctypes.c_void_p) for name in (
        "k1", "k2", "commitments", "commit_rows", "g1", "g2", "g2_tau")]


class Verdict(ctypes.Structure):
    """nlx_bn254_verdict of the PLONK verifier: accepted, and for a rejected proof the first reason that applies and the field
    a malformed proof is named by"""
    _fields_ = [("accepted", ctypes.c_uint32), ("reason", ctypes.c_uint32), ("index", ctypes.c_uint32)]

    k = None      # the key's commitment count, set by VerifyingKey.verify_many: what the indices above 6 are counted from
    counts_off = False   # set there too: the bytes' length or one of their two counts does not fit the key (index 0 is then not L)

    def field_name(self):
        i, k = int(self.index), self.k
        if i == 0 and self.reason == VERIFY_MALFORMED and self.counts_off:
            return "the length or a count"
        if i < 7:
            return ("L", "R", "O", "Z", "H1", "H2", "H3")[i]
        if k is None:
            return "field %d" % i
        if i < 7 + k:
            return "PI2_%d" % (i - 7)
        if i < 9 + k:
            return ("the batched opening's H", "the shifted opening's H")[i - 7 - k]
        if i < 16 + 2 * k:
            return "claimed value %d" % (i - 9 - k)
        return "the shifted value"

    def __bool__(self):
        return bool(self.accepted)

    def __str__(self):
        if self.accepted:
            return "accepted"
        text = "rejected: " + _REASONS.get(int(self.reason), "reason %d" % self.reason)
        return text + (" at " + self.field_name() if self.reason == VERIFY_MALFORMED else "")

    def raise_if_rejected(self):
        if not self.accepted:
            from ._lib import NlxError
            raise NlxError(_NLX_E_INVAL, "PLONK proof " + str(self))
        return self


_G1_WORDS = B.bn254_g1_pack([(1, 2)])[0]


class VerifyingKey:
    """nlx_bn254_plonk_vk: gnark's plonk.VerifyingKey resident on the device (owns the handle; close() or the context's close()
    releases it).  k1, k2: integers; commitments: (8 + k, 8) G1Affine words in ResidentKey.key_commitments' order (s1 s2 s3 ql
    qr qm qo qk qcp_0 ..); commit_rows: the k rows i_j; g1: the SRS's first point (8 words; the generator by default); g2,
    g2_tau: [1]_2 and [tau]_2, 16 words each (batch.bn254_g2_pack)."""

    def __init__(self, ctx, log_n, n_public, k1, k2, commitments, commit_rows=(), g1=None, g2=None, g2_tau=None):
        from ._lib import NlxError, dll
        self.ctx, self.handle = ctx, None
        if g2 is None or g2_tau is None:
            raise ValueError("the key needs [1]_2 and [tau]_2")
        self.log_n, self.n_public = int(log_n), int(n_public)
        keep = {"commitments": np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)}
        self.k = len(keep["commitments"]) - 8
        if self.k < 0 or len(commit_rows) != self.k:
            raise ValueError("8 + k commitments and k commitment rows")
        for name, x in (("k1", k1), ("k2", k2)):
            x = int(x)
            if not 0 <= x < (1 << 256):
                raise NlxError(_NLX_E_RANGE, "%s does not fit four words" % name)
            keep[name] = B._fr_words(_to_mont(x) if x < R else x)   # r <= x < 2^256 is no residue: the library refuses its words
        rows = [int(i) for i in commit_rows]
        if any(not 0 <= i < (1 << 32) for i in rows) or not 0 <= self.log_n < (1 << 32) or not 0 <= self.n_public < (1 << 32):
            raise NlxError(_NLX_E_RANGE, "a row or a count does not fit 32 bits")
        keep["commit_rows"] = np.array(rows + [0], dtype=np.uint32)
        keep["g1"] = np.ascontiguousarray(_G1_WORDS if g1 is None else g1, dtype=np.uint64).reshape(8)
        keep["g2"] = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        keep["g2_tau"] = np.ascontiguousarray(g2_tau, dtype=np.uint64).reshape(16)
        d = _PlonkVkDesc()
        d.log_n, d.n_public, d.n_commit = self.log_n, self.n_public, self.k
        for name in ("k1", "k2", "commitments", "commit_rows", "g1", "g2", "g2_tau"):
            setattr(d, name, keep[name].ctypes.data)
        h = ctypes.c_void_p()
        ctx.check(dll.nlx_bn254_plonk_vk_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)

    @classmethod
    def from_resident(cls, key, g2, g2_tau, n_public, g1=None):
        """the verifying key of a ResidentKey: its 8 + k commitments (nlx_bn254_plonk_key_commitments), k1, k2 and commitment rows"""
        return cls(key.ctx, key.log_n, n_public, key.k1, key.k2, key.key_commitments(), [c["row"] for c in key.bsb22], g1=g1, g2=g2, g2_tau=g2_tau)

    def verify_many(self, proofs, publics):
        """One Verdict per proof.  proofs: the bytes of Proof.WriteTo; publics: per proof its n_public public inputs as integers.
        The whole batch is the same four launches as one proof.  An integer not below r raises NlxError (NLX_E_RANGE)."""
        from ._lib import NlxError, dll
        if not self.handle:
            raise NlxError(_NLX_E_INVAL, "the verifying key is closed")
        n = len(proofs)
        if len(publics) != n or any(len(p) != self.n_public for p in publics):
            raise ValueError("one list of n_public public inputs per proof")
        blobs = [bytes(p) for p in proofs]
        ptrs = (ctypes.c_char_p * max(n, 1))(*blobs)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in blobs])
        words = np.zeros((max(n * self.n_public, 1), 4), dtype=np.uint64)
        row = 0
        for p in publics:
            for x in p:
                x = int(x)
                if not 0 <= x < (1 << 256):
                    raise NlxError(_NLX_E_RANGE, "proof %d: a public input does not fit four words" % (row // max(self.n_public, 1)))
                m = _to_mont(x) if x < R else x               # r <= x < 2^256 is no residue: its words go as they are and the library refuses them
                for w in range(4):
                    words[row, w] = (m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
                row += 1
        verdicts = (Verdict * max(n, 1))()
        self.ctx.check(dll.nlx_bn254_plonk_verify_batch(self.handle, ptrs, lens, n, words.ctypes.data, verdicts))
        out = []
        for i in range(n):
            v = Verdict(verdicts[i].accepted, verdicts[i].reason, verdicts[i].index)
            v.k = self.k
            b, at = blobs[i], 260 + 32 * self.k
            v.counts_off = (len(b) != 552 + 64 * self.k or int.from_bytes(b[224:228], "big") != self.k
                            or int.from_bytes(b[at:at + 4], "big") != 7 + self.k)
            out.append(v)
        return out

    def verify(self, proof, public=()):
        """nlx_bn254_plonk_verify: one proof's Verdict"""
        return self.verify_many([proof], [list(public)])[0]

    def close(self):
        if self.handle and self.ctx.handle:
            from ._lib import dll
            dll.nlx_bn254_plonk_vk_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
