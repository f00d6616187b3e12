#!/usr/bin/env python3
"""PLONK over BN254 in gnark's proof shape WITH Bsb22 commitments ("commit to some wires, get a hash of the commitment back as a
wire": gnark's api.Commit), on big integers: an instance generator, a model prover that returns the proof's bytes, a parser for
any number of commitments and a trapdoor verifier (the pairing replaced by the test SRS's tau).  Test infrastructure, in the
manner of tools/bn128_config_model.py; field, group, NTT, transcript and KZG division come from the frozen oracle/bn254_py.py.

Status of every rule: RECALLED from gnark v0.9 backend/plonk/bn254 (prove.go, verify.go, setup.go) and gnark-crypto
(fr.Hash, kzg.BatchOpenSinglePoint), UNPINNED - there is no Go source and no gnark-produced vector to compare with (DESIGN.md
section 18).  Each rule is written once, here; with k = 0 commitments every byte equals bn254_py.gnark_plonk_prove_model's.

  rule 1  selectors     the key gains one selector qcp_j per commitment; on H the gate identity is
                        ql l + qr r + qm l r + qo o + qk + PI + sum_j qcp_j pi2_j = 0                        (quotient)
  rule 2  rows          commitment j has committed rows, ONE commitment row i_j and two blinding rows: i_j and the key-wide
                        last_row (gnark: the last constraint).  qcp_j = 1 on j's committed rows, 0 elsewhere (both blinding
                        rows included).  A committed row has ql = -1, qr = qm = qo = qk = 0 and the committed variable on L,
                        so pi2_j = l there.  The commitment row has ql = -1, the rest 0 and PI(w^i_j) = c_j, so l[i_j] = c_j
                                                                                                             (instance)
  rule 3  solving       in commitment order (gnark's solver hint): pi2_j takes l on j's committed rows, a blinding scalar on
                        row i_j, THEN one on last_row (if the two rows coincide the second assignment stands), 0 elsewhere;
                        [PI2_j] = KZG commitment of pi2_j (iNTT, MSM over the monomial SRS: the point gnark gets from its
                        Lagrange SRS); c_j = hash_to_field([PI2_j].Marshal(), dst "BSB22-Plonk"); the committed values of
                        commitment j may depend on c_0 .. c_{j-1}: the witness is completed between commitments
                                                                                                             (solve)
  rule 4  hash_to_field gnark-crypto fr.Hash(msg, dst, 1): RFC 9380 expand_message_xmd over SHA-256 to 48 bytes, big-endian,
                        mod r                                                                                (hash_to_field)
  rule 5  transcript    gamma binds S1 S2 S3 Ql Qr Qm Qo Qk, then every [Qcp_j], then the REAL public inputs (not the c_j),
                        then L R O; alpha binds [PI2_0] .. [PI2_{k-1}], then [Z]; beta and zeta as without commitments
                                                                                                             (_bind_key, prove)
  rule 6  quotient      the gate term gains sum_j qcp_j pi2_j; pi2_j is not blinded by multiples of X^n - 1; the degree
                        bound stays 3 n + 6 coefficients, h1 h2 h3 of n + 2                                  (quotient)
  rule 7  linearisation lin(X) gains sum_j qcp_j(zeta) pi2_j(X); the verifier's linearised digest uses [PI2_j] with the
                        scalars qcp_j(zeta)                                                                  (prove, verify)
  rule 8  opening       the batch at zeta appends the polynomials qcp_j, the digests [Qcp_j] and the claimed values
                        qcp_j(zeta): 7 + k claimed values, all of them in the combiner's hash                (prove, verify)
  rule 9  verifier      PI(zeta) gains sum_j c_j L_{i_j}(zeta), c_j recomputed from the proof's own points   (verify)
  rule 10 bytes         Proof.WriteTo: L R O Z H1 H2 H3 | k as uint32 big-endian, k compressed points | BatchedProof.H,
                        7 + k as uint32, the claimed values | ZShiftedOpening.H, its value                   (proof_bytes)
"""
import hashlib
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import bn254_py as bn  # noqa: E402

R = bn.R
BSB22_DST = b"BSB22-Plonk"
FIXED = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")
VK_ORDER = ("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk")


# ---- rule 4 ----
def expand_message_xmd(msg, dst, length):
    """RFC 9380 section 5.3.1 over SHA-256 (b_in_bytes = 32, s_in_bytes = 64)"""
    ell = (length + 31) // 32
    assert ell <= 255 and len(dst) <= 255
    dst_prime = bytes(dst) + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + bytes(msg) + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:length]


def hash_to_field(msg, dst=BSB22_DST):
    """fr.Hash(msg, dst, 1)[0]: L = 16 + 32 bytes, read big-endian, reduced mod r"""
    return int.from_bytes(expand_message_xmd(msg, dst, 48), "big") % R


# ---- rule 2: an instance ----
class Instance:
    """A satisfying circuit with k commitments.  Every wire cell holds a VARIABLE; the permutation is built from the cells'
    variables, so it does not depend on the c_j.  complete(cs) gives the wires once c_0 .. c_{len(cs)-1} are known (the
    unknown c_j stand as 0 until then)."""

    def __init__(self, log_n, k, rng, n_pi=0, chain=True, k1=5, k2=25, extra=2):
        n = self.n = 1 << log_n
        self.log_n, self.k, self.k1, self.k2 = log_n, k, k1, k2
        self.public_inputs = [rng.randrange(R) for _ in range(n_pi)]
        # the rows' roles: public rows first; last_row is an ordinary row when there is room, else the last commitment's row
        avail = list(range(n_pi, n))
        room = len(avail) - 2 * k
        if room < 0:
            raise ValueError("2^%d rows do not hold %d public rows and %d commitments" % (log_n, n_pi, k))
        self.last_row = n - 1
        last_is_commit_row = k > 0 and room == 0
        if avail:
            avail.remove(n - 1)
        room -= 0 if last_is_commit_row else 1
        rng.shuffle(avail)
        counts = [1] * k
        for j in range(k):
            more = min(room, rng.randrange(extra + 1))
            counts[j] += more
            room -= more
        self.commit_rows = [avail.pop() for _ in range(k - 1 if last_is_commit_row else k)] + ([n - 1] if last_is_commit_row else [])
        self.committed = []
        for j in range(k):
            self.committed.append(sorted(avail.pop() for _ in range(counts[j])))
        role = {}
        for j in range(k):
            role[self.commit_rows[j]] = ("commit", j)
            for i in self.committed[j]:
                role[i] = ("committed", j)
        # variables: a pool of free ones (random values, shared among cells), and C_j
        n_free = max(2, n // 2)
        self.values = [rng.randrange(R) for _ in range(n_free)]
        self.c_var = list(range(n_free, n_free + k))
        self.values += [0] * k
        pick = lambda: rng.randrange(n_free)
        self.cells = [[pick() for _ in range(n)] for _ in range(3)]
        for j in range(k):
            self.cells[0][self.commit_rows[j]] = self.c_var[j]
            if chain and j:
                self.cells[0][self.committed[j][0]] = self.c_var[j - 1]     # depth: commitment j covers c_{j-1}
        sel = {name: [0] * n for name in ("ql", "qr", "qm", "qo", "qk")}
        for i in range(n):
            if i in role:
                sel["ql"][i] = R - 1
                continue
            a, b, c = (self.values[self.cells[col][i]] for col in range(3))
            for name in ("ql", "qr", "qm", "qo"):
                sel[name][i] = rng.randrange(R)
            pub = self.public_inputs[i] if i < n_pi else 0
            sel["qk"][i] = -(sel["ql"][i] * a + sel["qr"][i] * b + sel["qm"][i] * a * b + sel["qo"][i] * c + pub) % R
        self.qcp = [[1 if role.get(i) == ("committed", j) else 0 for i in range(n)] for j in range(k)]
        w = bn.root_of_unity(log_n)
        ident = [[s * pow(w, i, R) % R for i in range(n)] for s in (1, k1, k2)]
        where = {}
        for col in range(3):
            for i in range(n):
                where.setdefault(self.cells[col][i], []).append((col, i))
        sigma = [[0] * n for _ in range(3)]
        for pos in where.values():
            for a, b in zip(pos, pos[1:] + pos[:1]):
                sigma[a[0]][a[1]] = ident[b[0]][b[1]]
        self.fixed = dict(sel, s1=sigma[0], s2=sigma[1], s3=sigma[2])

    def complete(self, cs):
        vals = list(self.values)
        for j, c in enumerate(cs):
            vals[self.c_var[j]] = int(c) % R
        return tuple([vals[v] for v in col] for col in self.cells)

    def key_values(self):
        """what a ProvingKey is built from: the eight fixed polynomials and qcp0 .. by values on H"""
        return dict(self.fixed, **{"qcp%d" % j: q for j, q in enumerate(self.qcp)})

    def commitment_info(self):
        return [{"committed": list(self.committed[j]), "row": self.commit_rows[j], "last_row": self.last_row} for j in range(self.k)]


# ---- rule 3 ----
def pi2_values(inst, j, l, b_row, b_last):
    v = [0] * inst.n
    for i in inst.committed[j]:
        v[i] = l[i]
    v[inst.commit_rows[j]] = int(b_row) % R
    v[inst.last_row] = int(b_last) % R
    return v


def committer(srs, tau=None):
    """coefficients -> the KZG commitment: the MSM over the SRS, or - the same point, one scalar multiplication instead of one
    per coefficient - p(tau) G when the caller hands over the test SRS's trapdoor"""
    if tau is None:
        return lambda c: bn.msm_g1(c, srs[:len(c)])
    return lambda c: bn.g1_mul(bn.eval_poly(c, tau), bn.G1)


def solve(inst, srs, commit_blinding, tau=None):
    """-> (wires l r o, [pi2_j values], [pi2_j coefficients], [[PI2_j]], [c_j])"""
    com = committer(srs, tau)
    cs, pi2, pi2_co, pts = [], [], [], []
    for j in range(inst.k):
        l, _, _ = inst.complete(cs)
        pi2.append(pi2_values(inst, j, l, commit_blinding[2 * j], commit_blinding[2 * j + 1]))
        pi2_co.append(bn.ntt(pi2[j], inverse=True))
        pts.append(com(pi2_co[j]))
        cs.append(hash_to_field(bn.g1_marshal(pts[j])))
    return inst.complete(cs), pi2, pi2_co, pts, cs


# ---- rules 1 and 6 ----
def quotient(co, n, shift, k1, k2, alpha, beta, gamma, k=0):
    """co: coefficient lists by name (fixed, l r o z - blinded or not -, optional pi, qcp0 .. pi20 ..) -> the 4 n coefficients of
    the quotient computed on the coset shift <w_4n>"""
    n4, log_n = 4 * n, n.bit_length() - 1
    ev = {}
    for name, c in co.items():
        s, pts = 1, []
        for j in range(n4):
            pts.append((int(c[j]) * s % R) if j < len(c) else 0)
            s = s * shift % R
        ev[name] = bn.ntt(pts)
    w4 = bn.root_of_unity(log_n + 2)
    t, x = [], shift
    for i in range(n4):
        l, r, o, z, zn = ev["l"][i], ev["r"][i], ev["o"][i], ev["z"][i], ev["z"][(i + 4) % n4]
        gate = ev["ql"][i] * l + ev["qr"][i] * r + ev["qm"][i] * l * r + ev["qo"][i] * o + ev["qk"][i] + (ev["pi"][i] if "pi" in ev else 0)
        for j in range(k):
            gate += ev["qcp%d" % j][i] * ev["pi2%d" % j][i]
        f = (l + beta * x + gamma) * (r + beta * k1 * x + gamma) % R * (o + beta * k2 * x + gamma) % R * z % R
        g = (l + beta * ev["s1"][i] + gamma) * (r + beta * ev["s2"][i] + gamma) % R * (o + beta * ev["s3"][i] + gamma) % R * zn % R
        zh = (pow(x, n, R) - 1) % R
        l1 = zh * pow(n * (x - 1) % R, R - 2, R) % R
        t.append((gate + alpha * (f - g) + alpha * alpha % R * l1 % R * (z - 1)) % R * pow(zh, R - 2, R) % R)
        x = x * w4 % R
    c = bn.ntt(t, inverse=True)
    sinv, s, out = pow(shift, R - 2, R), 1, []
    for j in range(n4):
        out.append(c[j] * s % R)
        s = s * sinv % R
    return out


def grand_product(l, r, o, fixed, n, beta, gamma, k1, k2):
    w = bn.root_of_unity(n.bit_length() - 1)
    z, acc, x = [], 1, 1
    for i in range(n):
        z.append(acc)
        num = (l[i] + beta * x + gamma) * (r[i] + beta * k1 * x + gamma) * (o[i] + beta * k2 * x + gamma) % R
        den = (l[i] + beta * fixed["s1"][i] + gamma) * (r[i] + beta * fixed["s2"][i] + gamma) * (o[i] + beta * fixed["s3"][i] + gamma) % R
        acc = acc * num % R * pow(den, R - 2, R) % R
        x = x * w % R
    assert acc == 1, "the wires do not respect the copy constraints"
    return z


# ---- rule 5 ----
def _bind_key(fs, vk, public_inputs):
    for name in VK_ORDER:
        fs.bind("gamma", bn.g1_marshal(vk[name]))
    for q in vk["qcp"]:
        fs.bind("gamma", bn.g1_marshal(q))
    for x in public_inputs:
        fs.bind("gamma", bn.fr_bytes(x))


def _batch_gamma(zeta, digests, claimed):
    fs = bn.GnarkTranscript("gamma")
    fs.bind("gamma", bn.fr_bytes(zeta))
    for d in digests:
        fs.bind("gamma", bn.g1_marshal(d))
    for v in claimed:
        fs.bind("gamma", bn.fr_bytes(v))
    return fs.challenge("gamma")


def _lin_scalars(l, r, o, s1, s2, zw, n, zeta, alpha, beta, gamma, k1, k2):
    """the linearised polynomial's coefficients on qm ql qr qo qk z s3 (rule 7 adds qcp_j(zeta) on pi2_j)"""
    zh = (pow(zeta, n, R) - 1) % R
    l1 = zh * pow(n * (zeta - 1) % R, R - 2, R) % R
    a_ = (l + beta * zeta + gamma) * (r + beta * k1 * zeta + gamma) % R * (o + beta * k2 * zeta + gamma) % R
    b_ = (l + beta * s1 + gamma) * (r + beta * s2 + gamma) % R
    return {"qm": l * r % R, "ql": l, "qr": r, "qo": o, "qk": 1, "z": (alpha * a_ + alpha * alpha % R * l1) % R,
            "s3": (-alpha * b_ % R * beta % R * zw) % R}, l1, b_


def verifying_key(inst, srs, tau=None):
    com = committer(srs, tau)
    vk = {name: com(bn.ntt(inst.fixed[name], inverse=True)) for name in FIXED}
    vk["qcp"] = [com(bn.ntt(q, inverse=True)) for q in inst.qcp]
    vk["commit_rows"] = list(inst.commit_rows)
    return vk


def prove(inst, srs, blinding=(0,) * 9, commit_blinding=None, tau=None):
    """-> (proof dict, bytes).  blinding: b for l (2), r (2), o (2), z (3); commit_blinding: 2 k scalars (row i_j, last_row);
    tau: the SRS's trapdoor, if the caller wants the commitments made the short way (committer)"""
    n, k, k1, k2 = inst.n, inst.k, inst.k1, inst.k2
    w, u = bn.root_of_unity(inst.log_n), k1
    com = committer(srs, tau)
    cb = [0] * (2 * k) if commit_blinding is None else [int(x) % R for x in commit_blinding]
    (l, r, o), pi2, pi2_co, pi2_pts, cs = solve(inst, srs, cb, tau)
    for j in range(k):
        assert l[inst.commit_rows[j]] == cs[j]
    co = {name: bn.ntt(inst.fixed[name], inverse=True) for name in FIXED}
    co.update(l=bn.ntt(l, inverse=True), r=bn.ntt(r, inverse=True), o=bn.ntt(o, inverse=True))
    qcp_co = [bn.ntt(q, inverse=True) for q in inst.qcp]
    vk = {name: com(co[name]) for name in FIXED}
    vk["qcp"] = [com(c) for c in qcp_co]
    pubs = list(inst.public_inputs)
    if pubs or k:
        pi_vals = [int(x) % R for x in pubs] + [0] * (n - len(pubs))
        for j in range(k):
            pi_vals[inst.commit_rows[j]] = cs[j]
        co["pi"] = bn.ntt(pi_vals, inverse=True)
    fs = bn.GnarkTranscript("gamma", "beta", "alpha", "zeta")
    _bind_key(fs, vk, pubs)
    b = [int(x) % R for x in blinding]
    bl = {"l": bn.blind_coeffs(co["l"], n, b[0:2]), "r": bn.blind_coeffs(co["r"], n, b[2:4]), "o": bn.blind_coeffs(co["o"], n, b[4:6])}
    proof = {"lro": [com(bl["l"]), com(bl["r"]), com(bl["o"])], "bsb22": pi2_pts}
    for c in proof["lro"]:
        fs.bind("gamma", bn.g1_marshal(c))
    gamma = fs.challenge("gamma")
    beta = fs.challenge("beta")
    z = grand_product(l, r, o, inst.fixed, n, beta, gamma, k1, k2)
    bl["z"] = bn.blind_coeffs(bn.ntt(z, inverse=True), n, b[6:9])
    proof["z"] = com(bl["z"])
    for c in pi2_pts:
        fs.bind("alpha", bn.g1_marshal(c))
    fs.bind("alpha", bn.g1_marshal(proof["z"]))
    alpha = fs.challenge("alpha")
    qco = dict(co)
    qco.update(bl)
    for j in range(k):
        qco["qcp%d" % j], qco["pi2%d" % j] = qcp_co[j], pi2_co[j]
    h = quotient(qco, n, u, k1, k2, alpha, beta, gamma, k)
    assert not any(h[3 * n + 6:]), "the witness does not satisfy the circuit"
    hs = [h[0:n + 2], h[n + 2:2 * n + 4], h[2 * n + 4:3 * n + 6]]
    proof["h"] = [com(c) for c in hs]
    for c in proof["h"]:
        fs.bind("zeta", bn.g1_marshal(c))
    zeta = fs.challenge("zeta")
    ev = {name: bn.eval_poly(bl[name], zeta) for name in ("l", "r", "o")}
    ev["s1"], ev["s2"] = bn.eval_poly(co["s1"], zeta), bn.eval_poly(co["s2"], zeta)
    qcp_z = [bn.eval_poly(c, zeta) for c in qcp_co]
    zw, zq = bn.kzg_open(bl["z"], zeta * w % R)
    proof["z_shifted"] = {"h": com(zq), "value": zw}
    sc, _, _ = _lin_scalars(ev["l"], ev["r"], ev["o"], ev["s1"], ev["s2"], zw, n, zeta, alpha, beta, gamma, k1, k2)
    src = {"qm": co["qm"], "ql": co["ql"], "qr": co["qr"], "qo": co["qo"], "qk": co["qk"], "z": bl["z"], "s3": co["s3"]}
    for j in range(k):
        sc["pi2%d" % j], src["pi2%d" % j] = qcp_z[j], pi2_co[j]
    m = n + 3
    lin = [sum(sc[name] * (src[name][i] if i < len(src[name]) else 0) for name in sc) % R for i in range(m)]
    zn2 = pow(zeta, n + 2, R)
    folded_h = [(hs[0][i] + zn2 * hs[1][i] + zn2 * zn2 % R * hs[2][i]) % R for i in range(n + 2)]
    polys = [folded_h, lin, bl["l"], bl["r"], bl["o"], co["s1"], co["s2"]] + qcp_co
    folded_h_digest = bn.g1_add(bn.g1_add(proof["h"][0], bn.g1_mul(zn2, proof["h"][1])), bn.g1_mul(zn2 * zn2 % R, proof["h"][2]))
    digests = [folded_h_digest, com(lin)] + proof["lro"] + [vk["s1"], vk["s2"]] + vk["qcp"]
    claimed = [bn.eval_poly(c, zeta) for c in polys]
    gp = _batch_gamma(zeta, digests, claimed)
    folded, g = [0] * m, 1
    for c in polys:
        for i, v in enumerate(c):
            folded[i] = (folded[i] + g * int(v)) % R
        g = g * gp % R
    _, q = bn.kzg_open(folded, zeta)
    proof["batched"] = {"h": com(q), "values": claimed}
    proof["quotient"], proof["c"] = h, cs      # not part of the bytes
    return proof, proof_bytes(proof)


# ---- rule 10 ----
def proof_bytes(proof):
    out = b"".join(bn.g1_compress(c) for c in proof["lro"]) + bn.g1_compress(proof["z"]) + b"".join(bn.g1_compress(c) for c in proof["h"])
    out += len(proof["bsb22"]).to_bytes(4, "big") + b"".join(bn.g1_compress(c) for c in proof["bsb22"])
    out += bn.g1_compress(proof["batched"]["h"]) + len(proof["batched"]["values"]).to_bytes(4, "big")
    out += b"".join(bn.fr_bytes(v) for v in proof["batched"]["values"])
    return out + bn.g1_compress(proof["z_shifted"]["h"]) + bn.fr_bytes(proof["z_shifted"]["value"])


def proof_length(k):
    return 7 * 32 + 4 + 32 * k + 32 + 4 + 32 * (7 + k) + 64


def proof_regions(k):
    """name -> (offset, length) of every part of the bytes"""
    reg, off = {}, 0
    for name in ("l", "r", "o", "z", "h1", "h2", "h3"):
        reg[name], off = (off, 32), off + 32
    reg["bsb22_count"], off = (off, 4), off + 4
    for j in range(k):
        reg["bsb22_%d" % j], off = (off, 32), off + 32
    reg["batched_h"], off = (off, 32), off + 32
    reg["claimed_count"], off = (off, 4), off + 4
    for name in ["folded_h", "lin", "l_zeta", "r_zeta", "o_zeta", "s1_zeta", "s2_zeta"] + ["qcp%d_zeta" % j for j in range(k)]:
        reg[name], off = (off, 32), off + 32
    reg["z_shifted_h"], off = (off, 32), off + 32
    reg["z_shifted_value"], off = (off, 32), off + 32
    assert off == proof_length(k)
    return reg


def proof_from_bytes(data):
    """any k; raises ValueError on bytes that are not a proof (a length that does not fit, a point off the curve, a value >= r)"""
    data = bytes(data)

    def point(off):
        if off + 32 > len(data):
            raise ValueError("truncated")
        try:
            return bn.g1_decompress(data[off:off + 32])
        except AssertionError:
            raise ValueError("not a point of the curve")

    def u32(off):
        if off + 4 > len(data):
            raise ValueError("truncated")
        return int.from_bytes(data[off:off + 4], "big")

    pts = [point(32 * i) for i in range(7)]
    off = 224
    k = u32(off)
    off += 4
    if k > (len(data) - off) // 32:
        raise ValueError("commitment count does not fit the length")
    bsb = [point(off + 32 * j) for j in range(k)]
    off += 32 * k
    bh = point(off)
    off += 32
    m = u32(off)
    off += 4
    if off + 32 * m + 64 != len(data):
        raise ValueError("claimed-value count does not fit the length")
    vals = [int.from_bytes(data[off + 32 * i:off + 32 * i + 32], "big") for i in range(m)]
    off += 32 * m
    zh = point(off)
    zv = int.from_bytes(data[off + 32:off + 64], "big")
    if any(v >= R for v in vals + [zv]):
        raise ValueError("a value is not below r")
    return {"lro": pts[0:3], "z": pts[3], "h": pts[4:7], "bsb22": bsb, "batched": {"h": bh, "values": vals},
            "z_shifted": {"h": zh, "value": zv}}


# ---- rules 7, 8, 9: the verifier, pairing replaced by the trapdoor ----
def verify_trapdoor(data, vk, n, tau, k1, k2, public_inputs=()):
    """vk: the eight commitments by name, "qcp": the list of [Qcp_j], "commit_rows": the rows i_j"""
    try:
        proof = proof_from_bytes(data)
    except ValueError:
        return False
    k = len(vk["qcp"])
    if len(proof["bsb22"]) != k or len(proof["batched"]["values"]) != 7 + k:
        return False
    w = bn.root_of_unity(n.bit_length() - 1)
    fs = bn.GnarkTranscript("gamma", "beta", "alpha", "zeta")
    _bind_key(fs, vk, public_inputs)
    for c in proof["lro"]:
        fs.bind("gamma", bn.g1_marshal(c))
    gamma, beta = fs.challenge("gamma"), fs.challenge("beta")
    for c in proof["bsb22"]:
        fs.bind("alpha", bn.g1_marshal(c))
    fs.bind("alpha", bn.g1_marshal(proof["z"]))
    alpha = fs.challenge("alpha")
    for c in proof["h"]:
        fs.bind("zeta", bn.g1_marshal(c))
    zeta = fs.challenge("zeta")
    vals = proof["batched"]["values"]
    folded_h_zeta, lin_zeta, l, r, o, s1, s2 = vals[:7]
    qcp_z = vals[7:]
    zw = proof["z_shifted"]["value"]
    sc, l1, b_ = _lin_scalars(l, r, o, s1, s2, zw, n, zeta, alpha, beta, gamma, k1, k2)
    zh = (pow(zeta, n, R) - 1) % R
    lagrange = lambda i: pow(w, i, R) * zh % R * pow(n * (zeta - pow(w, i, R)) % R, R - 2, R) % R
    pi = 0
    for i, x in enumerate(public_inputs):
        pi = (pi + int(x) * lagrange(i)) % R
    for j in range(k):
        pi = (pi + hash_to_field(bn.g1_marshal(proof["bsb22"][j])) * lagrange(vk["commit_rows"][j])) % R
    if (lin_zeta + pi - alpha * b_ % R * (o + gamma) % R * zw - alpha * alpha % R * l1) % R != folded_h_zeta * zh % R:
        return False
    pts = {"qm": vk["qm"], "ql": vk["ql"], "qr": vk["qr"], "qo": vk["qo"], "qk": vk["qk"], "z": proof["z"], "s3": vk["s3"]}
    names = list(sc)
    lin_digest = bn.msm_g1([sc[x] for x in names] + qcp_z, [pts[x] for x in names] + proof["bsb22"])
    zn2 = pow(zeta, n + 2, R)
    folded_h_digest = bn.g1_add(bn.g1_add(proof["h"][0], bn.g1_mul(zn2, proof["h"][1])), bn.g1_mul(zn2 * zn2 % R, proof["h"][2]))
    digests = [folded_h_digest, lin_digest] + proof["lro"] + [vk["s1"], vk["s2"]] + vk["qcp"]
    gp = _batch_gamma(zeta, digests, vals)
    acc, g = None, 1
    for d, v in zip(digests, vals):
        acc = bn.g1_add(acc, bn.g1_mul(g, bn.g1_add(d, bn.g1_neg(bn.g1_mul(v, bn.G1)))))
        g = g * gp % R
    rhs = bn.g1_mul((tau - zeta) % R, proof["batched"]["h"]) if proof["batched"]["h"] is not None else None
    if acc != rhs:
        return False
    lhs2 = bn.g1_add(proof["z"], bn.g1_neg(bn.g1_mul(zw, bn.G1)))
    rhs2 = bn.g1_mul((tau - zeta * w) % R, proof["z_shifted"]["h"]) if proof["z_shifted"]["h"] is not None else None
    return lhs2 == rhs2


if __name__ == "__main__":
    import random
    rng = random.Random(1)
    for k in (0, 1, 2):
        inst = Instance(4, k, rng, n_pi=2)
        tau = rng.randrange(1, R)
        srs = bn.kzg_srs(tau, inst.n + 3)
        _, data = prove(inst, srs, [rng.randrange(R) for _ in range(9)], [rng.randrange(R) for _ in range(2 * k)])
        print("k = %d: %d bytes, verifier %s" % (k, len(data), verify_trapdoor(data, verifying_key(inst, srs), inst.n, tau, inst.k1, inst.k2, inst.public_inputs)))
