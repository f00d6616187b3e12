#!/usr/bin/env python3
"""Groth16 over BN254 with gnark's Bsb22 / Pedersen commitments, on big integers: what tools/groth16_model.py is for keys
without commitments, for keys with them.  Fields, points, `Instance`, the G2 code and compression come from groth16_model;
this file adds an instance builder that places commitments into an R1CS, the setup with a trapdoor extended by sigma, the
solver's hint, an honest prover (from the key's points and from discrete logs), Proof.WriteTo's 164 + 32 k bytes with their
parser, and the verifier in the exponent.

Status of every rule: RECALLED from gnark v0.9 (backend/groth16/bn254 setup.go, prove.go, verify.go, marshal.go;
constraint/commitment.go; gnark-crypto ecc/bn254/fr/pedersen), UNPINNED - there is no Go source and no gnark-produced vector to
compare with.  Each rule is written once, here; this file is the place of record.

Commitment j of k has PrivateCommitted_j (private wire ids, ascending; the sets are pairwise disjoint),
PublicAndCommitmentCommitted_j (public wires and earlier commitments' wires) and CommitmentIndex_j (the wire that receives the
challenge).  M = sum_j |PrivateCommitted_j|.

  rule 1  setup      the wires of every PrivateCommitted_j and every CommitmentIndex_j leave G1.K, which keeps
                     n_wires - n_public - M - k points; their K-polynomials are divided by gamma instead of delta; the private
                     committed ones are the Pedersen Basis_j, BasisExpSigma_j = sigma Basis_j with ONE sigma for all k keys; the
                     commitment wires' points join the verifying key's K after the public wires                    (setup)
  rule 2  hint       while the witness is solved (later wires do not exist yet): C_j = sum_i w[PrivateCommitted_j[i]] Basis_j[i];
                     w[CommitmentIndex_j] = fr.Hash(C_j.Marshal() || the PublicAndCommitmentCommitted_j values, 32 bytes
                     big-endian each, dst "bsb22-commitment", 1)[0]; Marshal() = 64 uncompressed bytes; fr.Hash = RFC 9380
                     expand_message_xmd over SHA-256 to 48 bytes, read big-endian, mod r
                                                                           (commit, commitment_challenge, hash_to_field, solve)
  rule 3  PoK        pedersen.BatchProve: rho = fr.Hash(the k commitment-wire values, 32 bytes big-endian each, "G16-BSB22",
                     1)[0]; Pok = sum_j rho^j sum_i w[PrivateCommitted_j[i]] BasisExpSigma_j[i]; for k = 1 this is
                     ProveKnowledge (rho^0 = 1: rho is not used)                                                (fold_challenge, prove)
  rule 4  Krs        the G1.K sum runs over the remaining private wires only; Ar, Bs, h, G1.Z and the blinding tail are those of
                     groth16_model; the prover does NOT add C_j to Krs (the verifier adds them to the public sum)  (prove)
  rule 5  bytes      Proof.WriteTo: Ar (32), Bs (64), Krs (32) compressed, uint32 big-endian k, k compressed C_j, compressed Pok:
                     164 + 32 k bytes; k = 0 gives groth16_model's 164                              (proof_bytes, proof_from_bytes)
  rule 6  verifier   recompute each commitment-wire value from the proof's C_j and the public inputs; check
                     e(Ar, Bs) = e(alpha, beta) e(sum_(public and commitment wires) w_i K_i + sum_j C_j, gamma) e(Krs, delta)
                     and the Pedersen equation e(sum_j rho^j C_j, [-1/sigma]_2) e(Pok, [1]_2) = 1              (verify_trapdoor)
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import groth16_model as gm  # noqa: E402

bn = gm.bn
R, Q = gm.R, gm.Q
inv = gm.inv
COMMITMENT_DST = b"bsb22-commitment"
FOLD_DST = b"G16-BSB22"


def hash_to_field(msg, dst):
    """gnark-crypto fr.Hash(msg, dst, 1)[0] (rule 2)"""
    dst_prime = bytes(dst) + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + bytes(msg) + (48).to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b1 = hashlib.sha256(b0 + b"\x01" + dst_prime).digest()
    b2 = hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dst_prime).digest()
    return int.from_bytes((b1 + b2)[:48], "big") % R


def fr_bytes(x):
    return (int(x) % R).to_bytes(32, "big")


# ---- an instance with commitments ----
class CommittedInstance(gm.Instance):
    """groth16_model's random R1CS of one of its shapes, post-processed: k of its defining constraints give their new wire away
    to a commitment (the constraint keeps its A row and loses B and C: it holds for every value, and the wire becomes what a
    solver's hint fills in), and the next defining constraint, where there is one, gets that wire into its A row - so everything
    defined after it depends on the challenge.  Every wire is still either free (ONE, public, secret), a commitment wire, or
    defined by one constraint in order: solve() walks the constraints front to back.

    private_counts   |PrivateCommitted_j| for each commitment; 0 gives the empty set (C_j = the point at infinity)
    hashed_public    how many public wires (the constant wire included) each PublicAndCommitmentCommitted_j holds; every
                     EARLIER commitment's wire is hashed too
    dependent        commitment j > 0 with a non-empty set commits the internal wire defined right after commitment j - 1's
                     wire, whose value depends on that challenge
    secret_only      the sets (but for the dependent wire) are drawn from the secret wires, whose values a test may choose
    The witness exists only after solve(); `free` holds the values of the free wires and may be changed before it."""

    def __init__(self, n_constraints, rng, private_counts, hashed_public=1, dependent=True, secret_only=False, **shape):
        super().__init__(n_constraints, rng, **shape)
        k = len(private_counts)
        n_free = self.n_public + shape.get("n_secret", 3)
        self.n_free, self.free = n_free, list(self.witness[:n_free])
        rows = self.rows
        nonzero = [i for i, v in enumerate(self.coeffs) if v]
        self.defines = {}                                   # constraint -> (its new wire, the coefficient id it carries in C)
        for j, rc in enumerate(rows["C"]):
            if rc:
                new = max(i for i, _ in rc)
                self.defines[j] = (new, [c for i, c in rc if i == new][0])
        defs = sorted(self.defines)
        assert len(defs) >= k, "one defining constraint per commitment"
        at = [defs[(j + 1) * len(defs) // (k + 1)] for j in range(k)]     # spread out, defining constraints in between
        self.commit_at = {}                                  # constraint -> commitment
        self.commitments = []
        taken = set()
        for j, row in enumerate(at):
            wire = self.defines.pop(row)[0]
            rows["B"][row], rows["C"][row] = [], []
            self.commit_at[row] = j
            later = [d for d in defs if d > row and d not in at]
            follower = None
            if later and (j + 1 == k or later[0] < at[j + 1]):
                follower = later[0]
                rows["A"][follower] = rows["A"][follower] + [(wire, nonzero[rng.randrange(len(nonzero))])]
            self.commitments.append({"wire": wire, "follower": follower})
        wires_c = set(c["wire"] for c in self.commitments)
        for j, c in enumerate(self.commitments):
            count, forced = private_counts[j], []
            if dependent and j > 0 and count > 0:
                f = self.commitments[j - 1]["follower"]
                assert f is not None, "no defining constraint between commitments %d and %d" % (j - 1, j)
                forced = [self.defines[f][0]]
            top = min(c["wire"], n_free) if secret_only else c["wire"]
            pool = [i for i in range(self.n_public, top) if i not in wires_c and i not in taken and i not in forced]
            assert len(pool) >= count - len(forced), "commitment %d: %d private wires wanted, %d free to commit" % (j, count, len(pool))
            c["private"] = sorted(forced + rng.sample(pool, count - len(forced)))
            taken.update(c["private"])
            publics = sorted(rng.sample(range(self.n_public), min(hashed_public, self.n_public)))
            c["public"] = publics + [e["wire"] for e in self.commitments[:j]]
        self.k, self.n_committed = k, sum(private_counts)
        self.witness = None
        self.csr = {}
        for name in "ABC":
            row_ptr, wire, cid = [0], [], []
            for r_ in rows[name]:
                wire += [i for i, _ in r_]
                cid += [c_ for _, c_ in r_]
                row_ptr.append(len(wire))
            self.csr[name] = (row_ptr, wire, cid)

    def k_wires(self):
        """the private wires G1.K keeps (rule 1), ascending"""
        out = set(c["wire"] for c in self.commitments)
        for c in self.commitments:
            out.update(c["private"])
        return [i for i in range(self.n_public, self.n_wires) if i not in out]

    def solve(self, challenge, upto=None):
        """The witness, front to back.  challenge(j, w) -> the value of commitment j's wire; w holds every wire solved so far
        (None elsewhere) - the solver's hint (rule 2).  upto = j: stop before commitment j's hint and return the partial w."""
        w = self.free + [None] * (self.n_wires - self.n_free)
        val = lambda terms: sum(self.coeffs[c] * w[i] for i, c in terms) % R
        for row in range(self.n_constraints):
            if row in self.commit_at:
                j = self.commit_at[row]
                if upto == j:
                    return w
                w[self.commitments[j]["wire"]] = int(challenge(j, w)) % R
            elif row in self.defines:
                new, kid = self.defines[row]
                rest = [(i, c) for i, c in self.rows["C"][row] if i != new]
                w[new] = (val(self.rows["A"][row]) * val(self.rows["B"][row]) - val(rest)) * inv(self.coeffs[kid]) % R
        assert None not in w
        self.witness = w
        return w


# ---- rule 1: setup ----
class Trapdoor(gm.Trapdoor):
    def __init__(self, tau, alpha, beta, gamma, delta, sigma):
        super().__init__(tau, alpha, beta, gamma, delta)
        self.sigma = int(sigma) % R

    @classmethod
    def random(cls, rng):
        return cls(*(rng.randrange(2, R) for _ in range(6)))


def k_logs(inst, td):
    """beta A_i(tau) + alpha B_i(tau) + C_i(tau) for every wire"""
    at, bt, ct = gm.wire_polys_at(inst, td.tau)
    return [(td.beta * at[i] + td.alpha * bt[i] + ct[i]) % R for i in range(inst.n_wires)]


def setup(inst, td):
    """gnark's ProvingKey with its CommitmentKeys (dict "pk"; pk["commitments"][j] = private, public, wire, basis,
    basis_exp_sigma) and what the verifier needs (dict "vk": ic over the public wires THEN the commitment wires)"""
    pk, vk = gm.setup(inst, td)
    kept = inst.k_wires()
    pk["g1_k"] = [pk["g1_k"][i - inst.n_public] for i in kept]          # the others were divided by delta: dropped (rule 1)
    k_all, ginv = k_logs(inst, td), inv(td.gamma)
    pk["commitments"] = []
    for c in inst.commitments:
        logs = [k_all[i] * ginv % R for i in c["private"]]
        pk["commitments"].append({"private": list(c["private"]), "public": list(c["public"]), "wire": c["wire"],
                                  "basis": [gm.g1_gen_mul(x) for x in logs],
                                  "basis_exp_sigma": [gm.g1_gen_mul(x * td.sigma) for x in logs]})
        vk["ic"].append(gm.g1_gen_mul(k_all[c["wire"]] * ginv))
    return pk, vk


# ---- rule 2: the solver's hint ----
def commit(pk, j, w):
    """C_j from the key's points; w needs only PrivateCommitted_j filled"""
    c = pk["commitments"][j]
    return bn.msm_g1([w[i] for i in c["private"]], c["basis"])


def commit_log(inst, td, j, w):
    """C_j's discrete log"""
    k_all, ginv = k_logs(inst, td), inv(td.gamma)
    return sum(w[i] * k_all[i] for i in inst.commitments[j]["private"]) % R * ginv % R


def commitment_challenge(point, hashed_values):
    return hash_to_field(bn.g1_marshal(point) + b"".join(fr_bytes(v) for v in hashed_values), COMMITMENT_DST)


def solve(inst, pk=None, td=None):
    """the instance's witness with every commitment wire filled by its hint; from the key's points, or from the trapdoor"""
    def challenge(j, w):
        point = commit(pk, j, w) if td is None else gm.g1_gen_mul(commit_log(inst, td, j, w))
        return commitment_challenge(point, [w[i] for i in inst.commitments[j]["public"]])
    return inst.solve(challenge)


# ---- rules 3 and 4: the prover ----
def fold_challenge(wire_values):
    return hash_to_field(b"".join(fr_bytes(v) for v in wire_values), FOLD_DST)


def prove(inst, pk, witness, r, s, rho=None):
    """(Ar, Bs, Krs, [C_j], Pok) as affine points from the key's POINTS.  rho: override the folding challenge (tests)."""
    assert witness[0] == 1 and len(witness) == inst.n_wires
    a, b, c = inst.abc(witness)
    h = bn.groth16_quotient(a, b, c, gm.COSET_SHIFT)
    wa = [witness[i] for i in range(inst.n_wires) if not pk["infinity_a"][i]]
    wb = [witness[i] for i in range(inst.n_wires) if not pk["infinity_b"][i]]
    ar = bn.g1_add(bn.g1_add(bn.msm_g1(wa, pk["g1_a"]), pk["g1_alpha"]), bn.g1_mul(r, pk["g1_delta"]))
    bs1 = bn.g1_add(bn.g1_add(bn.msm_g1(wb, pk["g1_b"]), pk["g1_beta"]), bn.g1_mul(s, pk["g1_delta"]))
    bs = bn.g2_add(bn.g2_add(gm.msm_g2(wb, pk["g2_b"]), pk["g2_beta"]), gm.g2_mul(s, pk["g2_delta"]))
    kept = inst.k_wires()
    assert len(kept) == len(pk["g1_k"])
    krs = bn.g1_add(bn.msm_g1([witness[i] for i in kept], pk["g1_k"]), bn.msm_g1(h[:inst.n - 1], pk["g1_z"]))   # rule 4
    krs = bn.g1_add(krs, bn.g1_mul(s, ar))
    krs = bn.g1_add(krs, bn.g1_mul(r, bs1))
    krs = bn.g1_add(krs, bn.g1_neg(bn.g1_mul(r * s % R, pk["g1_delta"])))
    cs = [commit(pk, j, witness) for j in range(inst.k)]
    if rho is None:
        rho = fold_challenge([witness[c_["wire"]] for c_ in pk["commitments"]])
    pok, power = None, 1
    for c_ in pk["commitments"]:                                                                               # rule 3
        pok = bn.g1_add(pok, bn.msm_g1([witness[i] * power % R for i in c_["private"]], c_["basis_exp_sigma"]))
        power = power * rho % R
    return ar, bs, krs, cs, pok


def proof_logs(inst, td, witness, r, s, rho=None):
    """the discrete logs of an honest proof's Ar, Bs, Krs, every C_j and Pok"""
    at, bt, ct = gm.wire_polys_at(inst, td.tau)
    A = sum(w * x for w, x in zip(witness, at)) % R
    B = sum(w * x for w, x in zip(witness, bt)) % R
    C = sum(w * x for w, x in zip(witness, ct)) % R
    a = (A + td.alpha + r * td.delta) % R
    b = (B + td.beta + s * td.delta) % R
    priv = sum(witness[i] * (td.beta * at[i] + td.alpha * bt[i] + ct[i]) for i in inst.k_wires()) % R
    c = ((priv + A * B - C) * inv(td.delta) + s * a + r * b - r * s % R * td.delta) % R
    ginv = inv(td.gamma)
    cs = [sum(witness[i] * (td.beta * at[i] + td.alpha * bt[i] + ct[i]) for i in c_["private"]) % R * ginv % R for c_ in inst.commitments]
    if rho is None:
        rho = fold_challenge([witness[c_["wire"]] for c_ in inst.commitments])
    pok = sum(pow(rho, j, R) * x for j, x in enumerate(cs)) % R * td.sigma % R
    return a, b, c, cs, pok


def prove_by_logs(inst, td, witness, r, s, rho=None):
    """the same points as prove(), from the trapdoor: 3 + k + 1 fixed-base multiples"""
    a, b, c, cs, pok = proof_logs(inst, td, witness, r, s, rho)
    return gm.g1_gen_mul(a), gm.g2_gen_mul(b), gm.g1_gen_mul(c), [gm.g1_gen_mul(x) for x in cs], gm.g1_gen_mul(pok)


# ---- rule 5: bytes ----
def proof_bytes(ar, bs, krs, commitments=(), pok=None):
    out = bn.g1_compress(ar) + gm.g2_compress(bs) + bn.g1_compress(krs) + len(commitments).to_bytes(4, "big")
    return out + b"".join(bn.g1_compress(c) for c in commitments) + bn.g1_compress(pok)


def _g1_decompress(data):
    if data[0] >> 6 == 1:
        assert data[0] == 0x40 and not any(data[1:])
        return None
    assert data[0] >> 6 in (2, 3), "not a compressed point"
    p = bn.g1_decompress(data)
    assert p[0] < Q
    return p


def proof_from_bytes(data):
    """(Ar, Bs, Krs, [C_j], Pok)"""
    assert len(data) >= gm.PROOF_BYTES
    k = int.from_bytes(data[128:132], "big")
    assert len(data) == gm.PROOF_BYTES + 32 * k
    cs = [_g1_decompress(data[132 + 32 * j:164 + 32 * j]) for j in range(k)]
    return _g1_decompress(data[0:32]), gm.g2_decompress(data[32:96]), _g1_decompress(data[96:128]), cs, _g1_decompress(data[132 + 32 * k:])


# ---- rule 6: the verifier, in the exponent ----
def verify_trapdoor(data, inst, td, witness, r, s, public=None, logs=None):
    """The verifier's two checks on the proof BYTES with the setup's trapdoor in place of the pairings.  The commitment wires'
    values are RECOMPUTED from the bytes' C_j and the public inputs (`public`: wires 1 .. n_public - 1 as the verifier holds
    them; by default the witness's own), never taken from the witness.  The witness and r, s only serve to find the discrete
    logs of Ar, Bs, Krs and C_j, which the pairing equation is checked on (points that are not those multiples of the
    generators: rejected); logs = (a, b, c): the logs of Ar, Bs, Krs where a test crafted those points itself.  The Pedersen
    equation needs no logs: with sigma in hand it says Pok = sigma sum_j rho^j C_j."""
    try:
        ar, bs, krs, cs, pok = proof_from_bytes(data)
    except (AssertionError, ValueError):
        return False
    if len(cs) != inst.k:
        return False
    v = {i: witness[i] for i in range(inst.n_public)}                    # what the verifier knows: wire -> value
    if public is not None:
        assert len(public) == inst.n_public - 1
        v.update({i + 1: int(x) % R for i, x in enumerate(public)})
    for j, c_ in enumerate(inst.commitments):                             # public and EARLIER commitment wires only
        v[c_["wire"]] = commitment_challenge(cs[j], [v[i] for i in c_["public"]])
    rho = fold_challenge([v[c_["wire"]] for c_ in inst.commitments]) if inst.k else 0
    folded, power = None, 1
    for c_point in cs:
        folded = bn.g1_add(folded, bn.g1_mul(power, c_point))
        power = power * rho % R
    if pok != bn.g1_mul(td.sigma, folded):
        return False
    a, b, c, c_logs, _ = proof_logs(inst, td, witness, r, s)
    if logs is not None:
        a, b, c = logs
    if ar != gm.g1_gen_mul(a) or bs != gm.g2_gen_mul(b) or krs != gm.g1_gen_mul(c):
        return False
    if any(p != gm.g1_gen_mul(x) for p, x in zip(cs, c_logs)):
        return False
    k_all = k_logs(inst, td)
    ic = sum(val * k_all[i] for i, val in v.items()) % R * inv(td.gamma) % R
    return a * b % R == (td.alpha * td.beta + (ic + sum(c_logs)) * td.gamma + c * td.delta) % R


if __name__ == "__main__":
    import random
    rng = random.Random(21)
    for name, counts in (("common", [3]), ("public3", [2, 0, 3]), ("empty", [4, 2]), ("unit", [1, 1, 1])):
        inst = CommittedInstance(16, rng, counts, **gm.SHAPES[name])
        td = Trapdoor.random(rng)
        pk, vk = setup(inst, td)
        w = solve(inst, pk)
        assert inst.satisfied(w) and w == solve(inst, td=td)
        r, s = rng.randrange(R), rng.randrange(R)
        pts = prove(inst, pk, w, r, s)
        assert pts == prove_by_logs(inst, td, w, r, s)
        data = proof_bytes(*pts)
        assert verify_trapdoor(data, inst, td, w, r, s)
        print("%-8s %d constraints, %d wires, committed sets %r: %d-byte proof verifies" % (name, inst.n_constraints, inst.n_wires, counts, len(data)))
