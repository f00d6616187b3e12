"""Cases of the Groth16 verifier shared by tests/test_bn254_pairing_model_cpu.py (the model's pairing verifier against the
trapdoor verifier) and tests/test_gpu_bn254_groth16_verify.py (the device's verifier against both): model keys, honest proofs
from prove_by_logs, and the named tampers with the verdict each must get."""
import os
import random
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_pairing_model as pm  # noqa: E402
import groth16_commit_model as cm  # noqa: E402
import groth16_model as gm  # noqa: E402

bn, R, Q = gm.bn, gm.R, gm.Q
ACCEPT, MALFORMED, PEDERSEN, PAIRING = 0, 1, 2, 3


class Case:
    """One key and one honest proof.  k = 0: tools/groth16_model.py; k > 0: tools/groth16_commit_model.py, commitment j
    holding j + 1 private wires."""

    def __init__(self, shape, n_constraints, k, seed):
        rng = random.Random(seed)
        self.k, self.shape, self.rng = k, shape, rng
        if k == 0:
            self.inst = gm.Instance(n_constraints, rng, **gm.SHAPES[shape])
            self.td = gm.Trapdoor.random(rng)
            self.pk, self.vk = gm.setup(self.inst, self.td)
            self.w = self.inst.witness
            self.pedersen = None
        else:
            # "empty" at 2^3 constraints: two idle rows leave too few wires for growing sets and for a dependent wire between
            # three commitments - one wire per set there
            small = shape == "empty" and n_constraints < 16
            counts = [1] * k if small else [j + 1 for j in range(k)]
            self.inst = cm.CommittedInstance(n_constraints, rng, counts, dependent=not small, **gm.SHAPES[shape])
            self.td = cm.Trapdoor.random(rng)
            self.pk, self.vk = cm.setup(self.inst, self.td)
            self.w = cm.solve(self.inst, td=self.td)
            self.pedersen = pm.pedersen_vk(self.td)
        self.r, self.s = rng.randrange(R), rng.randrange(R)
        self.public = list(self.w[1:self.inst.n_public])
        self.points = self.honest_points()
        self.proof = self.bytes_of(self.points)

    def honest_points(self):
        if self.k == 0:
            return list(gm.prove_by_logs(self.inst, self.td, self.w, self.r, self.s)) + [[], None]
        return list(cm.prove_by_logs(self.inst, self.td, self.w, self.r, self.s))

    @staticmethod
    def bytes_of(points):
        return cm.proof_bytes(points[0], points[1], points[2], points[3], points[4])

    def trapdoor_accepts(self, data, public=None):
        if self.k == 0:
            if len(data) != gm.PROOF_BYTES:
                return False
            return gm.verify_trapdoor(data, self.inst, self.td, self.w, self.r, self.s, public)
        return cm.verify_trapdoor(data, self.inst, self.td, self.w, self.r, self.s, public)

    def model_accepts(self, data, public=None):
        public = self.public if public is None else public
        if self.k == 0:
            return pm.groth16_verify(self.vk, self.pk, data, public)
        return pm.groth16_verify_committed(self.vk, self.pk, self.inst, self.pedersen, data, public)

    def hashed_positions(self):
        """PublicAndCommitmentCommitted as positions in vk["ic"]: a public wire's id, n_public + i for commitment i's wire"""
        wire_pos = {c["wire"]: self.inst.n_public + i for i, c in enumerate(self.inst.commitments)} if self.k else {}
        return [[wire_pos.get(i, i) for i in c["public"]] for c in self.inst.commitments] if self.k else []

    def verifying_key(self, nlx, ctx, **override):
        """the device's VerifyingKey for this case"""
        g2 = lambda p: nlx.bn254_g2_pack([p])[0]
        kw = dict(n_public=self.inst.n_public, g1_alpha=nlx.bn254_g1_pack([self.pk["g1_alpha"]])[0], g2_beta=g2(self.pk["g2_beta"]),
                  g2_gamma=g2(self.vk["g2_gamma"]), g2_delta=g2(self.pk["g2_delta"]), ic=nlx.bn254_g1_pack(self.vk["ic"]),
                  commitments=[{"public": p} for p in self.hashed_positions()],
                  pedersen=None if self.k == 0 else (g2(self.pedersen[0]), g2(self.pedersen[1])))
        kw.update(override)
        return nlx.bn254_groth16.VerifyingKey(ctx, **kw)

    # ---- the named tampers: (label, bytes, public inputs, reason, index) ----
    def with_point(self, index, point):
        pts = [self.points[0], self.points[1], self.points[2], list(self.points[3]), self.points[4]]
        if index < 3:
            pts[index] = point
        elif index < 3 + self.k:
            pts[3][index - 3] = point
        else:
            pts[4] = point
        return self.bytes_of(pts)

    def offset_of(self, index):
        return (0, 32, 96)[index] if index < 3 else 132 + 32 * (index - 3)

    def tampers(self):
        rng, k = self.rng, self.k
        other1 = lambda: gm.g1_gen_mul(rng.randrange(2, R))
        out = [("Ar replaced", self.with_point(0, other1()), self.public, PAIRING, 0),
               ("Krs replaced", self.with_point(2, other1()), self.public, PAIRING, 0),
               ("Bs replaced", self.with_point(1, gm.g2_gen_mul(rng.randrange(2, R))), self.public, PAIRING, 0)]
        if self.public:
            changed = list(self.public)
            changed[-1] = (changed[-1] + 1) % R
            out.append(("public input changed", self.proof, changed, PAIRING, 0))
        if k:
            out.append(("Pok replaced", self.with_point(3 + k, other1()), self.public, PEDERSEN, 0))
            out.append(("C_0 replaced", self.with_point(3, other1()), self.public, PEDERSEN, 0))
        out.append(("Bs outside the subgroup", self.with_point(1, pm.twist_point_outside_subgroup(rng)), self.public, MALFORMED, 1))
        # an x with no y: Krs's x walked upward until x^3 + 3 is no square, the flag bits kept
        data = bytearray(self.proof)
        x = self.points[2][0]
        while gm.fq_sqrt(x * x * x + 3) is not None:
            x += 1
        data[96:128] = x.to_bytes(32, "big")
        data[96] |= self.proof[96] & 0xC0
        out.append(("Krs: x with no y", bytes(data), self.public, MALFORMED, 2))
        # a coordinate >= q: Bs's X.A1 = q, and the last point's x = q
        data = bytearray(self.proof)
        data[32:64] = Q.to_bytes(32, "big")
        data[32] |= 0x80
        out.append(("Bs: X.A1 = q", bytes(data), self.public, MALFORMED, 1))
        last = 3 + k
        data = bytearray(self.proof)
        at = self.offset_of(last)
        data[at:at + 32] = Q.to_bytes(32, "big")
        data[at] |= 0x80
        out.append(("Pok: x = q", bytes(data), self.public, MALFORMED, last))
        out.append(("one byte short", self.proof[:-1], self.public, MALFORMED, 0))
        out.append(("one byte long", self.proof + b"\x00", self.public, MALFORMED, 0))
        data = bytearray(self.proof)
        data[128:132] = (k + 1).to_bytes(4, "big")
        out.append(("commitment count off by one", bytes(data), self.public, MALFORMED, 0))
        return out


_CASES = {}


def case(shape, n_constraints, k, seed=2600):
    key = (shape, n_constraints, k, seed)
    if key not in _CASES:
        _CASES[key] = Case(shape, n_constraints, k, seed + 7 * k + n_constraints)
    return _CASES[key]
