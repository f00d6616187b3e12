"""Cases of the PLONK verifier over BN254 shared by tests/test_gnark_plonk_verify_model_cpu.py (the model with real pairings,
tools/gnark_plonk_verify_model.py, against the trapdoor verifier) and tests/test_gpu_bn254_plonk_verify.py (the device's
verifier against both): model instances, honest proofs from gnark_bsb22_model.prove, and the named tampers.  The verdict a
tamper must get is whatever the model with pairings gives (computed once per case); the table also records what the issue of
the verifier expects of each, and the tests check that the two agree where the issue is definite."""
import os
import random
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnark_bsb22_model as gm  # noqa: E402
import gnark_plonk_verify_model as vm  # noqa: E402

bn, pm = vm.bn, vm.pm
R, Q = bn.R, bn.Q
ACCEPT, MALFORMED, PAIRING, ALGEBRAIC = vm.ACCEPT, vm.MALFORMED, vm.PAIRING, vm.ALGEBRAIC


class Case:
    """One instance, its keys and one honest proof"""

    def __init__(self, log_n, k, n_pi, seed):
        rng = self.rng = random.Random(seed)
        self.log_n, self.k = log_n, k
        self.inst = gm.Instance(log_n, k, rng, n_pi=n_pi)
        self.n = self.inst.n
        self.tau = rng.randrange(1, R)
        self.srs = bn.kzg_srs(self.tau, self.n + 3)
        self.vk = gm.verifying_key(self.inst, self.srs, self.tau)
        self.g2, self.g2_tau = vm.g2_pair(self.tau)
        self.public = list(self.inst.public_inputs)
        self.blinding = [rng.randrange(R) for _ in range(9)]
        self.commit_blinding = [rng.randrange(R) for _ in range(2 * k)]
        self.parts, self.proof = gm.prove(self.inst, self.srs, self.blinding, self.commit_blinding, tau=self.tau)
        self.reg = gm.proof_regions(k)
        self._verdicts = {}

    def trapdoor_accepts(self, data, public=None):
        return gm.verify_trapdoor(data, self.vk, self.n, self.tau, self.inst.k1, self.inst.k2, self.public if public is None else public)

    def model_verdict(self, data, public=None):
        """(accepted, reason, index) of the model with pairings, remembered"""
        public = self.public if public is None else list(public)
        key = (bytes(data), tuple(public))
        if key not in self._verdicts:
            a, reason, index = vm.verify(data, self.vk, self.n, self.inst.k1, self.inst.k2, public, self.g2, self.g2_tau)
            self._verdicts[key] = (int(a), reason, index)
        return self._verdicts[key]

    def key_commitments(self):
        return [self.vk[name] for name in gm.VK_ORDER] + list(self.vk["qcp"])

    def verifying_key(self, nlx, ctx, **override):
        """the device's VerifyingKey for this case"""
        g2 = lambda p: nlx.bn254_g2_pack([p])[0]
        kw = dict(log_n=self.log_n, n_public=len(self.public), k1=self.inst.k1, k2=self.inst.k2,
                  commitments=nlx.bn254_g1_pack(self.key_commitments()), commit_rows=list(self.vk["commit_rows"]),
                  g1=nlx.bn254_g1_pack([bn.G1])[0], g2=g2(self.g2), g2_tau=g2(self.g2_tau))
        kw.update(override)
        return nlx.bn254_plonk.VerifyingKey(ctx, **kw)

    # ---- the named tampers: (label, bytes, public inputs, the reason the issue expects or None, the index or None) ----
    def with_bytes(self, name, new):
        off, length = self.reg[name]
        assert len(new) == length
        return self.proof[:off] + bytes(new) + self.proof[off + length:]

    def with_value(self, name, delta=1):
        off, _ = self.reg[name]
        v = (int.from_bytes(self.proof[off:off + 32], "big") + delta) % R
        return self.with_bytes(name, v.to_bytes(32, "big"))

    def tampers(self):
        rng, k, reg = self.rng, self.k, self.reg
        other = lambda: bn.g1_compress(bn.g1_mul(rng.randrange(2, R), bn.G1))
        out = [("batched H replaced", self.with_bytes("batched_h", other()), self.public, PAIRING, 0),
               ("shifted H replaced", self.with_bytes("z_shifted_h", other()), self.public, PAIRING, 0),
               ("L replaced", self.with_bytes("l", other()), self.public, None, None),          # L enters the transcript: the model decides
               ("l_zeta + 1", self.with_value("l_zeta"), self.public, ALGEBRAIC, 0),
               ("shifted value + 1", self.with_value("z_shifted_value"), self.public, ALGEBRAIC, 0)]
        if k:
            out.append(("PI2_0 replaced", self.with_bytes("bsb22_0", other()), self.public, ALGEBRAIC, 0))
        # an x with no y: H2's x walked upward until x^3 + 3 is no square, the flag bits kept
        off = reg["h2"][0]
        x = int.from_bytes(bytes([self.proof[off] & 0x3F]) + self.proof[off + 1:off + 32], "big")
        while pow((x * x * x + 3) % Q, (Q - 1) // 2, Q) == 1:
            x += 1
        b = bytearray(x.to_bytes(32, "big"))
        b[0] |= self.proof[off] & 0xC0
        out.append(("H2: x with no y", self.with_bytes("h2", b), self.public, MALFORMED, 5))
        b = bytearray(Q.to_bytes(32, "big"))
        b[0] |= 0x80
        out.append(("Z: x = q", self.with_bytes("z", b), self.public, MALFORMED, 3))
        for i, name in ((2, "l_zeta"), (6 + k, "s2_zeta" if k == 0 else "qcp%d_zeta" % (k - 1))):
            out.append(("claimed value %d = r" % i, self.with_bytes(name, R.to_bytes(32, "big")), self.public, MALFORMED, 9 + k + i))
        out.append(("one byte short", self.proof[:-1], self.public, MALFORMED, 0))
        out.append(("one byte long", self.proof + b"\x00", self.public, MALFORMED, 0))
        out.append(("commitment count off by one", self.with_bytes("bsb22_count", (k + 1).to_bytes(4, "big")), self.public, MALFORMED, 0))
        out.append(("claimed-value count off by one", self.with_bytes("claimed_count", (8 + k).to_bytes(4, "big")), self.public, MALFORMED, 0))
        same = self.proof[reg["l"][0]:reg["l"][0] + 32]
        out.append(("L = R = O", same * 3 + self.proof[96:], self.public, None, None))
        return out

    def bit_flips(self, count, seed):
        rng = random.Random(seed)
        out = []
        for _ in range(count):
            data = bytearray(self.proof)
            bit = rng.randrange(8 * len(data))
            data[bit >> 3] ^= 1 << (bit & 7)
            out.append((bit, bytes(data)))
        return out


def parser_refuses(data):
    try:
        gm.proof_from_bytes(data)
    except ValueError:
        return True
    return False


_CASES = {}


def case(log_n, k, n_pi=2, seed=3200):
    key = (log_n, k, n_pi, seed)
    if key not in _CASES:
        _CASES[key] = Case(log_n, k, n_pi, seed + 11 * k + log_n + 101 * n_pi)
    return _CASES[key]
