#!/usr/bin/env python3
"""Poseidon over BN254's scalar field (PoseidonBN128: the hash of plonky2x's wrapper config) - constants, reference model, tables.

One file holds the whole spec, each choice with where it comes from ("pinned": reproduced from published known answers by
tests/test_poseidon_bn128_cpu.py; "recalled": written from memory of plonky2x / gnark-plonky2-verifier, no source to check it
against - see DESIGN.md §16):

  * the permutation (pinned): circomlib's parameters, constants regenerated from the Grain LFSR recipe of the Poseidon
    reference implementation; two circomlib known answers (t = 3 and t = 4) pin recipe and round structure together;
  * the hash family over Goldilocks inputs (recalled): hash_no_pad, hash_or_noop, two_to_one;
  * the Merkle tree (plonky2's MerkleTree::new, unchanged but for the hasher).

The device permutation (csrc/poseidon_bn128.hpp) runs the PLAIN form (every round: t constants, S-box, full MDS product, the
MDS row as one 4-term dot product with a single Montgomery reduction) on the 29-bit-limb Montgomery arithmetic of
csrc/bn254_f29.hpp, so the tables are the plain constants in that form: nothing is derived that would need a check of its own.

Usage: python tools/gen_poseidon_bn128.py   (rewrites near-light-client_amd/csrc/poseidon_bn128_constants.inc)
"""
import os

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # BN254 scalar field (pinned: EIP-197)
T, RF, RP = 4, 8, 56          # circomlib poseidon([a, b, c]): width 4, 8 full rounds, 56 partial rounds (pinned by the t = 4 KAT)
ALPHA = 5                     # S-box x^5: gcd(5, r - 1) = 1 (pinned by both KATs)
N_BITS = 254                  # bit length of r: the Grain recipe's n
GL_P = 0xFFFFFFFF00000001     # Goldilocks: the hash family's inputs
RATE = 3                      # state[1..3] take input, state[0] is the capacity/output slot (recalled)
GL_PER_FR = 3                 # Goldilocks elements packed into one Fr slot: 3 * 64 = 192 bits < 254 (recalled)
SPONGE_CHUNK = RATE * GL_PER_FR   # 9 Goldilocks elements per permutation (recalled)

# ---- nine 29-bit limbs, Montgomery form with R' = 2^261 (csrc/bn254_f29.hpp) ----
NL, LB = 9, 29
RP_MONT = 1 << 261


def grain_bits(t, rf, rp, field=1, sbox=0, n=N_BITS):
    """the Grain LFSR output stream of the Poseidon reference implementation (generate_parameters_grain.sage)"""
    init = []
    for v, w in ((field, 2), (sbox, 4), (n, 12), (t, 12), (rf, 10), (rp, 10)):   # 80-bit state, every field MSB-first
        init += [(v >> (w - 1 - i)) & 1 for i in range(w)]
    init += [1] * 30
    b = init

    def clock():
        nb = b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13] ^ b[0]   # feedback taps; the new bit is shifted in at the end
        b.pop(0)
        b.append(nb)
        return nb

    for _ in range(160):   # warm-up, output discarded
        clock()
    while True:            # self-shrinking: a pair (1, x) outputs x, a pair (0, x) outputs nothing
        first, second = clock(), clock()
        if first:
            yield second


def _read(bits, n):
    v = 0
    for _ in range(n):   # MSB-first
        v = (v << 1) | next(bits)
    return v


def constants(t=T, rf=RF, rp=RP, p=R, n=N_BITS):
    """(round constants [(rf + rp) t], MDS [t][t]) exactly as the reference recipe draws them"""
    bits = grain_bits(t, rf, rp, n=n)
    rc = []
    while len(rc) < (rf + rp) * t:
        v = _read(bits, n)
        if v < p:          # a draw >= p is rejected and redrawn
            rc.append(v)
    while True:            # Cauchy matrix: 2t draws reduced mod p, all of them redrawn if any two coincide
        xy = [_read(bits, n) % p for _ in range(2 * t)]
        if len(set(xy)) == 2 * t:
            break
    x, y = xy[:t], xy[t:]
    mds = [[pow(x[i] + y[j], p - 2, p) for j in range(t)] for i in range(t)]
    return rc, mds


_CACHE = {}


def _params(t, rp):
    key = (t, rp)
    if key not in _CACHE:
        _CACHE[key] = constants(t, RF, rp)
    return _CACHE[key]


def permute(state, t=T, rp=RP):
    """the plain-form permutation: RF/2 full rounds, rp partial rounds, RF/2 full rounds; each round adds t constants, applies
    the S-box (every element in a full round, element 0 in a partial one) and multiplies by the MDS matrix s'_i = sum_j M[i][j] s_j"""
    rc, mds = _params(t, rp)
    s = [int(v) % R for v in state]
    assert len(s) == t
    for rnd in range(RF + rp):
        s = [(s[i] + rc[rnd * t + i]) % R for i in range(t)]
        full = rnd < RF // 2 or rnd >= RF // 2 + rp
        s = [pow(v, ALPHA, R) for v in s] if full else [pow(s[0], ALPHA, R)] + s[1:]
        s = [sum(mds[i][j] * s[j] for j in range(t)) % R for i in range(t)]
    return s


# ---- the hash family over Goldilocks inputs (recalled: plonky2x backend/wrapper/plonky2_config.rs, gnark-plonky2-verifier) ----
def pack3(elems):
    """up to three Goldilocks elements as one Fr: sum canon(e_k) 2^(64 k) (< 2^192 < r)"""
    return sum((int(e) % GL_P) << (64 * k) for k, e in enumerate(elems))


def hash_no_pad(x):
    """state [0; 4]; per chunk of 9 elements, its j-th group of <= 3 OVERWRITES state[j + 1] (slots a short last chunk does not
    reach keep their value), then one permutation; the digest is state[0]"""
    s = [0] * T
    for c in range(0, len(x), SPONGE_CHUNK):
        chunk = x[c:c + SPONGE_CHUNK]
        for j in range(0, len(chunk), GL_PER_FR):
            s[j // GL_PER_FR + 1] = pack3(chunk[j:j + GL_PER_FR])
        s = permute(s)
    return s[0]


class RangeError(ValueError):
    """a <= 4-element input whose packed value is not below r (plonky2x's from_bytes fails there too: recalled)"""


def hash_or_noop(x):
    """plonky2's default with HASH_SIZE = 32: inputs of <= 4 elements ARE the digest (sum canon(x_i) 2^(64 i)), must be < r"""
    if len(x) <= 4:
        v = sum((int(e) % GL_P) << (64 * i) for i, e in enumerate(x))
        if v >= R:
            raise RangeError("packed value >= r")
        return v
    return hash_no_pad(x)


def two_to_one(a, b):
    """compress: permute [0, 0, a, b], digest state[0]"""
    return permute([0, 0, a, b])[0]


def to_words(v):
    """a digest at the ABI: four little-endian u64 words, canonical (not Montgomery)"""
    return [(v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]


def from_words(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


def merkle_digests(leaves, cap_height):
    """MerkleTree::new: leaf digests hash_or_noop(row), nodes two_to_one; level-major list of levels down to and including the cap"""
    lvl = [hash_or_noop(list(row)) for row in leaves]
    levels = [lvl]
    while len(lvl) > (1 << cap_height):
        lvl = [two_to_one(lvl[2 * i], lvl[2 * i + 1]) for i in range(len(lvl) // 2)]
        levels.append(lvl)
    return levels


def merkle_root_from_path(leaf_digest, index, path):
    """walks a MerkleTree::prove path (siblings bottom-up) from a leaf digest: returns (cap index, the digest reached)"""
    h = leaf_digest
    for sib in path:
        h = two_to_one(sib, h) if index & 1 else two_to_one(h, sib)
        index >>= 1
    return index, h


# ---- the tables of csrc/poseidon_bn128.hpp ----
def limbs(v):
    return [(v >> (LB * i)) & ((1 << LB) - 1) if i < NL - 1 else v >> (LB * (NL - 1)) for i in range(NL)]


def mont(v):
    return v * RP_MONT % R


def render():
    rc, mds = constants()
    out = ["// GENERATED by tools/gen_poseidon_bn128.py - do not edit.  PoseidonBN128 (circomlib t = 4, R_F = 8, R_P = 56) in the",
           "// plain form, every constant in the Montgomery form of csrc/bn254_f29.hpp (x 2^261 mod r, nine 29-bit limbs).",
           "#define NLX_PBN_T %d" % T, "#define NLX_PBN_RF %d" % RF, "#define NLX_PBN_RP %d" % RP,
           "// round constants: [round][element][limb]",
           "#define NLX_PBN_RC_INIT { \\"]
    for rnd in range(RF + RP):
        row = []
        for i in range(T):
            row += ["0x%08xu" % x for x in limbs(mont(rc[rnd * T + i]))]
        out.append("    " + ", ".join(row) + ", \\")
    out.append("}")
    out.append("// MDS matrix M[i][j]: [i][j][limb] (canonical Montgomery values < r: limb 8 < 2^22)")
    out.append("#define NLX_PBN_MDS_INIT { \\")
    for i in range(T):
        row = []
        for j in range(T):
            row += ["0x%08xu" % x for x in limbs(mont(mds[i][j]))]
        out.append("    " + ", ".join(row) + ", \\")
    out.append("}")
    out.append("// 2^522 mod r: mul(x, R2) takes a value into the Montgomery form")
    out.append("#define NLX_PBN_R2_INIT { %s }" % ", ".join("0x%08xu" % x for x in limbs(pow(2, 522, R))))
    return "\n".join(out) + "\n"


INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "near-light-client_amd", "csrc",
                   "poseidon_bn128_constants.inc")

# circomlib known answers (pinned): poseidon([1, 2]) = perm([0, 1, 2])[0] at t = 3, poseidon([1, 2, 3]) at t = 4
KAT_T3 = 7853200120776062878684798364095072458815029376092732009249414926327459813530
KAT_T4 = 6542985608222806190361240322586112750744169038454362455181422643027100751666


def self_check():
    assert permute([0, 1, 2], t=3, rp=57)[0] == KAT_T3, "t = 3 known answer"
    assert permute([0, 1, 2, 3])[0] == KAT_T4, "t = 4 known answer"
    rc3, mds3 = constants(3, RF, 57)
    assert rc3[0] >> 224 == 0x0ee9a592 and rc3[0] & 0xFFFFFFFF == 0x04cd8e6e
    assert mds3[0][0] >> 224 == 0x109b7f41 and mds3[0][0] & 0xFFFFFFFF == 0x2ba8118b


if __name__ == "__main__":
    self_check()
    text = render()
    with open(INC, "w") as f:
        f.write(text)
    print("wrote %s" % INC)
