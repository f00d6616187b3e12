#!/usr/bin/env python3
"""plonky2x's PoseidonBN128GoldilocksConfig in pure Python: how BN128 digests meet the Goldilocks transcript, and a proof replay
verifier for proofs made under it (nlx_circuit_build_hasher with NLX_HASHER_POSEIDON_BN128).

Status of every rule: RECALLED from plonky2 / plonky2x (backend/wrapper/plonky2_config.rs), UNPINNED - there is no Rust-produced
proof to compare with.  Each rule is written once, here:

  rule 1  Hasher = PoseidonBN128Hash, InnerHasher = PoseidonHash (Goldilocks), Hasher::Permutation = PoseidonPermutation<Goldilocks>:
          the challenger's sponge and the proof of work stay the Goldilocks permutation              (replay: oracle_py.Challenger)
  rule 2  GenericHashOut::to_vec of a BN128 digest: its 32 little-endian bytes in chunks of 7, 7, 7, 7, 4 bytes, each one
          Goldilocks element; observe_hash, observe_cap and MerkleCap::flatten go through it         (digest_limbs)
  rule 3  public_inputs_hash = InnerHasher::hash_no_pad: Goldilocks, four elements                  (replay)
  rule 4  circuit_digest = Hasher::hash_no_pad(cap.flatten() || to_vec(Hasher::hash_no_pad(P)) || degree_bits), P the padded
          empty domain separator [1, 0 x 10, 1]                                                     (circuit_digest)
  rule 5  transcript order as under the Goldilocks config                                           (replay)
  rule 6  every Merkle tree: BN128 hash_or_noop leaves, two_to_one nodes (tools/gen_poseidon_bn128.py); a commit-phase leaf is
          the 2 arity words of one coset                                                            (verify)
  rule 7  proof bytes as under the Goldilocks config, a digest = four little-endian u64 words       (parse_proof)

The replay verifier is test infrastructure: it re-derives every challenge from the proof bytes and checks the FRI part the way
plonky2's verify_fri_proof does (proof of work, initial Merkle paths, the reduced opening at the query point, every commit-phase
coset's path and its interpolation at beta, the final polynomial).  It does NOT check the PLONK identities at zeta: the tests pin
the committed polynomials to the frozen oracle's instead.
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "oracle"))
import gen_poseidon_bn128 as m  # noqa: E402

R = m.R
P = m.GL_P
W = 7                      # the quadratic extension F_p[X] / (X^2 - 7)
DIGEST_LIMBS = 5
LIMB_BYTES = (7, 7, 7, 7, 4)
DOMAIN_SEPARATOR_PADDED = [1] + [0] * 10 + [1]   # hash_pad of the empty domain separator, as the Goldilocks path hashes it


class Reject(Exception):
    """the replay verifier's "no", with the first failed check"""


# ---- rule 2 ----
def digest_limbs(v):
    """a digest (int < r) -> its five Goldilocks elements"""
    if not 0 <= v < R:
        raise ValueError("digest is not below r")
    b = int(v).to_bytes(32, "little")
    out, off = [], 0
    for k in LIMB_BYTES:
        out.append(int.from_bytes(b[off:off + k], "little"))
        off += k
    return out


def digest_from_limbs(limbs):
    b = b"".join(int(x).to_bytes(k, "little") for x, k in zip(limbs, LIMB_BYTES))
    return int.from_bytes(b, "little")


def flatten(digests):
    """MerkleCap::flatten"""
    return [x for d in digests for x in digest_limbs(d)]


# ---- rule 4 ----
def circuit_digest(cap, degree_bits):
    inner = m.hash_no_pad(DOMAIN_SEPARATOR_PADDED)
    return m.hash_no_pad(flatten(cap) + digest_limbs(inner) + [degree_bits])


# ---- Goldilocks and its quadratic extension (python ints) ----
def root_of_unity(bits):
    _, _, pow2_gen = _field()
    return pow(pow2_gen, 1 << (32 - bits), P)


_FIELD = None


def _field():
    """(set, MULTIPLICATIVE_GROUP_GENERATOR, POWER_OF_TWO_GENERATOR) of include/nlx_field.h"""
    global _FIELD
    if _FIELD is None:
        import re
        gen_set = os.environ.get("NLX_GL_GENERATOR_SET", "7")
        text = open(os.path.join(os.path.dirname(_HERE), "include", "nlx_field.h")).read()
        mt = re.search(r"NLX_GL_GENERATOR_SET == %s\s*\n#define NLX_GL_MULTIPLICATIVE_GROUP_GENERATOR (\d+)ULL\s*\n"
                       r"#define NLX_GL_POWER_OF_TWO_GENERATOR (\d+)ULL" % gen_set, text)
        _FIELD = (gen_set, int(mt.group(1)), int(mt.group(2)))
    return _FIELD


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_inv(a):
    n = pow((a[0] * a[0] - W * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, (-a[1]) * n % P)


def reduce_with_powers(vals, alpha):
    """ReducingFactor::reduce: sum alpha^i v_i"""
    acc = (0, 0)
    for v in reversed(vals):
        acc = e_add(e_mul(acc, alpha), v)
    return acc


def e_pow(a, n):
    r = (1, 0)
    while n:
        if n & 1:
            r = e_mul(r, a)
        a = e_mul(a, a)
        n >>= 1
    return r


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def fri_num_rounds(degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits):
    """FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits)"""
    r = 0
    while degree_bits > final_poly_bits and degree_bits + rate_bits >= cap_height + arity_bits and degree_bits >= arity_bits:
        degree_bits -= arity_bits
        r += 1
    return r


# ---- rule 7: the proof bytes ----
class Shape:
    """what the verifier knows of the circuit: column counts and the FRI configuration"""

    def __init__(self, degree_bits, n_constants_sigmas, num_wires, num_challenges, num_partial_products, quotient_degree_factor,
                 rate_bits, cap_height, fri_arity_bits, fri_final_poly_bits, fri_pow_bits, fri_num_queries):
        self.degree_bits, self.n_cs, self.num_wires, self.nc, self.npp = degree_bits, n_constants_sigmas, num_wires, num_challenges, num_partial_products
        self.qdf, self.rate_bits, self.cap_height = quotient_degree_factor, rate_bits, cap_height
        self.arity_bits, self.final_poly_bits, self.pow_bits, self.num_queries = fri_arity_bits, fri_final_poly_bits, fri_pow_bits, fri_num_queries
        self.n_zs = num_challenges * (1 + num_partial_products)
        self.n_q = num_challenges * quotient_degree_factor
        self.log_L = degree_bits + rate_bits
        self.n_rounds = fri_num_rounds(degree_bits, rate_bits, cap_height, fri_arity_bits, fri_final_poly_bits)
        self.oracle_cols = (self.n_cs, self.num_wires, self.n_zs, self.n_q)

    @classmethod
    def from_synthetic(cls, syn):
        c = syn.config
        return cls(syn.log_n, syn.num_selectors + c.num_constants + c.num_routed_wires, c.num_wires, c.num_challenges,
                   c.num_partial_products, c.quotient_degree_factor, c.rate_bits, c.cap_height, c.fri_arity_bits,
                   c.fri_final_poly_bits, c.fri_pow_bits, c.fri_num_queries)


class _Reader:
    def __init__(self, b):
        self.b, self.off = bytes(b), 0

    def u64s(self, n):
        if self.off + 8 * n > len(self.b):
            raise Reject("proof is truncated")
        out = [int.from_bytes(self.b[self.off + 8 * i:self.off + 8 * i + 8], "little") for i in range(n)]
        self.off += 8 * n
        return out

    def u8(self):
        if self.off + 1 > len(self.b):
            raise Reject("proof is truncated")
        self.off += 1
        return self.b[self.off - 1]

    def digests(self, n):
        w = self.u64s(4 * n)
        return [m.from_words(w[4 * i:4 * i + 4]) for i in range(n)]

    def exts(self, n):
        w = self.u64s(2 * n)
        return [(w[2 * i], w[2 * i + 1]) for i in range(n)]


def parse_proof(proof, sh):
    """-> dict; `offsets` names the byte ranges (for tests that flip bytes)"""
    rd = _Reader(proof)
    ncap = 1 << sh.cap_height
    p, off = {}, {}

    def mark(name, start):
        off[name] = (start, rd.off)

    s = rd.off
    p["wires_cap"], p["zs_cap"], p["quotient_cap"] = rd.digests(ncap), rd.digests(ncap), rd.digests(ncap)
    mark("caps", s)
    s = rd.off
    op = {}
    op["constants_sigmas"] = rd.exts(sh.n_cs)
    op["wires"] = rd.exts(sh.num_wires)
    op["zs"] = rd.exts(sh.nc)
    op["zs_next"] = rd.exts(sh.nc)
    op["partial_products"] = rd.exts(sh.nc * sh.npp)
    op["quotient"] = rd.exts(sh.n_q)
    p["openings"] = op
    mark("openings", s)
    s = rd.off
    p["commit_caps"] = [rd.digests(ncap) for _ in range(sh.n_rounds)]
    mark("commit_caps", s)
    arity = 1 << sh.arity_bits
    queries = []
    s = rd.off
    first_sibling = None
    for _ in range(sh.num_queries):
        q = {"rows": [], "paths": [], "steps": []}
        for cols in sh.oracle_cols:
            q["rows"].append(rd.u64s(cols))
            plen = rd.u8()
            if first_sibling is None and plen:
                first_sibling = (rd.off, rd.off + 32)
            q["paths"].append(rd.digests(plen))
        for _r in range(sh.n_rounds):
            evals = rd.exts(arity)
            plen = rd.u8()
            q["steps"].append((evals, rd.digests(plen)))
        queries.append(q)
    p["queries"] = queries
    mark("queries", s)
    off["first_sibling"] = first_sibling
    s = rd.off
    p["final_poly"] = rd.exts(1 << (sh.degree_bits - sh.n_rounds * sh.arity_bits))
    mark("final_poly", s)
    s = rd.off
    p["pow_witness"] = rd.u64s(1)[0]
    mark("pow_witness", s)
    n_pi = rd.u64s(1)[0]
    if n_pi > (len(rd.b) - rd.off) // 8:
        raise Reject("public input count")
    p["public_inputs"] = rd.u64s(n_pi)
    if rd.off != len(rd.b):
        raise Reject("trailing bytes")
    p["offsets"] = off
    return p


# ---- rules 1, 3, 5: the transcript ----
def _canonical(vals, what):
    for v in vals:
        if v >= P:
            raise Reject("%s: a field element is not canonical" % what)


def replay(proof, sh, circuit_digest_value, parsed=None):
    """re-derives every challenge from the proof bytes -> dict (the parsed proof under "proof")"""
    import oracle_py
    p = parsed or parse_proof(proof, sh)
    ch = oracle_py.Challenger()

    def observe(xs):
        for x in xs:
            ch.observe(x)

    def observe_hashes(ds, what):
        for d in ds:
            if d >= R:
                raise Reject("%s: a digest is not below r" % what)
        observe(flatten(ds))

    def ext():
        a = ch.challenge()
        return (a, ch.challenge())

    out = {"proof": p}
    pis = p["public_inputs"]
    _canonical(pis, "public inputs")
    pih = [int(x) for x in oracle_py.hash_no_pad(pis)] if pis else [int(x) for x in oracle_py.hash_no_pad([])]
    out["public_inputs_hash"] = pih
    observe_hashes([circuit_digest_value], "circuit digest")
    observe(pih)
    observe_hashes(p["wires_cap"], "wires cap")
    out["betas"] = [ch.challenge() for _ in range(sh.nc)]
    out["gammas"] = [ch.challenge() for _ in range(sh.nc)]
    observe_hashes(p["zs_cap"], "Zs cap")
    out["alphas"] = [ch.challenge() for _ in range(sh.nc)]
    observe_hashes(p["quotient_cap"], "quotient cap")
    out["zeta"] = ext()
    op = p["openings"]
    # the zeta batch in FRI order (constants_sigmas, wires, Zs ++ partial products, quotient), then the g zeta batch
    batch0 = op["constants_sigmas"] + op["wires"] + op["zs"] + op["partial_products"] + op["quotient"]
    batch1 = op["zs_next"]
    for e in batch0 + batch1:
        _canonical(e, "openings")
        observe(e)
    out["batch0"], out["batch1"] = batch0, batch1
    out["fri_alpha"] = ext()
    betas = []
    for cap in p["commit_caps"]:
        observe_hashes(cap, "commit-phase cap")
        betas.append(ext())
    out["fri_betas"] = betas
    for e in p["final_poly"]:
        _canonical(e, "final polynomial")
        observe(e)
    if p["pow_witness"] >= P:
        raise Reject("proof-of-work witness is not canonical")
    ch.observe(p["pow_witness"])
    out["pow_response"] = ch.challenge()
    out["query_indices"] = [ch.challenge() % (1 << sh.log_L) for _ in range(sh.num_queries)]
    return out


# ---- rule 6 and verify_fri_proof ----
def _check_path(leaf_words, index, path, cap, what):
    ci, h = m.merkle_root_from_path(m.hash_or_noop(leaf_words), index, path)
    if ci >= len(cap) or h != cap[ci]:
        raise Reject("%s: Merkle path does not reach the cap" % what)


def _interpolate(points, values, x):
    """Lagrange interpolation through (points[i] in F_p, values[i] in the extension), evaluated at x"""
    acc = (0, 0)
    for i, (xi, yi) in enumerate(zip(points, values)):
        num, den = (1, 0), 1
        for j, xj in enumerate(points):
            if j != i:
                num = e_mul(num, e_sub(x, (xj, 0)))
                den = den * (xi - xj) % P
        acc = e_add(acc, e_mul(e_mul(num, (pow(den, P - 2, P), 0)), yi))
    return acc


def verify(proof, sh, circuit_digest_value, constants_sigmas_cap):
    """the replay verifier: returns replay()'s dict or raises Reject at the first failed check"""
    t = replay(proof, sh, circuit_digest_value)
    p = t["proof"]
    _, gen, _ = _field()
    if sh.pow_bits and t["pow_response"] >> (64 - sh.pow_bits):
        raise Reject("proof of work")
    if len(p["final_poly"]) != 1 << (sh.degree_bits - sh.n_rounds * sh.arity_bits):
        raise Reject("final polynomial length")
    alpha, zeta = t["fri_alpha"], t["zeta"]
    g_zeta = e_mul(zeta, (root_of_unity(sh.degree_bits), 0))
    red0, red1 = reduce_with_powers(t["batch0"], alpha), reduce_with_powers(t["batch1"], alpha)
    alpha_n1 = e_pow(alpha, len(t["batch1"]))
    caps = (constants_sigmas_cap, p["wires_cap"], p["zs_cap"], p["quotient_cap"])
    arity = 1 << sh.arity_bits
    w_L, w_A = root_of_unity(sh.log_L), root_of_unity(sh.arity_bits)
    for qi, (x_index, q) in enumerate(zip(t["query_indices"], p["queries"])):
        for o in range(4):
            _canonical(q["rows"][o], "query %d oracle %d row" % (qi, o))
            if len(q["paths"][o]) != sh.log_L - sh.cap_height:
                raise Reject("query %d oracle %d: path length" % (qi, o))
            _check_path(q["rows"][o], x_index, q["paths"][o], caps[o], "query %d oracle %d" % (qi, o))
        subgroup_x = gen * pow(w_L, bitrev(x_index, sh.log_L), P) % P
        sx = (subgroup_x, 0)
        evals0 = [(v, 0) for row in q["rows"] for v in row]
        evals1 = [(v, 0) for v in q["rows"][2][:sh.nc]]
        s0, s1 = reduce_with_powers(evals0, alpha), reduce_with_powers(evals1, alpha)
        old = e_mul(e_sub(s0, red0), e_inv(e_sub(sx, zeta)))
        old = e_add(e_mul(old, alpha_n1), e_mul(e_sub(s1, red1), e_inv(e_sub(sx, g_zeta))))
        for r, (evals, path) in enumerate(q["steps"]):
            for e in evals:
                _canonical(e, "query %d round %d" % (qi, r))
            coset_index, within = x_index >> sh.arity_bits, x_index & (arity - 1)
            if evals[within] != old:
                raise Reject("query %d round %d: the coset does not hold the folded value" % (qi, r))
            # compute_evaluation: the coset in natural order starts at x * w_A^(arity - rev(within))
            evals_nat = [evals[bitrev(i, sh.arity_bits)] for i in range(arity)]
            start = subgroup_x * pow(w_A, arity - bitrev(within, sh.arity_bits), P) % P
            points = [start * pow(w_A, i, P) % P for i in range(arity)]
            old = _interpolate(points, evals_nat, t["fri_betas"][r])
            _check_path([v for e in evals for v in e], coset_index, path, p["commit_caps"][r], "query %d round %d" % (qi, r))
            subgroup_x = pow(subgroup_x, arity, P)
            x_index = coset_index
        fe = (0, 0)
        for c in reversed(p["final_poly"]):
            fe = e_add(e_mul(fe, (subgroup_x, 0)), c)
        if fe != old:
            raise Reject("query %d: final polynomial" % qi)
    return t
