"""Row f.4, the Groth16 half: whole proofs over BN254 from a proving key resident in HBM - the host-side mirror of gnark's
backend/groth16/bn254 `ProvingKey` and `Prove` (Go, not in the reference; layout and rules recalled from gnark v0.9, parity with
gnark-produced bytes unpinned: DESIGN.md section 19).

  ProvingKey(ctx, ...)   nlx_bn254_groth16_key_create: gnark's key as it lies in memory, uploaded and converted once
  r1cs_eval(pk, w)       nlx_bn254_r1cs_eval: A w, B w, C w
  prove(pk, w, r, s)     nlx_bn254_groth16_prove: the proof's three points (G1Affine / G2Affine / G1Affine words)
  proof_bytes(...)       gnark's Proof.WriteTo, 164 + 32 k bytes; g1_compress / g2_compress: gnark-crypto's Bytes()
  VerifyingKey(ctx, ...) nlx_bn254_groth16_vk_create: gnark's VerifyingKey resident, e(alpha, beta) precomputed on the device;
                         .verify(proof_bytes, public) / .verify_many(proofs, publics) -> Verdict
  setup(ctx, ..., r1cs)  nlx_bn254_groth16_setup: gnark's groth16.Setup from a trapdoor on the device -> (ProvingKey,
                         VerifyingKey, SetupArrays); Setup is the resident result itself
  Setup.proving_key_bytes(raw) / ProvingKey.from_bytes(ctx, data, r1cs=, commitments=)
                         gnark's ProvingKey.WriteTo / WriteRawTo and ReadFrom, the points through the device codec
                         (bn254_codec.py; layout: tools/gnark_bytes_model.py)
Keys with k Bsb22 / Pedersen commitments (rules: tools/groth16_commit_model.py):
  ProvingKey(ctx, ..., commitments=[...])   nlx_bn254_groth16_key_create_committed: the Pedersen bases resident next to the key
  commit(pk, j, w)                          nlx_bn254_groth16_commit: C_j, the call a solver's hint makes
  commitment_challenge(pk, j, point, w)     the value of commitment j's wire: fr.Hash(C_j.Marshal() || hashed values)
  prove_committed(pk, w, r, s)              nlx_bn254_groth16_prove_committed: (ar, bs, krs, [C_j], pok)

Every element is an fr.Element / fp.Element as it lies in memory (four little-endian words, Montgomery); arrays are numpy uint64
or device tensors.  Parity: device bytes equal the big-integer model's (tools/groth16_model.py) and its trapdoor verifier accepts
them (tests/test_gpu_bn254_groth16.py)."""
import ctypes
import secrets

import numpy as np

from . import batch as B
from ._lib import NlxError, dll, ptr
from .bn254_plonk import fr_bytes, g1_marshal, hash_to_field, root_of_unity

R, Q = B.BN254_R, B.BN254_Q
_MONT = (1 << 256) % R
NLX_BN254_MONTGOMERY = 1
KEY_INFO_WORDS = 8
MAX_COMMITMENTS = 8
COMMITMENT_DST = b"bsb22-commitment"     # the hint's hash (gnark constraint/commitment.go)
FOLD_DST = b"G16-BSB22"                  # pedersen.BatchProve's folding challenge (gnark backend/groth16/bn254/prove.go)
NLX_E_INVAL, NLX_E_RANGE = -1, -4


class _KeyDesc(ctypes.Structure):
    """nlx_bn254_groth16_key_desc (include/nlx.h)"""
    _fields_ = ([("log_n", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_wires", ctypes.c_uint64), ("n_public", ctypes.c_uint64),
                 ("n_constraints", ctypes.c_uint64)]
                + [f for k in ("g1_a", "g1_b", "g2_b", "g1_k", "g1_z") for f in ((k, ctypes.c_void_p), ("n_" + k, ctypes.c_uint64))]
                + [(k, ctypes.c_void_p) for k in ("infinity_a", "infinity_b", "g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta",
                                                  "a_row_ptr", "b_row_ptr", "c_row_ptr", "a_wire", "b_wire", "c_wire",
                                                  "a_coeff_id", "b_coeff_id", "c_coeff_id", "coeffs")]
                + [("n_coeffs", ctypes.c_uint64), ("n_commitments", ctypes.c_uint32)])


class _CommitDesc(ctypes.Structure):
    """nlx_bn254_groth16_commit_desc (include/nlx.h)"""
    _fields_ = [("n_commitments", ctypes.c_uint32), ("n_private", ctypes.c_void_p), ("private_wires", ctypes.c_void_p),
                ("basis", ctypes.c_void_p), ("basis_exp_sigma", ctypes.c_void_p), ("commitment_wires", ctypes.c_void_p)]


def fr_words(x):
    """an integer below r -> its fr.Element words (Montgomery)"""
    m = int(x) % R * _MONT % R
    return np.array([(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)], dtype=np.uint64)


def fr_pack(values):
    """integers below r -> (n, 4) uint64 fr.Element words (Montgomery)"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, x in enumerate(values):
        m = int(x) % R * _MONT % R
        for w in range(4):
            out[i, w] = (m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def fr_unpack(words):
    """(n, 4) fr.Element words -> integers"""
    minv = pow(_MONT, R - 2, R)
    a = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(a[i, w]) << (64 * w) for w in range(4)) * minv % R for i in range(a.shape[0])]


DOMAIN_BYTES = 8 + 5 * 32


def domain_bytes(log_n):
    """fft.Domain.WriteTo as a ProvingKey carries it: the cardinality (uint64), then CardinalityInv, Generator, GeneratorInv,
    FrMultiplicativeGen (5) and FrMultiplicativeGenInv as 32-byte big-endian canonical integers"""
    n, w = 1 << log_n, root_of_unity(log_n)
    return n.to_bytes(8, "big") + b"".join(v.to_bytes(32, "big") for v in (pow(n, R - 2, R), w, pow(w, R - 2, R), 5, pow(5, R - 2, R)))


def _buf(a, dtype, width=None, size=None):
    """(object kept alive, address, rows) of a numpy array or a contiguous device tensor.  width: the array is (rows, width);
    width 0: one-dimensional; size: its total number of elements.  A wrong shape raises here: the library reads what the
    descriptor's counts say and cannot see where the caller's buffer ends."""
    if a is None:
        return None, None, 0
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise TypeError("expected a contiguous tensor")
        if a.element_size() != np.dtype(dtype).itemsize or a.is_floating_point():
            raise TypeError("expected %d-byte integer elements" % np.dtype(dtype).itemsize)
        shape, count = tuple(a.shape), a.numel()
    else:
        a = np.ascontiguousarray(a, dtype=dtype)
        shape, count = a.shape, a.size
    if width == 0 and len(shape) != 1:
        raise ValueError("expected a one-dimensional array, got shape %r" % (shape,))
    if width and (len(shape) != 2 or shape[1] != width):
        raise ValueError("expected shape (n, %d), got %r" % (width, shape))
    if size is not None and count != size:
        raise ValueError("expected %d elements, got %d" % (size, count))
    return a, (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data), (shape[0] if shape else 0)


class ProvingKey:
    """nlx_bn254_groth16_key: gnark's groth16.ProvingKey resident on the device (owns the handle; close() or the context's
    close() releases it).

    g1_a, g1_b, g1_k, g1_z: (count, 8) G1Affine words; g2_b: (count, 16) G2Affine words - the queries filtered of their points at
    infinity, as gnark keeps them; infinity_a, infinity_b: one byte (or bool) per wire, non-zero = filtered out; g1_alpha,
    g1_beta, g1_delta (8 words), g2_beta, g2_delta (16 words).  r1cs (optional): {"A": (row_ptr, wire, coeff_id), "B": ...,
    "C": ..., "coeffs": (n_coeffs, 4) fr.Element words} with row_ptr uint64, wire and coeff_id uint32.  Arrays are numpy or device
    tensors.  commitments (optional): gnark's Bsb22 / Pedersen commitments, one dict each - "private": PrivateCommitted (wire
    ids, ascending), "public": PublicAndCommitmentCommitted (wire ids; kept on the host, for the hash), "wire": CommitmentIndex,
    "basis" / "basis_exp_sigma": the Pedersen key's points, (len(private), 8) words, numpy - and g1_k then holds the private wires
    that are neither committed nor a commitment's.  n_commitments without `commitments`: anything but 0 raises (the bases have
    nowhere to go)."""

    def __init__(self, ctx, log_n, n_wires, n_public, n_constraints, g1_a, g1_b, g2_b, g1_k, g1_z, infinity_a, infinity_b,
                 g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta, r1cs=None, n_commitments=None, flags=NLX_BN254_MONTGOMERY,
                 commitments=None):
        self.ctx, self.handle = ctx, None
        self.commitments = [] if commitments is None else [
            {"private": [int(i) for i in c["private"]], "public": [int(i) for i in c["public"]], "wire": int(c["wire"])} for c in commitments]
        if n_commitments is None:
            n_commitments = len(self.commitments)
        self.log_n, self.n_wires, self.n_public, self.n_constraints = int(log_n), int(n_wires), int(n_public), int(n_constraints)
        d = _KeyDesc()
        d.log_n, d.flags, d.n_wires, d.n_public, d.n_constraints = self.log_n, int(flags), self.n_wires, self.n_public, self.n_constraints
        d.n_commitments = int(n_commitments)
        keep = []
        for name, arr, width in (("g1_a", g1_a, 8), ("g1_b", g1_b, 8), ("g2_b", g2_b, 16), ("g1_k", g1_k, 8), ("g1_z", g1_z, 8)):
            k, p, rows = _buf(arr, np.uint64, width)
            keep.append(k)
            setattr(d, name, p)
            setattr(d, "n_" + name, rows)
        for name, arr in (("infinity_a", infinity_a), ("infinity_b", infinity_b)):
            k, p, _ = _buf(arr, np.uint8, 0, size=self.n_wires)
            keep.append(k)
            setattr(d, name, p)
        for name, arr, count in (("g1_alpha", g1_alpha, 8), ("g1_beta", g1_beta, 8), ("g1_delta", g1_delta, 8), ("g2_beta", g2_beta, 16),
                                 ("g2_delta", g2_delta, 16)):
            k, p, _ = _buf(arr, np.uint64, size=count)
            keep.append(k)
            setattr(d, name, p)
        if r1cs is not None:
            for m in "ABC":
                rows = {}
                for field, arr, dt in zip(("row_ptr", "wire", "coeff_id"), r1cs[m], (np.uint64, np.uint32, np.uint32)):
                    k, p, rows[field] = _buf(arr, dt, 0)
                    keep.append(k)
                    setattr(d, "%s_%s" % (m.lower(), field), p)
                # the library finds the number of terms in row_ptr's last entry, which it validates against nothing but itself
                if rows["row_ptr"] != self.n_constraints + 1 or rows["wire"] != rows["coeff_id"]:
                    raise ValueError("matrix %s: row_ptr holds n_constraints + 1 offsets, wire and coeff_id one entry per term" % m)
                last = int(r1cs[m][0][-1]) if rows["row_ptr"] else 0
                if last > rows["wire"]:
                    raise ValueError("matrix %s: row_ptr ends at %d, the matrix holds %d terms" % (m, last, rows["wire"]))
            k, p, rows = _buf(r1cs["coeffs"], np.uint64, 4)
            keep.append(k)
            d.coeffs, d.n_coeffs = p, rows
        h = ctypes.c_void_p()
        if commitments is None:
            ctx.check(dll.nlx_bn254_groth16_key_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        else:
            cd = _CommitDesc()
            cd.n_commitments = len(commitments)
            counts = np.array([len(c["private"]) for c in self.commitments], dtype=np.uint64)
            ids = np.array([i for c in self.commitments for i in c["private"]], dtype=np.uint32)
            wires = np.array([c["wire"] for c in self.commitments], dtype=np.uint32)
            bases = []
            for name in ("basis", "basis_exp_sigma"):
                parts = [np.ascontiguousarray(c[name], dtype=np.uint64).reshape(-1, 8) for c in commitments]
                if [len(p) for p in parts] != [len(c["private"]) for c in self.commitments]:
                    raise ValueError("%s holds one point per committed wire" % name)
                bases.append(np.concatenate(parts) if parts else np.zeros((0, 8), dtype=np.uint64))
            keep += [counts, ids, wires] + bases
            cd.n_private, cd.private_wires, cd.commitment_wires = counts.ctypes.data, ids.ctypes.data, wires.ctypes.data
            cd.basis, cd.basis_exp_sigma = bases[0].ctypes.data, bases[1].ctypes.data
            ctx.check(dll.nlx_bn254_groth16_key_create_committed(ctx.handle, ctypes.byref(d), ctypes.byref(cd), ctypes.byref(h)))
        self.handle = h
        self.has_r1cs = r1cs is not None
        ctx._adopt(self)

    @classmethod
    def _from_handle(cls, ctx, handle, log_n, n_wires, n_public, n_constraints, commitments=()):
        """a key the library built itself (Setup.key): the handle is adopted as it is"""
        self = cls.__new__(cls)
        self.ctx, self.handle = ctx, handle
        self.commitments = [{"private": [int(i) for i in c["private"]], "public": [int(i) for i in c["public"]], "wire": int(c["wire"])}
                            for c in commitments]
        self.log_n, self.n_wires, self.n_public, self.n_constraints = int(log_n), int(n_wires), int(n_public), int(n_constraints)
        self.has_r1cs = True
        ctx._adopt(self)
        return self

    @classmethod
    def from_bytes(cls, ctx, data, r1cs, commitments=None):
        """gnark's groth16.ProvingKey.ReadFrom, the result resident: `data` is what ProvingKey.WriteTo or WriteRawTo wrote (the
        mode is read off G1.Alpha's flag bits; layout: tools/gnark_bytes_model.py rule 10, recalled and unpinned).  The R1CS and
        the commitments' wire sets live in gnark's constraint system, not in the key, so they stay arguments: r1cs as for the
        constructor; commitments: one dict per commitment key with "private", "public", "wire" (Basis and BasisExpSigma come from
        the bytes).  n_constraints is the matrices' row count; n_public follows from the sizes: the wires that are neither in
        G1.K nor committed nor a commitment's.  Every point goes through the device codec, each slice in one call and the big
        ones without leaving the device; NlxError (NLX_E_INVAL) names the section for short or trailing data, for a count that
        disagrees with the sizes, and section and index for a bad point."""
        from . import bn254_codec as C
        rd = C.Reader(ctx, data, C.container_is_raw(data, [("domain", DOMAIN_BYTES)], "G1.Alpha"), "cuda:%d" % ctx.device)
        n = rd.u64("domain")
        if n == 0 or n & (n - 1) or n > 1 << 28:
            raise NlxError(NLX_E_INVAL, "domain: the cardinality %d is no power of two up to 2^28" % n)
        log_n = n.bit_length() - 1
        if bytes(rd.take(DOMAIN_BYTES - 8, "domain")) != domain_bytes(log_n)[8:]:
            raise NlxError(NLX_E_INVAL, "domain: not the domain of cardinality %d" % n)
        single = {k: rd.point(False, "G1." + k[3:].capitalize()) for k in ("g1_alpha", "g1_beta", "g1_delta")}
        big = {k: rd.points(False, "G1." + k[3:].upper(), device=True) for k in ("g1_a", "g1_b", "g1_z", "g1_k")}
        single["g2_beta"], single["g2_delta"] = rd.point(True, "G2.Beta"), rd.point(True, "G2.Delta")
        big["g2_b"] = rd.points(True, "G2.B", device=True)
        n_wires, nb_a, nb_b = rd.u64("nbWires"), rd.u64("NbInfinityA"), rd.u64("NbInfinityB")
        inf_a, inf_b = rd.bools("InfinityA"), rd.bools("InfinityB")
        for name, mask, nb, pts in (("A", inf_a, nb_a, big["g1_a"]), ("B", inf_b, nb_b, big["g1_b"])):
            if len(mask) != n_wires or int(mask.sum()) != nb or len(pts) != n_wires - nb:
                raise NlxError(NLX_E_INVAL, "Infinity%s: %d flags, %d set, NbInfinity%s %d, %d wires, %d points in G1.%s"
                               % (name, len(mask), int(mask.sum()), name, nb, n_wires, len(pts), name))
        if len(big["g2_b"]) != len(big["g1_b"]):
            raise NlxError(NLX_E_INVAL, "G2.B: %d points, G1.B has %d" % (len(big["g2_b"]), len(big["g1_b"])))
        if len(big["g1_z"]) != n - 1:
            raise NlxError(NLX_E_INVAL, "G1.Z: %d points, the domain wants %d" % (len(big["g1_z"]), n - 1))
        k = rd.u32("commitment keys count")
        sets = [] if commitments is None else [dict(c) for c in commitments]
        if k != len(sets):
            raise NlxError(NLX_E_INVAL, "commitment keys count: the key holds %d, %d wire sets were given" % (k, len(sets)))
        for j, c in enumerate(sets):
            c["basis"], c["basis_exp_sigma"] = rd.points(False, "commitment key %d Basis" % j), rd.points(False, "commitment key %d BasisExpSigma" % j)
            for name, pts in (("Basis", c["basis"]), ("BasisExpSigma", c["basis_exp_sigma"])):
                if len(pts) != len(c["private"]):
                    raise NlxError(NLX_E_INVAL, "commitment key %d %s: %d points, %d committed wires" % (j, name, len(pts), len(c["private"])))
        rd.end("proving key")
        n_public = n_wires - len(big["g1_k"]) - sum(len(c["private"]) for c in sets) - k
        if n_public < 1:
            raise NlxError(NLX_E_INVAL, "G1.K: %d points leave no public wire among %d" % (len(big["g1_k"]), n_wires))
        return cls(ctx, log_n, n_wires, n_public, len(r1cs["A"][0]) - 1, big["g1_a"], big["g1_b"], big["g2_b"], big["g1_k"], big["g1_z"], inf_a, inf_b,
                   single["g1_alpha"], single["g1_beta"], single["g1_delta"], single["g2_beta"], single["g2_delta"], r1cs=r1cs,
                   commitments=sets if commitments is not None else None)

    def info(self):
        """what the key reports: resident bytes, and the SpMV's row split"""
        out = np.zeros(KEY_INFO_WORDS, dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_groth16_key_info(self.handle, out.ctypes.data))
        names = ("resident_bytes", "lane_rows", "wave_rows", "terms", "unit_terms", "long_row_threshold", "committed_wires", "commitments")
        return {k: int(out[i]) for i, k in enumerate(names)}

    def close(self):
        if self.handle and self.ctx.handle:
            dll.nlx_bn254_groth16_key_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def r1cs_eval(pk, witness):
    """A w, B w, C w.  witness: (n_wires, 4) fr.Element words, numpy or a device tensor; returns (3, 2^log_n, 4) of the same kind
    (rows past n_constraints are zero)."""
    n = 1 << pk.log_n
    if hasattr(witness, "data_ptr"):
        import torch
        if tuple(witness.shape) != (pk.n_wires, 4) or not witness.is_contiguous():
            raise ValueError("expected a contiguous (n_wires, 4) tensor")
        out = torch.empty((3, n, 4), dtype=witness.dtype, device=witness.device)
        w_ptr, o_ptr = witness.data_ptr(), out.data_ptr()
    else:
        witness = np.ascontiguousarray(witness, dtype=np.uint64)
        if witness.shape != (pk.n_wires, 4):
            raise ValueError("expected shape (n_wires, 4)")
        out = np.zeros((3, n, 4), dtype=np.uint64)
        w_ptr, o_ptr = witness.ctypes.data, out.ctypes.data
    pk.ctx.check(dll.nlx_bn254_r1cs_eval(pk.ctx.handle, pk.handle, w_ptr, o_ptr, o_ptr + n * 32, o_ptr + 2 * n * 32))
    return out


def prove(pk, witness, r=None, s=None, abc=None):
    """One proof: (ar, bs, krs) as 8 / 16 / 8 words.  r, s: the blinding scalars (integers below r; from `secrets` when not
    given); abc: the solver's (a, b, c), each (2^log_n, 4) words, numpy or device - otherwise computed from the key's matrices."""
    r = secrets.randbelow(R) if r is None else int(r)
    s = secrets.randbelow(R) if s is None else int(s)
    if not (0 <= r < R and 0 <= s < R):
        raise ValueError("r and s must be below the group order")
    wk, w_ptr, rows = _buf(witness, np.uint64, 4)
    if rows != pk.n_wires:
        raise ValueError("the witness has %d rows, the key %d wires" % (rows, pk.n_wires))
    keep, ptrs = [], [None, None, None]
    if abc is not None:
        for i, v in enumerate(abc):
            k, p, rows = _buf(v, np.uint64, 4)
            if rows != 1 << pk.log_n:
                raise ValueError("a, b, c hold 2^log_n rows")
            keep.append(k)
            ptrs[i] = p
    rw, sw = fr_words(r), fr_words(s)
    ar, bs, krs = np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    pk.ctx.check(dll.nlx_bn254_groth16_prove(pk.ctx.handle, pk.handle, w_ptr, ptrs[0], ptrs[1], ptrs[2], ptr(rw), ptr(sw),
                                             ptr(ar), ptr(bs), ptr(krs)))
    return ar, bs, krs


def _lex_largest(y):
    return int(y) > (Q - 1) // 2


def g1_compress(words):
    """G1Affine.Bytes(): x big-endian, 0b10 / 0b11 in the top two bits for the smaller / larger y, 0b01 for infinity"""
    p = B.bn254_g1_unpack(words)
    if p is None:
        return bytes([0x40]) + bytes(31)
    b = bytearray(p[0].to_bytes(32, "big"))
    b[0] |= 0xC0 if _lex_largest(p[1]) else 0x80
    return bytes(b)


def g2_compress(words):
    """G2Affine.Bytes(): X.A1 || X.A0 big-endian, flags as for G1; "largest" Y decided on Y.A1, on Y.A0 when Y.A1 is zero"""
    p = B.bn254_g2_unpack(words)
    if p is None:
        return bytes([0x40]) + bytes(63)
    (x0, x1), (y0, y1) = p
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))
    b[0] |= 0xC0 if _lex_largest(y0 if y1 == 0 else y1) else 0x80
    return bytes(b)


def proof_bytes(ar, bs, krs, commitments=(), pok=None):
    """gnark's Proof.WriteTo: Ar, Bs, Krs compressed, the Commitments slice (uint32 k, big-endian, then k compressed points) and
    CommitmentPok (compressed; the point at infinity without commitments) - 164 + 32 k bytes"""
    return (g1_compress(ar) + g2_compress(bs) + g1_compress(krs) + len(commitments).to_bytes(4, "big")
            + b"".join(g1_compress(c) for c in commitments) + (bytes([0x40]) + bytes(31) if pok is None else g1_compress(pok)))


# ---- keys with Bsb22 / Pedersen commitments ----
def _witness_values(witness, ids):
    """the integers of a few wires of a witness (numpy or a device tensor)"""
    if not ids:
        return []
    if hasattr(witness, "data_ptr"):
        import torch
        rows = witness[torch.as_tensor(ids, device=witness.device)].cpu().numpy().view(np.uint64)
    else:
        rows = np.asarray(witness, dtype=np.uint64)[ids]
    return fr_unpack(rows)


def commit(pk, j, witness):
    """C_j = sum_i w[PrivateCommitted_j[i]] Basis_j[i] as 8 G1Affine words - what a solver's hint computes while it solves: only
    the wires of PrivateCommitted_j need to be filled."""
    _, w_ptr, rows = _buf(witness, np.uint64, 4)
    if rows != pk.n_wires:
        raise ValueError("the witness has %d rows, the key %d wires" % (rows, pk.n_wires))
    out = np.zeros(8, dtype=np.uint64)
    pk.ctx.check(dll.nlx_bn254_groth16_commit(pk.ctx.handle, pk.handle, int(j), w_ptr, ptr(out)))
    return out


def commitment_challenge(pk, j, point, witness):
    """the value commitment j's wire must hold: fr.Hash(C_j.Marshal() || the PublicAndCommitmentCommitted_j values, 32 bytes
    big-endian each, "bsb22-commitment", 1)[0].  point: C_j's words; of the witness only those wires are read."""
    hashed = _witness_values(witness, pk.commitments[j]["public"])
    return hash_to_field(g1_marshal(point) + b"".join(fr_bytes(v) for v in hashed), COMMITMENT_DST)


def prove_committed(pk, witness, r=None, s=None, abc=None):
    """One proof on a key with commitments: (ar, bs, krs, [C_j], pok).  r, s, abc as for prove().  The folding challenge rho is
    fr.Hash(the k commitment-wire values, "G16-BSB22"); every C_j is recomputed from the finished witness, and the value of its
    wire is checked against the challenge the returned C_j gives: NlxError (NLX_E_INVAL, naming the commitment) if not."""
    r = secrets.randbelow(R) if r is None else int(r)
    s = secrets.randbelow(R) if s is None else int(s)
    if not (0 <= r < R and 0 <= s < R):
        raise ValueError("r and s must be below the group order")
    wk, w_ptr, rows = _buf(witness, np.uint64, 4)
    if rows != pk.n_wires:
        raise ValueError("the witness has %d rows, the key %d wires" % (rows, pk.n_wires))
    keep, ptrs = [], [None, None, None]
    if abc is not None:
        for i, v in enumerate(abc):
            k_, p, rows = _buf(v, np.uint64, 4)
            if rows != 1 << pk.log_n:
                raise ValueError("a, b, c hold 2^log_n rows")
            keep.append(k_)
            ptrs[i] = p
    k = len(pk.commitments)
    wire_values = _witness_values(wk, [c["wire"] for c in pk.commitments])
    rho = hash_to_field(b"".join(fr_bytes(v) for v in wire_values), FOLD_DST)
    rw, sw, rhow = fr_words(r), fr_words(s), fr_words(rho)
    ar, bs, krs = np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    cs, pok = np.zeros((max(k, 1), 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    pk.ctx.check(dll.nlx_bn254_groth16_prove_committed(pk.ctx.handle, pk.handle, w_ptr, ptrs[0], ptrs[1], ptrs[2], ptr(rw), ptr(sw), ptr(rhow),
                                                       ptr(ar), ptr(bs), ptr(krs), ptr(cs), ptr(pok)))
    for j in range(k):
        if commitment_challenge(pk, j, cs[j], wk) != wire_values[j]:
            raise NlxError(NLX_E_INVAL, "commitment %d: wire %d does not hold the challenge of the witness's own commitment"
                           % (j, pk.commitments[j]["wire"]))
    return ar, bs, krs, [cs[j] for j in range(k)], pok


# ---- the verifier (csrc/bn254_pairing.hip; the model with real pairings is tools/bn254_pairing_model.py) ----
VERIFY_ACCEPT, VERIFY_MALFORMED, VERIFY_PEDERSEN, VERIFY_PAIRING = 0, 1, 2, 3
_REASONS = {VERIFY_ACCEPT: "accepted", VERIFY_MALFORMED: "malformed", VERIFY_PEDERSEN: "the Pedersen proof of knowledge fails",
            VERIFY_PAIRING: "the pairing equation fails"}


class _VkDesc(ctypes.Structure):
    """nlx_bn254_groth16_vk_desc (include/nlx.h)"""
    _fields_ = [("g1_alpha", ctypes.c_void_p), ("g2_beta", ctypes.c_void_p), ("g2_gamma", ctypes.c_void_p), ("g2_delta", ctypes.c_void_p),
                ("ic", ctypes.c_void_p), ("n_ic", ctypes.c_uint64), ("n_public", ctypes.c_uint32), ("n_commitments", ctypes.c_uint32),
                ("n_hashed", ctypes.c_void_p), ("hashed", ctypes.c_void_p), ("pedersen_g", ctypes.c_void_p),
                ("pedersen_g_root_sigma_neg", ctypes.c_void_p)]


class Verdict(ctypes.Structure):
    """nlx_bn254_verdict: accepted, and for a rejected proof the first reason in gnark's order and the point it names"""
    _fields_ = [("accepted", ctypes.c_uint32), ("reason", ctypes.c_uint32), ("index", ctypes.c_uint32)]

    k = None      # the key's commitment count, set by VerifyingKey.verify_many: what tells C_j from Pok

    def point_name(self):
        i, k = int(self.index), self.k
        if i < 3:
            return ("Ar", "Bs", "Krs")[i]
        if k is None:
            return "point %d (C_%d, or Pok after %d commitments)" % (i, i - 3, i - 3)
        return "Pok" if i == 3 + k else "C_%d" % (i - 3)

    def __bool__(self):
        return bool(self.accepted)

    def __str__(self):
        if self.accepted:
            return "accepted"
        text = "rejected: " + _REASONS.get(int(self.reason), "reason %d" % self.reason)
        return text + (" at " + self.point_name() if self.reason == VERIFY_MALFORMED else "")

    def raise_if_rejected(self):
        if not self.accepted:
            raise NlxError(NLX_E_INVAL, "Groth16 proof " + str(self))
        return self


class VerifyingKey:
    """nlx_bn254_groth16_vk: gnark's groth16.VerifyingKey resident on the device (owns the handle; close() or the context's
    close() releases it).  g1_alpha: 8 words; g2_beta, g2_gamma, g2_delta: 16 words; ic: (n_public + k, 8) words - G1.K over the
    public wires (the constant wire first), then one point per commitment wire.  commitments: one dict per Bsb22 commitment with
    "public" = PublicAndCommitmentCommitted as positions in ic (a public wire's id, or n_public + i for commitment i's wire);
    pedersen: the Pedersen verifying key's (G, GRootSigmaNeg), 16 words each - needed when there are commitments."""

    def __init__(self, ctx, n_public, g1_alpha, g2_beta, g2_gamma, g2_delta, ic, commitments=(), pedersen=None, n_ic=None):
        self.ctx, self.handle = ctx, None
        self.n_public, self.k = int(n_public), len(commitments)
        keep = {}
        d = _VkDesc()
        for name, arr, count in (("g1_alpha", g1_alpha, 8), ("g2_beta", g2_beta, 16), ("g2_gamma", g2_gamma, 16), ("g2_delta", g2_delta, 16)):
            keep[name] = np.ascontiguousarray(arr, dtype=np.uint64).reshape(count)
            setattr(d, name, keep[name].ctypes.data)
        keep["ic"] = np.ascontiguousarray(ic, dtype=np.uint64).reshape(-1, 8)
        d.ic, d.n_ic = keep["ic"].ctypes.data, len(keep["ic"]) if n_ic is None else int(n_ic)
        d.n_public, d.n_commitments = self.n_public, self.k
        if self.k:
            if pedersen is None:
                raise ValueError("a key with commitments needs the Pedersen verifying key")
            keep["n_hashed"] = np.array([len(c["public"]) for c in commitments], dtype=np.uint32)
            keep["hashed"] = np.array([i for c in commitments for i in c["public"]] + [0], dtype=np.uint32)
            keep["ped"] = [np.ascontiguousarray(p, dtype=np.uint64).reshape(16) for p in pedersen]
            d.n_hashed, d.hashed = keep["n_hashed"].ctypes.data, keep["hashed"].ctypes.data
            d.pedersen_g, d.pedersen_g_root_sigma_neg = keep["ped"][0].ctypes.data, keep["ped"][1].ctypes.data
        h = ctypes.c_void_p()
        ctx.check(dll.nlx_bn254_groth16_vk_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)

    def verify_many(self, proofs, publics):
        """One Verdict per proof.  proofs: the bytes of Proof.WriteTo (proof_bytes); publics: per proof the n_public - 1 public
        inputs (wires 1 .. n_public - 1) as integers.  The whole batch is the same five launches as one proof.  An integer not
        below r raises NlxError (NLX_E_RANGE)."""
        if not self.handle:
            raise NlxError(NLX_E_INVAL, "the verifying key is closed")
        n = len(proofs)
        if len(publics) != n or any(len(p) != self.n_public - 1 for p in publics):
            raise ValueError("one list of n_public - 1 public inputs per proof")
        blobs = [bytes(p) for p in proofs]
        ptrs = (ctypes.c_char_p * max(n, 1))(*blobs)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in blobs])
        words = np.zeros((max(n * (self.n_public - 1), 1), 4), dtype=np.uint64)
        row = 0
        for p in publics:
            for x in p:
                x = int(x)
                if not 0 <= x < (1 << 256):
                    raise NlxError(NLX_E_RANGE, "proof %d: a public input does not fit four words" % (row // max(self.n_public - 1, 1)))
                m = x * _MONT % R if x < R else x               # r <= x < 2^256 is no residue: its words go as they are and the library refuses them
                for w in range(4):
                    words[row, w] = (m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
                row += 1
        verdicts = (Verdict * max(n, 1))()
        self.ctx.check(dll.nlx_bn254_groth16_verify_batch(self.handle, ptrs, lens, n, words.ctypes.data, verdicts))
        out = []
        for i in range(n):
            v = Verdict(verdicts[i].accepted, verdicts[i].reason, verdicts[i].index)
            v.k = self.k
            out.append(v)
        return out

    def verify(self, proof, public=()):
        """nlx_bn254_groth16_verify: one proof's Verdict"""
        return self.verify_many([proof], [list(public)])[0]

    def close(self):
        if self.handle and self.ctx.handle:
            dll.nlx_bn254_groth16_vk_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- setup from a trapdoor (csrc/bn254_groth16_setup.hip; rules: tools/groth16_model.py rule 3, tools/groth16_commit_model.py rule 1) ----
SETUP_INFO_WORDS = 8
(SETUP_G1_A, SETUP_G1_B, SETUP_G2_B, SETUP_G1_K, SETUP_G1_Z, SETUP_INFINITY_A, SETUP_INFINITY_B, SETUP_G1_ALPHA, SETUP_G1_BETA,
 SETUP_G1_DELTA, SETUP_G2_BETA, SETUP_G2_DELTA, SETUP_BASIS, SETUP_BASIS_EXP_SIGMA, SETUP_G2_GAMMA, SETUP_IC, SETUP_PEDERSEN_G,
 SETUP_PEDERSEN_G_ROOT_SIGMA_NEG) = range(18)


class _SetupDesc(ctypes.Structure):
    """nlx_bn254_groth16_setup_desc (include/nlx.h)"""
    _fields_ = ([("log_n", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_wires", ctypes.c_uint64), ("n_public", ctypes.c_uint64),
                 ("n_constraints", ctypes.c_uint64)]
                + [(k, ctypes.c_void_p) for k in ("a_row_ptr", "b_row_ptr", "c_row_ptr", "a_wire", "b_wire", "c_wire",
                                                  "a_coeff_id", "b_coeff_id", "c_coeff_id", "coeffs")]
                + [("n_coeffs", ctypes.c_uint64)]
                + [(k, ctypes.c_void_p) for k in ("tau", "alpha", "beta", "gamma", "delta")]
                + [("n_commitments", ctypes.c_uint32), ("n_private", ctypes.c_void_p), ("private_wires", ctypes.c_void_p),
                   ("commitment_wires", ctypes.c_void_p), ("sigma", ctypes.c_void_p)])


class Trapdoor:
    """The setup's toxic waste: tau, alpha, beta, gamma, delta and, for keys with commitments, the Pedersen sigma - integers in
    1 .. r - 1 (the library refuses anything else, and a tau inside the domain).  Whoever keeps it can forge proofs."""

    def __init__(self, tau, alpha, beta, gamma, delta, sigma=None):
        self.tau, self.alpha, self.beta, self.gamma, self.delta = int(tau), int(alpha), int(beta), int(gamma), int(delta)
        self.sigma = None if sigma is None else int(sigma)

    @classmethod
    def random(cls):
        return cls(*(1 + secrets.randbelow(R - 1) for _ in range(6)))


def _trapdoor_words(x):
    x = int(x)
    if not 0 <= x < (1 << 256):
        raise NlxError(NLX_E_RANGE, "a trapdoor value does not fit four words")
    m = x * _MONT % R if x < R else x              # r <= x < 2^256 is no residue: its words go as they are and the library refuses them
    return np.array([(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)], dtype=np.uint64)


class SetupArrays:
    """gnark's ProvingKey and VerifyingKey arrays of one setup as numpy words (G1Affine 8, G2Affine 16, Montgomery): g1_a, g1_b,
    g2_b, g1_k, g1_z, infinity_a, infinity_b, g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta, commitments (per commitment
    {"basis", "basis_exp_sigma"}), and g2_gamma, ic, pedersen_g, pedersen_g_root_sigma_neg (None without commitments)."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)


class Setup:
    """struct nlx_bn254_groth16_setup: the result of gnark's groth16.Setup from a trapdoor, resident on the device (owns the
    handle).  r1cs as for ProvingKey (required); commitments: one dict per Bsb22 commitment - "private", "public", "wire" as for
    ProvingKey, optionally "hashed" (the verifier's PublicAndCommitmentCommitted as positions in ic; by default "public" with
    commitment i's wire as n_public + i)."""

    def __init__(self, ctx, log_n, n_wires, n_public, n_constraints, r1cs, trapdoor, commitments=None, flags=NLX_BN254_MONTGOMERY):
        self.ctx, self.handle = ctx, None
        self.log_n, self.n_wires, self.n_public, self.n_constraints = int(log_n), int(n_wires), int(n_public), int(n_constraints)
        self.commitments = [] if commitments is None else [dict(c) for c in commitments]
        d = _SetupDesc()
        d.log_n, d.flags, d.n_wires, d.n_public, d.n_constraints = self.log_n, int(flags), self.n_wires, self.n_public, self.n_constraints
        keep = []
        for m in "ABC":
            rows = {}
            for field, arr, dt in zip(("row_ptr", "wire", "coeff_id"), r1cs[m], (np.uint64, np.uint32, np.uint32)):
                k, p, rows[field] = _buf(arr, dt, 0)
                keep.append(k)
                setattr(d, "%s_%s" % (m.lower(), field), p)
            if rows["row_ptr"] != self.n_constraints + 1 or rows["wire"] != rows["coeff_id"]:
                raise ValueError("matrix %s: row_ptr holds n_constraints + 1 offsets, wire and coeff_id one entry per term" % m)
            last = int(r1cs[m][0][-1]) if rows["row_ptr"] else 0
            if last > rows["wire"]:
                raise ValueError("matrix %s: row_ptr ends at %d, the matrix holds %d terms" % (m, last, rows["wire"]))
        k, p, rows = _buf(r1cs["coeffs"], np.uint64, 4)
        keep.append(k)
        d.coeffs, d.n_coeffs = p, rows
        for name in ("tau", "alpha", "beta", "gamma", "delta"):
            w = _trapdoor_words(getattr(trapdoor, name))
            keep.append(w)
            setattr(d, name, w.ctypes.data)
        d.n_commitments = len(self.commitments)
        if self.commitments:
            if trapdoor.sigma is None:
                raise ValueError("a setup with commitments needs the trapdoor's sigma")
            counts = np.array([len(c["private"]) for c in self.commitments], dtype=np.uint64)
            ids = np.array([i for c in self.commitments for i in c["private"]] + [0], dtype=np.uint32)
            wires = np.array([c["wire"] for c in self.commitments], dtype=np.uint32)
            sigma = _trapdoor_words(trapdoor.sigma)
            keep += [counts, ids, wires, sigma]
            d.n_private, d.private_wires, d.commitment_wires, d.sigma = counts.ctypes.data, ids.ctypes.data, wires.ctypes.data, sigma.ctypes.data
        h = ctypes.c_void_p()
        ctx.check(dll.nlx_bn254_groth16_setup(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        self.handle = h
        ctx._adopt(self)

    def info(self):
        out = np.zeros(SETUP_INFO_WORDS, dtype=np.uint64)
        self.ctx.check(dll.nlx_bn254_groth16_setup_info(self.handle, out.ctypes.data))
        names = ("g1_a", "g1_b", "g1_k", "g1_z", "committed_wires", "commitments", "ic", "wave_wires")
        return {k: int(out[i]) for i, k in enumerate(names)}

    def read(self, which, device=None):
        """one array (SETUP_*): numpy words, or an int64 device tensor with device="cuda:k" (the masks: uint8)"""
        info = self.info()
        rows = {SETUP_G1_A: info["g1_a"], SETUP_G1_B: info["g1_b"], SETUP_G2_B: info["g1_b"], SETUP_G1_K: info["g1_k"], SETUP_G1_Z: info["g1_z"],
                SETUP_INFINITY_A: self.n_wires, SETUP_INFINITY_B: self.n_wires, SETUP_BASIS: info["committed_wires"],
                SETUP_BASIS_EXP_SIGMA: info["committed_wires"], SETUP_IC: info["ic"]}.get(which, 1)
        mask = which in (SETUP_INFINITY_A, SETUP_INFINITY_B)
        width = 16 if which in (SETUP_G2_B, SETUP_G2_BETA, SETUP_G2_DELTA, SETUP_G2_GAMMA, SETUP_PEDERSEN_G, SETUP_PEDERSEN_G_ROOT_SIGMA_NEG) else 8
        if device is not None:
            import torch
            out = torch.zeros((rows,) if mask else (rows, width), dtype=torch.uint8 if mask else torch.int64, device=device)
            self.ctx.check(dll.nlx_bn254_groth16_setup_read(self.handle, which, out.data_ptr() if rows else None))
            return out
        out = np.zeros((rows,) if mask else (rows, width), dtype=np.uint8 if mask else np.uint64)
        self.ctx.check(dll.nlx_bn254_groth16_setup_read(self.handle, which, out.ctypes.data if rows else None))
        return out

    def arrays(self):
        k = len(self.commitments)
        a = {name: self.read(which) for name, which in (
            ("g1_a", SETUP_G1_A), ("g1_b", SETUP_G1_B), ("g2_b", SETUP_G2_B), ("g1_k", SETUP_G1_K), ("g1_z", SETUP_G1_Z),
            ("infinity_a", SETUP_INFINITY_A), ("infinity_b", SETUP_INFINITY_B), ("ic", SETUP_IC))}
        for name, which in (("g1_alpha", SETUP_G1_ALPHA), ("g1_beta", SETUP_G1_BETA), ("g1_delta", SETUP_G1_DELTA), ("g2_beta", SETUP_G2_BETA),
                            ("g2_delta", SETUP_G2_DELTA), ("g2_gamma", SETUP_G2_GAMMA)):
            a[name] = self.read(which)[0]
        basis, sigma = self.read(SETUP_BASIS), self.read(SETUP_BASIS_EXP_SIGMA)
        a["commitments"], at = [], 0
        for c in self.commitments:
            a["commitments"].append({"basis": basis[at:at + len(c["private"])], "basis_exp_sigma": sigma[at:at + len(c["private"])]})
            at += len(c["private"])
        a["pedersen_g"] = self.read(SETUP_PEDERSEN_G)[0] if k else None
        a["pedersen_g_root_sigma_neg"] = self.read(SETUP_PEDERSEN_G_ROOT_SIGMA_NEG)[0] if k else None
        return SetupArrays(**a)

    def proving_key_bytes(self, raw=False):
        """gnark's groth16.ProvingKey.WriteTo (raw: WriteRawTo) of this setup's proving key: the domain, G1 Alpha Beta Delta and
        the slices A B Z K, G2 Beta Delta and the slice B, nbWires NbInfinityA NbInfinityB and the two masks, the commitment keys
        (tools/gnark_bytes_model.py rule 10, recalled and unpinned).  Each slice is read on the device and encoded there in one
        call; only the bytes come to the host."""
        from . import bn254_codec as C
        dev = "cuda:%d" % self.ctx.device
        one = lambda which: self.read(which)
        out = [domain_bytes(self.log_n)]
        out += [C.bn254_g1_encode(self.ctx, one(w), raw) for w in (SETUP_G1_ALPHA, SETUP_G1_BETA, SETUP_G1_DELTA)]
        out += [C.slice_bytes(self.ctx, False, self.read(w, device=dev), raw) for w in (SETUP_G1_A, SETUP_G1_B, SETUP_G1_Z, SETUP_G1_K)]
        out += [C.bn254_g2_encode(self.ctx, one(w), raw) for w in (SETUP_G2_BETA, SETUP_G2_DELTA)]
        out.append(C.slice_bytes(self.ctx, True, self.read(SETUP_G2_B, device=dev), raw))
        inf_a, inf_b = self.read(SETUP_INFINITY_A), self.read(SETUP_INFINITY_B)
        out += [C.u64(self.n_wires), C.u64(int((inf_a != 0).sum())), C.u64(int((inf_b != 0).sum()))]
        out += [C.u32(len(m)) + (m != 0).astype(np.uint8).tobytes() for m in (inf_a, inf_b)]
        out.append(C.u32(len(self.commitments)))
        basis, sigma, at = self.read(SETUP_BASIS), self.read(SETUP_BASIS_EXP_SIGMA), 0
        for c in self.commitments:
            m = len(c["private"])
            out += [C.slice_bytes(self.ctx, False, basis[at:at + m], raw), C.slice_bytes(self.ctx, False, sigma[at:at + m], raw)]
            at += m
        return b"".join(out)

    def key(self):
        """nlx_bn254_groth16_setup_key: the resident ProvingKey, built from the device arrays"""
        h = ctypes.c_void_p()
        self.ctx.check(dll.nlx_bn254_groth16_setup_key(self.handle, ctypes.byref(h)))
        return ProvingKey._from_handle(self.ctx, h, self.log_n, self.n_wires, self.n_public, self.n_constraints, self.commitments)

    def verifying_key(self):
        """the VerifyingKey of this setup (the verifying side is a few points: read to the host and handed to its creation)"""
        k = len(self.commitments)
        one = lambda which: self.read(which)[0]
        wire_at = {int(c["wire"]): self.n_public + i for i, c in enumerate(self.commitments)}
        hashed = [{"public": [int(i) for i in c["hashed"]] if "hashed" in c else [wire_at.get(int(i), int(i)) for i in c["public"]]}
                  for c in self.commitments]
        pedersen = (one(SETUP_PEDERSEN_G), one(SETUP_PEDERSEN_G_ROOT_SIGMA_NEG)) if k else None
        return VerifyingKey(self.ctx, self.n_public, one(SETUP_G1_ALPHA), one(SETUP_G2_BETA), one(SETUP_G2_GAMMA), one(SETUP_G2_DELTA),
                            self.read(SETUP_IC), commitments=hashed, pedersen=pedersen)

    def close(self):
        if self.handle and self.ctx.handle:
            dll.nlx_bn254_groth16_setup_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def setup(ctx, log_n, n_wires, n_public, n_constraints, r1cs, trapdoor=None, commitments=None):
    """gnark's groth16.Setup(r1cs) on the device: (ProvingKey, VerifyingKey, SetupArrays).  trapdoor: a Trapdoor (drawn from
    `secrets` when not given, and then gone with this call: nothing returned can forge).  The rules are recalled from gnark v0.9
    and unpinned (tools/groth16_model.py rule 3, tools/groth16_commit_model.py rule 1)."""
    s = Setup(ctx, log_n, n_wires, n_public, n_constraints, r1cs, Trapdoor.random() if trapdoor is None else trapdoor, commitments)
    try:
        return s.key(), s.verifying_key(), s.arrays()
    finally:
        s.close()
