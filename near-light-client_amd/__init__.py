"""nlx_amd - MI355X-native prover backend for the nearx plonky2x circuits (host-side mirror).

The compute path is the HIP library `libnlx.so` (C ABI in include/nlx.h).  This package is
the thin host layer above it, mirroring the plonky2 / plonky2x interface names the reference
calls (nearx/src/test_utils.rs:29,62,66): PolynomialBatch, MerkleTree, prove, ...
There is NO CPU fallback: importing `nlx_amd.lib` raises if libnlx.so is missing, and creating
a Context raises if no gfx950 device is usable.
"""
from . import _lib as lib  # noqa: F401  (raises loudly when the HIP extension is absent)
from ._lib import Context, DeviceBuffer, NlxError, GOLDILOCKS_P  # noqa: F401
from .batch import PolynomialBatch, MerkleTree, poseidon_permute, hash_rows, poseidon_bn128_permute, poseidon_bn128_hash_rows, poseidon_bn128_merkle_verify, ntt, field_ops, ext_ops, fe25519_ops, bn254_ntt, bn254_pack, bn254_unpack, BN254_R, bn254_msm_g1, bn254_g1_pack, bn254_g1_unpack, bn254_g1_sum, bn254_g1_lincomb, bn254_g1_multiples, bn254_g1_scalar_muls, bn254_g2_scalar_muls, bn254_g2_pack, bn254_g2_unpack, bn254_msm_g2, bn254_g2_sum, BN254_Q, bn254_plonk_quotient, bn254_kzg_open, bn254_f29_ops, BN254_F29_OPS, bn254_pairing, bn254_pairing_check, bn254_gt_unpack  # noqa: F401
from .bn254_codec import bn254_g1_decode, bn254_g2_decode, bn254_g1_encode, bn254_g2_encode  # noqa: F401
from .plonk import CircuitConfig, CircuitData, SyntheticCircuit, VerifierData, WitnessReport, pow_grind, batch_prove, ProveJob  # noqa: F401
from .stark import Air, Stark, StarkConfig, StarkProver, TraceReport, Verdict, fibonacci_air, fibonacci_trace, wide_air, wide_trace  # noqa: F401
from . import sha256_air, sha512_air, logup, fp25519, ed25519_air, nearx_io, near_protocol, stark, plonk, succinct_io, split_ntt, bn254_plonk, bn254_groth16, bn254_codec  # noqa: F401,E402
