import sys; sys.path.insert(0, ".")
import nlxpkg; nlx = nlxpkg.load()
ctx = nlx.Context(0)
syn = nlx.SyntheticCircuit(14, seed=1, pct_poseidon=25, pct_arithmetic=20, pct_u32=15)
cd = nlx.CircuitData.from_synthetic(ctx, syn)
proof = cd.prove(syn.wires, syn.public_inputs)
cd.check_witness(syn.wires, syn.public_inputs).raise_if_unsatisfied()
cd.verify(proof).raise_if_rejected()
bn = nlx.CircuitData.from_synthetic(ctx, syn, hasher="poseidon_bn128"); bn.verify(bn.prove(syn.wires, syn.public_inputs)).raise_if_rejected()   # the same under plonky2x's PoseidonBN128GoldilocksConfig
print("plonky2 proof", len(proof))
S = nlx.stark
air = S.Air(2, 3)
air.constraint_transition(air.next(0) - air.local(1))
air.constraint_transition(air.next(1) - air.local(0) - air.local(1))
prover = S.Stark(air, 10).build(ctx)
proof = prover.prove(*S.fibonacci_trace(10)[:1], [0, 1, 0])
prover.check(*S.fibonacci_trace(10)[:1], [0, 1, 0]).raise_if_unsatisfied()
print("stark proof", len(proof))
digest_proof, digest = nlx.sha256_air.Sha256Prover(ctx, 4).prove([b"abc", b"hello"])
print("sha256", len(digest_proof))
E = nlx.ed25519_air
pk = bytes.fromhex("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a")
sig = bytes.fromhex("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b")
msg = b""
slots = [E.slot_from_signature(pk, msg, sig)] * 255 + [E.inactive_slot()]
ed_proof = E.Ed25519Prover(ctx, 8).prove(slots)
print("ed25519", len(ed_proof))
import numpy as np
pts = nlx.bn254_g1_pack([(1, 2), (1, 2)])
ks = np.array([[3, 0, 0, 0], [4, 0, 0, 0]], dtype=np.uint64)
print("msm 7G", nlx.bn254_g1_unpack(nlx.bn254_msm_g1(ctx, pts, ks)))
G = nlx.bn254_groth16
inf8, inf16 = np.zeros(8, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
one = np.array([1, 1], dtype=np.uint64)              # the circuit "w1 * w1 = w1" on the wires (ONE, w1); a key of points at infinity
r1cs = {m: (np.array([0, 1], dtype=np.uint64), np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)) for m in "ABC"}
r1cs["coeffs"] = G.fr_pack([1])
key = G.ProvingKey(ctx, 1, 2, 1, 1, inf8[None][:0], inf8[None][:0], inf16[None][:0], inf8[None], inf8[None], one, one, inf8, inf8, inf8, inf16, inf16, r1cs=r1cs)
groth16_proof = G.proof_bytes(*G.prove(key, G.fr_pack([1, 1])))
print("groth16", len(groth16_proof))
G.VerifyingKey(ctx, 1, inf8, inf16, inf16, inf16, inf8[None]).verify(groth16_proof).raise_if_rejected()   # the matching key of points at infinity: e(alpha, beta) = 1
spk, svk, _ = G.setup(ctx, 1, 2, 1, 1, r1cs)        # an honest key of the same circuit, from a trapdoor drawn and dropped
svk.verify(G.proof_bytes(*G.prove(spk, G.fr_pack([1, 1])))).raise_if_rejected()
print("groth16 setup -> prove -> verify")
print("hash_to_field", hex(nlx.bn254_plonk.hash_to_field_native(b"abc")) == hex(nlx.bn254_plonk.hash_to_field(b"abc")))   # the PLONK prover's host hash (ResidentKey / prove_resident: DESIGN.md section 23)
P = nlx.bn254_plonk
srs, g2, g2_tau = P.kzg_srs(ctx, 12345, 8 + 3)      # a TEST SRS from its trapdoor: whoever knows 12345 forges openings
pkey, ps = P.setup(ctx, 3, 1, [(1, 1, 2, 0, 0, 1, 2, 0)], [0, 1, P.R - 1], srs)   # x * x = y on the variables (public, x, y): qm = 1, qo = -1
l, r, o = ps.wires([9, 3, 9])                        # the solver's last step: variables -> wire columns on the device
P.VerifyingKey.from_resident(pkey, g2, g2_tau, 1).verify(P.prove_resident(pkey, l, r, o, [9]), [9]).raise_if_rejected()
print("plonk setup -> prove -> verify")
values, report = ps.solver(1).solve([9, 3])          # gnark's witness solver: the inputs (public, x) in, every variable out - y = 9 from x * x = y
report.raise_if_unsolved()
l, r, o = ps.wires(values)
P.VerifyingKey.from_resident(pkey, g2, g2_tau, 1).verify(P.prove_resident(pkey, l, r, o, [9]), [9]).raise_if_rejected()
print("plonk setup -> solve -> prove -> verify:", report)
ss = G.Setup(ctx, 1, 2, 1, 1, r1cs, G.Trapdoor.random())
key_file = ss.proving_key_bytes()                    # gnark's ProvingKey.WriteTo: the points through the device codec
read_key = G.ProvingKey.from_bytes(ctx, key_file, r1cs=r1cs)
ss.verifying_key().verify(G.proof_bytes(*G.prove(read_key, G.fr_pack([1, 1])))).raise_if_rejected()
print("groth16 key bytes", len(key_file))
srs_file = P.srs_to_bytes(ctx, srs, g2, g2_tau)      # kzg.SRS.WriteTo; raw=True for WriteRawTo's uncompressed points
print("srs bytes", len(srs_file), np.array_equal(P.srs_from_bytes(ctx, srs_file)[0], srs), nlx.bn254_g1_encode(ctx, nlx.bn254_g1_decode(ctx, srs_file[4:36])) == srs_file[4:36])
