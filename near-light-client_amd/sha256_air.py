"""SHA-256 compression as an AIR for the STARK prover.

nearx hashes headers, Merkle nodes and approval messages with `curta_sha256` (nearx/src/variables.rs:71-72,
nearx/src/merkle.rs:49, nearx/src/builder.rs:220,316); curta proves those hashes with a STARK whose AIR is
not in the reference (starkyx is un-vendored).  This is an independent AIR for the same function, written
for the register-program VM of include/nlx.h and laid out for the MI355X: a WIDE trace, sixteen rounds per
row and four rows per 512-bit block, so that every state bit is stored exactly once.  A narrow one-round-per-row
layout has to carry copies of the working variables and of the message window from row to row (302 columns x 64
rows = 19 328 cells per block in the first version of this file); here a row sees the sixteen rounds before it
through the (local, next) window, and a block costs 4 x 1 953 = 7 812 cells - 2.5x less to extend, hash and open.
All constraints have degree <= 3, so the quotient fits two chunks at rate_bits = 1.

Row layout.  Round slot j (0..15) of a row holds, for round t = 16 q + j of its block (q = row within the block):

    A[32], E[32]    bits of the working variables a_t, e_t produced by round t      (LSB first)
    W[32]           bits of the schedule word W_t
    CA[3], CE[3]    carry bits of the two additions of the round;  CW[2] carries of the schedule addition
    SW              the word the schedule recurrence gives for this slot (equal to W_t in rows q >= 1)

followed by

    PA[4][32], PE[4][32]   bits of a_{t0-1..t0-4}, e_{t0-1..t0-4} (t0 = 16 q): the state the row starts from
    HIN[8]                 the block's input chaining value (constant over its four rows)
    CY[8]                  carries of HIN + final state (meaningful in the last row of a block)
    IS_FIRST               1 in the first row of a block that starts a new message (chaining value = IV)

Periodic columns (period 4 rows): K_t for each of the sixteen slots, the first-row and last-row selectors.
The program (15 k instructions) is cut into segments (NLX_AIR_SEGMENT) that the GPU evaluates in parallel.
Every constraint is an all-rows constraint: a block boundary either chains or resets to the IV, so the relations
between consecutive rows also hold across the wrap from the last row to the first.

Soundness notes: a word that only ever enters additions (HIN, SW) may be off by a multiple of 2^32 without
consequence, because every sum is re-derived from boolean bit columns and the carries are bounded; equalities
between boolean vectors are enforced as packed-word equalities.  Public inputs: the eight words of the last
block's output chaining value (the digest of the last message).
"""
from ._sha2 import ROWS_PER_BLOCK, Sha2, Sha2Prover   # noqa: F401
from .stark import STEP_TAG_LEN, Air

_H = Sha2(32, 64, 16, s0=(7, 18, 3), s1=(17, 19, 10), S0=(2, 13, 22), S1=(6, 11, 25))
ROUNDS, SLOTS = _H.ROUNDS, _H.SLOTS   # sixteen rounds per row
SLOT = _H.SLOT                  # 105 columns per round slot
oA, oE, oW, oCA, oCE, oCW, oSW = _H.offsets   # 0, 32, 64, 96, 99, 102, 104
PA, PE, HIN, CY, IS_FIRST = _H.PA, _H.PE, _H.HIN, _H.CY, _H.IS_FIRST   # 1680, 1808, 1936, 1944, 1952
N_COLS = IS_FIRST + 1           # 1953 (round 0)
ACC = N_COLS                    # round 1: the binding accumulator, one element of F_p^2 = two base columns
assert (SLOT, N_COLS) == (105, 1953)

K, IV = _H.K, _H.IV             # FIPS 180-4 §4.2.2 / §5.3.3
assert K[0] == 0x428a2f98 and K[63] == 0xc67178f2 and IV[0] == 0x6a09e667 and IV[7] == 0x5be0cd19


def sha256_air(tagged=False):
    air = Air(N_COLS + 2, 8 + (STEP_TAG_LEN if tagged else 0), rounds=[(N_COLS, 2), (2, 0)], round_values=[0, 2])   # tagged: public inputs 8..11 = the step tag
    L, N = air.local, air.next  # noqa: N806
    two32 = 1 << 32
    k_slot = [air.periodic([K[16 * q + j] for q in range(4)]) for j in range(16)]
    is_q0 = air.periodic([1, 0, 0, 0])
    is_q3 = air.periodic([0, 0, 0, 1])

    def weighted(terms):
        acc = terms[0]
        for i in range(1, 32):
            acc = acc + terms[i] * (1 << i)
        return acc

    # bit vectors of a_t / e_t for t relative to the row start (-4..15), on the local row
    def a_bits(t):
        base = t * SLOT + oA if t >= 0 else PA + 32 * (-t - 1)
        return [L(base + i) for i in range(32)]

    def e_bits(t):
        base = t * SLOT + oE if t >= 0 else PE + 32 * (-t - 1)
        return [L(base + i) for i in range(32)]

    def a_word(t, row_next=False):
        return air.pack(t * SLOT + oA if t >= 0 else PA + 32 * (-t - 1), 32, next_row=row_next)

    def e_word(t, row_next=False):
        return air.pack(t * SLOT + oE if t >= 0 else PE + 32 * (-t - 1), 32, next_row=row_next)

    # schedule words relative to the CURRENT row = `next`; negative indices reach into `local` (the previous row)
    def w_bits_cur(t):
        return [N(t * SLOT + oW + i) for i in range(32)] if t >= 0 else [L((16 + t) * SLOT + oW + i) for i in range(32)]

    def w_word_cur(t):
        return air.pack(t * SLOT + oW, 32, next_row=True) if t >= 0 else air.pack((16 + t) * SLOT + oW, 32)

    # 1. booleanity: all bits of the sixteen slots, the start state, the boundary carries and the flag
    for j in range(16):
        air.constraint_boolean(j * SLOT, 104)
    air.constraint_boolean(PA, 256)
    air.constraint_boolean(CY, 9)

    # 2. the sixteen rounds of the row
    for j in range(16):
        a1, a2, a3 = a_bits(j - 1), a_bits(j - 2), a_bits(j - 3)
        e1, e2, e3 = e_bits(j - 1), e_bits(j - 2), e_bits(j - 3)
        sig1 = weighted([air.xor3(e1[(i + 6) % 32], e1[(i + 11) % 32], e1[(i + 25) % 32]) for i in range(32)])
        ch = weighted([air.ch(e1[i], e2[i], e3[i]) for i in range(32)])
        sig0 = weighted([air.xor3(a1[(i + 2) % 32], a1[(i + 13) % 32], a1[(i + 22) % 32]) for i in range(32)])
        maj = weighted([air.maj(a1[i], a2[i], a3[i]) for i in range(32)])
        t1 = e_word(j - 4) + sig1 + ch + k_slot[j] + air.pack(j * SLOT + oW, 32)
        air.constraint(a_word(j) + air.pack(j * SLOT + oCA, 3) * two32 - (t1 + sig0 + maj))
        air.constraint(e_word(j) + air.pack(j * SLOT + oCE, 3) * two32 - (a_word(j - 4) + t1))
        # in rows q >= 1 the schedule word IS the recurrence's value (row 0 holds the message block)
        air.constraint((1 - is_q0) * (air.pack(j * SLOT + oW, 32) - L(j * SLOT + oSW)))

    # 3. the schedule recurrence, written on the current (= next) row with the previous row behind it:
    #    SW_t + 2^32 cw = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16]
    for j in range(16):
        w2, w15 = w_bits_cur(j - 2), w_bits_cur(j - 15)
        s0 = weighted([air.xor3(w15[(i + 7) % 32], w15[(i + 18) % 32], w15[i + 3]) if i + 3 < 32
                       else air.xor3(w15[(i + 7) % 32], w15[(i + 18) % 32], 0) for i in range(32)])
        s1 = weighted([air.xor3(w2[(i + 17) % 32], w2[(i + 19) % 32], w2[i + 10]) if i + 10 < 32
                       else air.xor3(w2[(i + 17) % 32], w2[(i + 19) % 32], 0) for i in range(32)])
        air.constraint(N(j * SLOT + oSW) + air.pack(j * SLOT + oCW, 2, next_row=True) * two32
                       - (s1 + w_word_cur(j - 7) + s0 + w_word_cur(j - 16)))

    # 4. row to row inside a block: the next row starts from this row's last four rounds; HIN is carried along
    nb = 1 - is_q3
    for k in range(4):
        air.constraint(nb * (a_word(-k - 1, True) - a_word(15 - k)))
        air.constraint(nb * (e_word(-k - 1, True) - e_word(15 - k)))
    for k in range(8):
        air.constraint(nb * (N(HIN + k) - L(HIN + k)))

    # 5. block boundary (this row is the last of its block): the next block starts from IV or from HIN + final state
    out = [a_word(15), a_word(14), a_word(13), a_word(12), e_word(15), e_word(14), e_word(13), e_word(12)]
    nxt = [a_word(-1, True), a_word(-2, True), a_word(-3, True), a_word(-4, True),
           e_word(-1, True), e_word(-2, True), e_word(-3, True), e_word(-4, True)]
    ho = [L(HIN + k) + out[k] - L(CY + k) * two32 for k in range(8)]
    for k in range(8):
        air.constraint(is_q3 * (nxt[k] - ho[k] - N(IS_FIRST) * (IV[k] - ho[k])))
        air.constraint(is_q3 * (N(HIN + k) - nxt[k]))

    # 6. the first row starts a message; 7. the last row's output chaining value is the public digest
    cur = [a_word(-1), a_word(-2), a_word(-3), a_word(-4), e_word(-1), e_word(-2), e_word(-3), e_word(-4)]
    air.constraint_first_row(L(IS_FIRST) - 1)
    for k in range(8):
        air.constraint_first_row(cur[k] - IV[k])
    for k in range(8):
        air.constraint_last_row(ho[k] - air.public(k))

    # 8. binding: a challenge gamma in F_p^2 (drawn once the trace is committed) and a round-1 accumulator fold every
    # block's (message-start flag, 16 message words) - on its first row - and 8 output chaining words - on its last row -
    # into one Horner fingerprint; the total is a round value of the proof, which the relying party recomputes from the
    # messages it believes were hashed (fingerprint() below).  Each row holds what was absorbed before it.
    def ext_mul(x, y):
        return x[0] * y[0] + x[1] * y[1] * 7, x[0] * y[1] + x[1] * y[0]
    gamma = (air.challenge(0), air.challenge(1))

    def horner(start, elems):
        """((start gamma + e_0) gamma + e_1) .. gamma + e_last: a chain, so that few values are live at a time"""
        c0, c1 = start
        for e in elems:
            c0, c1 = ext_mul((c0, c1), gamma)
            c0 = c0 + e
        return c0, c1
    acc = (L(ACC), L(ACC + 1))
    after_head = horner(acc, [L(IS_FIRST)] + [air.pack(j * SLOT + oW, 32) for j in range(16)])   # 17 elements, rows q = 0
    after_tail = horner(acc, ho)                                                                  # 8 elements, rows q = 3
    for c in range(2):
        air.constraint_first_row(acc[c])
        air.constraint_transition(N(ACC + c) - (acc[c] + is_q0 * (after_head[c] - acc[c]) + is_q3 * (after_tail[c] - acc[c])))
        air.constraint_last_row(after_tail[c] - air.round_value(1, c))
    return air


# ---------------------------------------------------------------------------------------------
# host helpers (_sha2.py): padding, a plain-Python trace generator (tests only; the product path generates the trace on
# the GPU with nlx_sha256_trace), the binding fingerprint.  Blocks are uint32 [n_blocks, 16]; the public inputs are the eight
# digest words themselves (digest_halves is the identity on them).
# ---------------------------------------------------------------------------------------------
pad_message, blocks_for_messages, digest_halves = _H.pad_message, _H.blocks_for_messages, _H.digest_halves
reference_trace, block_outputs = _H.reference_trace, _H.block_outputs
fingerprint, binding_columns, cpu_rounds = _H.fingerprint, _H.binding_columns, _H.cpu_rounds


class Sha256Prover(Sha2Prover):
    """Sha2Prover for SHA-256: nlx_sha256_trace, nlx_sha256_bind_round and the AIR above."""
    sha2, build_air = _H, staticmethod(sha256_air)
    trace_fn, bind_fn = "nlx_sha256_trace", "nlx_sha256_bind_round"
