"""SHA-512 compression as an AIR for the STARK prover.

Every Ed25519 verification nearx proves (`curta_eddsa_verify_sigs_conditional`, nearx/src/builder.rs:152) hashes
R || A || M with SHA-512 - for NEAR approvals 32 + 32 + 41 = 105 bytes, one 1024-bit block per signature.  curta's
AIR for it is not in the reference (starkyx is un-vendored); this is an independent AIR for the same function, the
64-bit sibling of sha256_air.py: a WIDE trace, twenty rounds per row and four rows per block, every state bit stored
once.  A 64-bit word does not fit a Goldilocks element uniquely, so every word is handled as two 32-bit halves and
every addition mod 2^64 is two additions mod 2^32 chained by the low half's carry.  All constraints have degree <= 3
(quotient factor 2 at rate_bits = 1).

Row layout.  Round slot j (0..19) of a row holds, for round t = 20 q + j of its block (q = row within the block):

    A[64], E[64]      bits of the working variables a_t, e_t produced by round t      (LSB first)
    W[64]             bits of the schedule word W_t
    CA[3+3], CE[3+3]  carry bits (low half, high half) of the two additions of the round
    CW[2+2]           carry bits of the schedule addition
    SW[2]             the halves of the word the schedule recurrence gives for this slot (= W_t in rows q >= 1)

followed by

    PA[4][64], PE[4][64]   bits of a_{t0-1..t0-4}, e_{t0-1..t0-4} (t0 = 20 q): the state the row starts from
    HIN[8][2]              the block's input chaining value as (low, high) halves, constant over its four rows
    CY[8][2]               carries of HIN + final state (meaningful in the last row of a block)
    IS_FIRST               1 in the first row of a block that starts a new message (chaining value = IV)

Periodic columns (period 4 rows): the halves of K_t for each of the twenty slots, the first-row-of-block and
last-row-of-block selectors.  Every constraint is an all-rows constraint (a block boundary either chains or resets
to the IV, so the row-to-row relations also hold across the wrap).  Public inputs: the sixteen halves (low, high per
word) of the last block's output chaining value - the digest of the last message.
"""
from ._sha2 import ROWS_PER_BLOCK, Sha2, Sha2Prover   # noqa: F401
from .stark import STEP_TAG_LEN, Air

_H = Sha2(64, 80, 20, s0=(1, 8, 7), s1=(19, 61, 6), S0=(28, 34, 39), S1=(14, 18, 41))
ROUNDS, SLOTS = _H.ROUNDS, _H.SLOTS   # twenty rounds per row
SLOT = _H.SLOT                  # 210 columns per round slot
oA, oE, oW, oCA, oCE, oCW, oSW = _H.offsets   # 0, 64, 128, 192, 198, 204, 208
PA, PE, HIN, CY, IS_FIRST = _H.PA, _H.PE, _H.HIN, _H.CY, _H.IS_FIRST   # 4200, 4456, 4712, 4728, 4744
N_COLS = IS_FIRST + 1           # 4745 (round 0)
ACC = N_COLS                    # round 1: the binding accumulator, one element of F_p^2 = two base columns
M64 = _H.MASK
assert (SLOT, N_COLS) == (210, 4745)

K, IV = _H.K, _H.IV             # FIPS 180-4 §4.2.3 / §5.3.5
assert K[0] == 0x428a2f98d728ae22 and K[79] == 0x6c44198c4a475817 and IV[0] == 0x6a09e667f3bcc908 and IV[7] == 0x5be0cd19137e2179
_halves = _H.halves


def sha512_air(tagged=False):
    air = Air(N_COLS + 2, 16 + (STEP_TAG_LEN if tagged else 0), rounds=[(N_COLS, 2), (2, 0)], round_values=[0, 2])   # tagged: public inputs 16..19 = the step tag
    L, N = air.local, air.next  # noqa: N806
    two32 = 1 << 32
    k_slot = [[air.periodic([_halves(K[SLOTS * q + j])[h] for q in range(4)]) for h in range(2)] for j in range(SLOTS)]
    is_q0 = air.periodic([1, 0, 0, 0])
    is_q3 = air.periodic([0, 0, 0, 1])

    def weighted(bits32):
        acc = bits32[0]
        for i in range(1, 32):
            acc = acc + bits32[i] * (1 << i)
        return acc

    def halves_of(bits64):
        return weighted(bits64[:32]), weighted(bits64[32:])

    def a_base(t):
        return t * SLOT + oA if t >= 0 else PA + 64 * (-t - 1)

    def e_base(t):
        return t * SLOT + oE if t >= 0 else PE + 64 * (-t - 1)

    def a_bits(t):
        return [L(a_base(t) + i) for i in range(64)]

    def e_bits(t):
        return [L(e_base(t) + i) for i in range(64)]

    def word(base, row_next=False):
        """(low half, high half) of the 64 bit columns starting at `base`"""
        return air.pack(base, 32, next_row=row_next), air.pack(base + 32, 32, next_row=row_next)

    # schedule words relative to the CURRENT row = `next`; negative indices reach into `local` (the previous row)
    def w_bits_cur(t):
        return [N(t * SLOT + oW + i) for i in range(64)] if t >= 0 else [L((SLOTS + t) * SLOT + oW + i) for i in range(64)]

    def w_word_cur(t):
        return word(t * SLOT + oW, True) if t >= 0 else word((SLOTS + t) * SLOT + oW)

    # 1. booleanity: all bits of the twenty slots, the start state, the boundary carries and the flag
    for j in range(SLOTS):
        air.constraint_boolean(j * SLOT, 208)
    air.constraint_boolean(PA, 512)
    air.constraint_boolean(CY, 17)

    # 2. the twenty rounds of the row
    for j in range(SLOTS):
        a1, a2, a3 = a_bits(j - 1), a_bits(j - 2), a_bits(j - 3)
        e1, e2, e3 = e_bits(j - 1), e_bits(j - 2), e_bits(j - 3)
        sig1 = halves_of([air.xor3(e1[(i + 14) % 64], e1[(i + 18) % 64], e1[(i + 41) % 64]) for i in range(64)])
        ch = halves_of([air.ch(e1[i], e2[i], e3[i]) for i in range(64)])
        sig0 = halves_of([air.xor3(a1[(i + 28) % 64], a1[(i + 34) % 64], a1[(i + 39) % 64]) for i in range(64)])
        maj = halves_of([air.maj(a1[i], a2[i], a3[i]) for i in range(64)])
        e4, a4 = word(e_base(j - 4)), word(a_base(j - 4))
        wj = word(j * SLOT + oW)
        an, en = word(a_base(j)), word(e_base(j))
        ca = (air.pack(j * SLOT + oCA, 3), air.pack(j * SLOT + oCA + 3, 3))
        ce = (air.pack(j * SLOT + oCE, 3), air.pack(j * SLOT + oCE + 3, 3))
        t1 = [e4[h] + sig1[h] + ch[h] + k_slot[j][h] + wj[h] for h in range(2)]
        air.constraint(an[0] + ca[0] * two32 - (t1[0] + sig0[0] + maj[0]))
        air.constraint(an[1] + ca[1] * two32 - (t1[1] + sig0[1] + maj[1] + ca[0]))
        air.constraint(en[0] + ce[0] * two32 - (a4[0] + t1[0]))
        air.constraint(en[1] + ce[1] * two32 - (a4[1] + t1[1] + ce[0]))
        # in rows q >= 1 the schedule word IS the recurrence's value (row 0 holds the message block)
        for h in range(2):
            air.constraint((1 - is_q0) * (wj[h] - L(j * SLOT + oSW + h)))

    # 3. the schedule recurrence, written on the current (= next) row with the previous row behind it:
    #    SW_t + 2^64 cw = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16], in halves
    for j in range(SLOTS):
        w2, w15 = w_bits_cur(j - 2), w_bits_cur(j - 15)
        s0 = halves_of([air.xor3(w15[(i + 1) % 64], w15[(i + 8) % 64], w15[i + 7] if i + 7 < 64 else 0) for i in range(64)])
        s1 = halves_of([air.xor3(w2[(i + 19) % 64], w2[(i + 61) % 64], w2[i + 6] if i + 6 < 64 else 0) for i in range(64)])
        w7, w16 = w_word_cur(j - 7), w_word_cur(j - 16)
        cw = (air.pack(j * SLOT + oCW, 2, next_row=True), air.pack(j * SLOT + oCW + 2, 2, next_row=True))
        air.constraint(N(j * SLOT + oSW) + cw[0] * two32 - (s1[0] + w7[0] + s0[0] + w16[0]))
        air.constraint(N(j * SLOT + oSW + 1) + cw[1] * two32 - (s1[1] + w7[1] + s0[1] + w16[1] + cw[0]))

    # 4. row to row inside a block: the next row starts from this row's last four rounds and HIN is carried along;
    # 5. block boundary (this row is the last of its block): the next block starts from IV or from HIN + final state;
    # 6. the first row starts a message; 7. the last row's output chaining value is the public digest.
    # Written word by word so that each word's packed halves are used while they are in registers.
    nb = 1 - is_q3
    air.constraint_first_row(L(IS_FIRST) - 1)
    out_halves = []                                             # the block's output chaining value, (low, high) per word
    for k in range(8):
        base_out = a_base(SLOTS - 1 - k) if k < 4 else e_base(SLOTS - 1 - (k - 4))
        base_start = a_base(-k - 1) if k < 4 else e_base(-(k - 4) - 1)
        out, nxt, cur = word(base_out), word(base_start, True), word(base_start)
        lo = L(HIN + 2 * k) + out[0] - L(CY + 2 * k) * two32
        hi = L(HIN + 2 * k + 1) + out[1] + L(CY + 2 * k) - L(CY + 2 * k + 1) * two32
        out_halves += [lo, hi]
        for h, ho in enumerate((lo, hi)):
            iv = _halves(IV[k])[h]
            air.constraint(nb * (nxt[h] - out[h]))
            air.constraint(nb * (N(HIN + 2 * k + h) - L(HIN + 2 * k + h)))
            air.constraint(is_q3 * (nxt[h] - ho - N(IS_FIRST) * (iv - ho)))
            air.constraint(is_q3 * (N(HIN + 2 * k + h) - nxt[h]))
            air.constraint_first_row(cur[h] - iv)
            air.constraint_last_row(ho - air.public(2 * k + h))

    # 8. binding (as in sha256_air.py): a challenge gamma in F_p^2 and a round-1 accumulator fold every block's
    # (message-start flag, 16 message words as (low, high) halves) - on its first row - and 8 output chaining words as
    # halves - on its last row - into one Horner fingerprint; the total is a round value of the proof.
    def ext_mul(x, y):
        return x[0] * y[0] + x[1] * y[1] * 7, x[0] * y[1] + x[1] * y[0]
    gamma = (air.challenge(0), air.challenge(1))

    def horner(start, elems):
        c0, c1 = start
        for e in elems:
            c0, c1 = ext_mul((c0, c1), gamma)
            c0 = c0 + e
        return c0, c1
    acc = (L(ACC), L(ACC + 1))
    msg = [L(IS_FIRST)]
    for j in range(16):
        msg += list(word(j * SLOT + oW))
    after_head, after_tail = horner(acc, msg), horner(acc, out_halves)      # 33 elements on rows q = 0, 16 on rows q = 3
    for c in range(2):
        air.constraint_first_row(acc[c])
        air.constraint_transition(N(ACC + c) - (acc[c] + is_q0 * (after_head[c] - acc[c]) + is_q3 * (after_tail[c] - acc[c])))
        air.constraint_last_row(after_tail[c] - air.round_value(1, c))
    return air


# ---------------------------------------------------------------------------------------------
# host helpers (_sha2.py): padding, a plain-Python trace generator (tests only; the product path generates the trace on
# the GPU with nlx_sha512_trace), the binding fingerprint.  Blocks are uint64 [n_blocks, 16]; digest_halves turns the eight
# digest words into the sixteen public inputs (low, high per word).
# ---------------------------------------------------------------------------------------------
pad_message, blocks_for_messages, digest_halves = _H.pad_message, _H.blocks_for_messages, _H.digest_halves
reference_trace, block_outputs = _H.reference_trace, _H.block_outputs
fingerprint, binding_columns, cpu_rounds = _H.fingerprint, _H.binding_columns, _H.cpu_rounds


class Sha512Prover(Sha2Prover):
    """Sha2Prover for SHA-512: nlx_sha512_trace, nlx_sha512_bind_round and the AIR above."""
    sha2, build_air = _H, staticmethod(sha512_air)
    trace_fn, bind_fn = "nlx_sha512_trace", "nlx_sha512_bind_round"
