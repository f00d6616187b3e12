// Trace generation and binding round for the two SHA-2 compression AIRs, written once over a traits type per hash.
// SHA-256 ("AIR evaluators + trace generation on GPU"; callers nearx/src/merkle.rs:43-50,
// nearx/src/variables.rs:71-72 via curta_sha256): layout near-light-client_amd/sha256_air.py, NLX_SHA256_COLS columns, sixteen
// rounds per row.  SHA-512 (the hash inside every Ed25519 verification nearx proves,
// curta_eddsa_verify_sigs_conditional at nearx/src/builder.rs:152): layout near-light-client_amd/sha512_air.py, NLX_SHA512_COLS
// columns, twenty rounds per row; a 64-bit word is committed as bits and added as two 32-bit halves chained by a carry.
// Four rows per block in both.
//
// Two kernels generate a trace.  k_sha2_chain: one lane per message start walks that message's blocks and records every
// block's input chaining value.  k_sha2_trace: one lane per trace row (below).
#include "bind_round.hpp"

namespace nlx {

namespace sha2 {
__constant__ static const uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
__constant__ static const uint32_t IV256[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                               0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
// FIPS 180-4 §4.2.3 / §5.3.5
__constant__ static const uint64_t K512[80] = {
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL,
    0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL,
    0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
    0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL,
    0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
    0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
    0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL,
    0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL, 0x06ca6351e003826fULL, 0x142929670a0e6e70ULL,
    0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
    0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
    0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL,
    0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
    0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL,
    0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL,
    0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL,
    0xca273eceea26619cULL, 0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL,
    0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
    0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL,
    0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};
__constant__ static const uint64_t IV512[8] = {
    0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
    0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};

// What tells the two hashes apart.  H: 32-bit halves per word; s0 / s1: two rotations and a shift; S0 / S1: three rotations.
struct Sha256 {
    using word = uint32_t;
    static constexpr int H = 1, ROUNDS = 64, SLOTS = 16;
    static constexpr uint32_t COLS = NLX_SHA256_COLS, MAX_LOG_BLOCKS = 20;
    static constexpr int s0[3] = {7, 18, 3}, s1[3] = {17, 19, 10}, S0[3] = {2, 13, 22}, S1[3] = {6, 11, 25};
    static __device__ __forceinline__ word k(int t) { return K256[t]; }
    static __device__ __forceinline__ word iv(int i) { return IV256[i]; }
};
struct Sha512 {
    using word = uint64_t;
    static constexpr int H = 2, ROUNDS = 80, SLOTS = 20;
    static constexpr uint32_t COLS = NLX_SHA512_COLS, MAX_LOG_BLOCKS = 18;
    static constexpr int s0[3] = {1, 8, 7}, s1[3] = {19, 61, 6}, S0[3] = {28, 34, 39}, S1[3] = {14, 18, 41};
    static __device__ __forceinline__ word k(int t) { return K512[t]; }
    static __device__ __forceinline__ word iv(int i) { return IV512[i]; }
};

template <class T> struct Ops {
    using W = typename T::word;
    static constexpr int BITS = 32 * T::H;
    template <int R> static __device__ __forceinline__ W rotr(W x) { return (x >> R) | (x << (BITS - R)); }
    template <int R> static __device__ __forceinline__ W shr(W x) { return x >> R; }
    static __device__ __forceinline__ W s0(W x) { return rotr<T::s0[0]>(x) ^ rotr<T::s0[1]>(x) ^ shr<T::s0[2]>(x); }
    static __device__ __forceinline__ W s1(W x) { return rotr<T::s1[0]>(x) ^ rotr<T::s1[1]>(x) ^ shr<T::s1[2]>(x); }
    static __device__ __forceinline__ W S0(W x) { return rotr<T::S0[0]>(x) ^ rotr<T::S0[1]>(x) ^ rotr<T::S0[2]>(x); }
    static __device__ __forceinline__ W S1(W x) { return rotr<T::S1[0]>(x) ^ rotr<T::S1[1]>(x) ^ rotr<T::S1[2]>(x); }
    // half h of a word, as the 64-bit term of a sum of 32-bit halves
    static __device__ __forceinline__ uint64_t half(W x, int h) { return (uint64_t)(x >> (32 * h)) & 0xFFFFFFFFull; }
    // the low 32 bits of half h's sum, back in their place in the word
    static __device__ __forceinline__ W place(uint64_t s, int h) { return (W)(uint32_t)s << (32 * h); }
};

// Column layout (sha256_air.py, sha512_air.py): SLOTS round slots of kSLOT columns, then the row's start state and block data.
// 105 / 1953 columns for SHA-256, 210 / 4745 for SHA-512.
template <class T> struct Cols {
    enum : uint32_t { BITS = 32 * T::H, oA = 0, oE = BITS, oW = 2 * BITS, oCA = 3 * BITS, oCE = oCA + 3 * T::H, oCW = oCE + 3 * T::H,
                      oSW = oCW + 2 * T::H, kSLOT = oSW + T::H, cPA = T::SLOTS * kSLOT, cPE = cPA + 4 * BITS, cHIN = cPE + 4 * BITS,
                      cCY = cHIN + 8 * T::H, cIS_FIRST = cCY + 8 * T::H };
};
static_assert(Cols<Sha256>::cIS_FIRST + 1 == NLX_SHA256_COLS, "column map");
static_assert(Cols<Sha512>::cIS_FIRST + 1 == NLX_SHA512_COLS, "column map");

// one block: h <- h + compress(h, m)
template <class T> __device__ void compress(typename T::word h[8], const typename T::word* __restrict__ m) {
    using W = typename T::word;
    using O = Ops<T>;
    W w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = m[i];
    W a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
    for (int r0 = 0; r0 < T::ROUNDS; r0 += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const W t1 = hh + O::S1(e) + ((e & f) ^ (~e & g)) + T::k(r0 + i) + w[i];
            const W t2 = O::S0(a) + ((a & b) ^ (a & c) ^ (b & c));
            w[i] = w[i] + O::s0(w[(i + 1) & 15]) + w[(i + 9) & 15] + O::s1(w[(i + 14) & 15]);
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
}  // namespace sha2

template <class T>
__global__ __launch_bounds__(64) void k_sha2_chain(const typename T::word* __restrict__ blocks, const uint8_t* __restrict__ is_first,
                                                   uint32_t n_blocks, typename T::word* __restrict__ hin) {
    const uint32_t b0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (b0 >= n_blocks || !(is_first[b0] || b0 == 0)) return;
    typename T::word h[8];
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = T::iv(k);
    for (uint32_t b = b0; b < n_blocks && (b == b0 || !is_first[b]); b++) {
#pragma unroll
        for (int k = 0; k < 8; k++) hin[(size_t)b * 8 + k] = h[k];
        sha2::compress<T>(h, blocks + (size_t)b * 16);
        if (b == n_blocks - 1) {  // output chaining value of the last block = digest of the last message
#pragma unroll
            for (int k = 0; k < 8; k++) hin[(size_t)n_blocks * 8 + k] = h[k];
        }
    }
}

// One lane per trace row (four rows per block, SLOTS rounds per row).  Every lane replays its block's rounds (a few hundred
// integer instructions, 4x redundant per block - noise next to the 15.6 KB / 38 KB it then writes) and emits its row; a
// wave's 64 lanes are 64 consecutive rows, so each of the 1 953 / 4 745 column stores is 512 contiguous bytes.
// Every addition is a sum of 32-bit halves in 64 bits, half by half with the carry of the half below: for H = 1 that is the
// plain 64-bit sum of 32-bit words, whose bits 32.. are the carry the AIR commits.
template <class T>
__global__ __launch_bounds__(256) void k_sha2_trace(const typename T::word* __restrict__ blocks, const uint8_t* __restrict__ is_first,
                                                    const typename T::word* __restrict__ hin, uint32_t n_blocks,
                                                    uint64_t* __restrict__ trace) {
    using W = typename T::word;
    using O = sha2::Ops<T>;
    using C = sha2::Cols<T>;
    constexpr int H = T::H, ROUNDS = T::ROUNDS, SLOTS = T::SLOTS, BITS = 32 * H;
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)n_blocks << 2;
    if (row >= n) return;
    const uint32_t blk = (uint32_t)(row >> 2), q = (uint32_t)(row & 3);
    const uint32_t prev = blk ? blk - 1 : n_blocks - 1;  // the schedule recurrence of row 0 looks back cyclically
    W w[16 + ROUNDS];  // w[16 + t] = W_t of this block; w[0..15] = the last sixteen W of the previous block
    {
        W wp[16];
#pragma unroll
        for (int i = 0; i < 16; i++) wp[i] = blocks[(size_t)prev * 16 + i];
#pragma unroll 1
        for (int t = 16; t < ROUNDS; t++) {
            const W v = wp[t & 15] + O::s0(wp[(t + 1) & 15]) + wp[(t + 9) & 15] + O::s1(wp[(t + 14) & 15]);
            wp[t & 15] = v;
        }
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = wp[(ROUNDS - 16 + i) & 15];
#pragma unroll
        for (int i = 0; i < 16; i++) w[16 + i] = blocks[(size_t)blk * 16 + i];
#pragma unroll 1
        for (int t = 16; t < ROUNDS; t++) w[16 + t] = w[t] + O::s0(w[t + 1]) + w[t + 9] + O::s1(w[t + 14]);
    }
    W h0[8];
#pragma unroll
    for (int k = 0; k < 8; k++) h0[k] = hin[(size_t)blk * 8 + k];
    // a[t + 4], e[t + 4] for t = -4..ROUNDS-1, with the carries of every round's two additions
    W a[ROUNDS + 4], e[ROUNDS + 4];
    uint8_t ca[ROUNDS], ce[ROUNDS];  // half h's carry in bits 4h..4h+3
    a[3] = h0[0]; a[2] = h0[1]; a[1] = h0[2]; a[0] = h0[3];
    e[3] = h0[4]; e[2] = h0[5]; e[1] = h0[6]; e[0] = h0[7];
#pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
        const W a1 = a[r + 3], a2 = a[r + 2], a3 = a[r + 1], a4 = a[r];
        const W e1 = e[r + 3], e2 = e[r + 2], e3 = e[r + 1], e4 = e[r];
        const W s1v = O::S1(e1), chv = (e1 & e2) ^ (~e1 & e3), kv = T::k(r), wv = w[16 + r];
        const W s0v = O::S0(a1), mjv = (a1 & a2) ^ (a1 & a3) ^ (a2 & a3);
        W an = 0, en = 0;
        uint64_t sa = 0, se = 0;
        uint32_t cab = 0, ceb = 0;
#pragma unroll
        for (int h = 0; h < H; h++) {
            const uint64_t t1 = O::half(e4, h) + O::half(s1v, h) + O::half(chv, h) + O::half(kv, h) + O::half(wv, h);
            sa = t1 + O::half(s0v, h) + O::half(mjv, h) + (sa >> 32);
            se = O::half(a4, h) + t1 + (se >> 32);
            an |= O::place(sa, h);
            en |= O::place(se, h);
            cab |= (uint32_t)(sa >> 32) << (4 * h);
            ceb |= (uint32_t)(se >> 32) << (4 * h);
        }
        a[r + 4] = an;
        e[r + 4] = en;
        ca[r] = (uint8_t)cab;
        ce[r] = (uint8_t)ceb;
    }
    auto put = [&](uint32_t col, uint64_t v) { trace[(size_t)col * n + row] = v; };
    auto put_bits = [&](uint32_t base, W v, int cnt) {
        for (int i = 0; i < cnt; i++) put(base + i, (v >> i) & 1u);
    };
#pragma unroll 1
    for (uint32_t j = 0; j < SLOTS; j++) {
        const uint32_t r = SLOTS * q + j, base = j * C::kSLOT;
        put_bits(base + C::oA, a[r + 4], BITS);
        put_bits(base + C::oE, e[r + 4], BITS);
        put_bits(base + C::oW, w[16 + r], BITS);
#pragma unroll
        for (int h = 0; h < H; h++) put_bits(base + C::oCA + 3 * h, (ca[r] >> (4 * h)) & 15u, 3);
#pragma unroll
        for (int h = 0; h < H; h++) put_bits(base + C::oCE + 3 * h, (ce[r] >> (4 * h)) & 15u, 3);
        // w[16 + r + k] is W_{r + k}, k >= -16 (k < 0 in row 0 reaches the previous block's last sixteen W)
        const W x1 = O::s1(w[16 + r - 2]), x2 = w[16 + r - 7], x3 = O::s0(w[16 + r - 15]), x4 = w[16 + r - 16];
        uint64_t sw[H];
#pragma unroll
        for (int h = 0; h < H; h++)
            sw[h] = O::half(x1, h) + O::half(x2, h) + O::half(x3, h) + O::half(x4, h) + (h ? sw[h - 1] >> 32 : 0);
#pragma unroll
        for (int h = 0; h < H; h++) put(base + C::oSW + h, sw[h] & 0xFFFFFFFFull);
#pragma unroll
        for (int h = 0; h < H; h++) put_bits(base + C::oCW + 2 * h, (W)(sw[h] >> 32), 2);
    }
#pragma unroll 1
    for (uint32_t k = 0; k < 4; k++) {
        put_bits(C::cPA + BITS * k, a[SLOTS * q + 3 - k], BITS);
        put_bits(C::cPE + BITS * k, e[SLOTS * q + 3 - k], BITS);
    }
    const W fin[8] = {a[ROUNDS + 3], a[ROUNDS + 2], a[ROUNDS + 1], a[ROUNDS], e[ROUNDS + 3], e[ROUNDS + 2], e[ROUNDS + 1], e[ROUNDS]};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint64_t cy[H];
#pragma unroll
        for (int h = 0; h < H; h++) {
            put(C::cHIN + H * k + h, O::half(h0[k], h));
            cy[h] = (O::half(h0[k], h) + O::half(fin[k], h) + (h ? cy[h - 1] : 0)) >> 32;
        }
#pragma unroll
        for (int h = 0; h < H; h++) put(C::cCY + H * k + h, q == 3 ? cy[h] : 0u);
    }
    put(C::cIS_FIRST, (q == 0 && (is_first[blk] || blk == 0)) ? 1u : 0u);
}

// ---- binding accumulator (round 1 of the AIR): Horner fingerprint in F_p^2 of every block's message-start flag, 16 message
// words and 8 output chaining words, each word as its H halves (low first), read back from the trace ----
__device__ __forceinline__ uint64_t packed_half(const uint64_t* __restrict__ trace, size_t n, size_t row, uint32_t base) {
    uint64_t v = 0;
#pragma unroll 8
    for (int i = 0; i < 32; i++) v |= trace[(size_t)(base + i) * n + row] << i;
    return v;
}
__device__ __forceinline__ gl::Ext absorb1(gl::Ext acc, gl::Ext gamma, uint64_t v) {
    acc = gl::mul(acc, gamma);
    acc.a = gl::add(acc.a, v);
    return acc;
}
// the 1 + 16 H + 8 H elements of block b, absorbed into acc: head from its first row, tail from its last
template <class T>
__device__ __forceinline__ gl::Ext absorb_head(gl::Ext acc, gl::Ext gamma, const uint64_t* __restrict__ trace, size_t n, size_t row0) {
    using C = sha2::Cols<T>;
    acc = absorb1(acc, gamma, trace[(size_t)C::cIS_FIRST * n + row0]);
    for (uint32_t j = 0; j < 16; j++) {
#pragma unroll
        for (int h = 0; h < T::H; h++) acc = absorb1(acc, gamma, packed_half(trace, n, row0, j * C::kSLOT + C::oW + 32 * h));
    }
    return acc;
}
template <class T>
__device__ __forceinline__ gl::Ext absorb_tail(gl::Ext acc, gl::Ext gamma, const uint64_t* __restrict__ trace, size_t n, size_t row3) {
    using C = sha2::Cols<T>;
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t base = (T::SLOTS - 1 - (k & 3)) * C::kSLOT + (k < 4 ? C::oA : C::oE);
        uint64_t s = 0;
#pragma unroll
        for (int h = 0; h < T::H; h++) {
            s = trace[(size_t)(C::cHIN + T::H * k + h) * n + row3] + packed_half(trace, n, row3, base + 32 * h) + (s >> 32);
            acc = absorb1(acc, gamma, s & 0xFFFFFFFFull);
        }
    }
    return acc;
}
template <class T>
__global__ __launch_bounds__(64) void k_sha2_bind_block(const uint64_t* __restrict__ trace, uint32_t n_blocks, gl::Ext gamma,
                                                        gl::Ext* __restrict__ block_fp) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const size_t n = (size_t)n_blocks << 2;
    gl::Ext acc = absorb_head<T>(gl::Ext{0, 0}, gamma, trace, n, (size_t)b * 4);
    block_fp[b] = absorb_tail<T>(acc, gamma, trace, n, (size_t)b * 4 + 3);
}
template <class T>
__global__ __launch_bounds__(64) void k_sha2_bind_rows(const uint64_t* __restrict__ trace, uint32_t n_blocks, gl::Ext gamma,
                                                       const gl::Ext* __restrict__ start, uint64_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const size_t n = (size_t)n_blocks << 2, row0 = (size_t)b * 4;
    const gl::Ext s0 = start[b], s1 = absorb_head<T>(s0, gamma, trace, n, row0);
    out[row0] = s0.a;
    out[n + row0] = s0.b;
    for (int q = 1; q < 4; q++) {  // rows 1..3 hold the value after the block's first row was absorbed
        out[row0 + q] = s1.a;
        out[n + row0 + q] = s1.b;
    }
}

template <class T>
static int32_t sha2_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_blocks, const uint64_t gamma[2], uint64_t* acc_out,
                               uint64_t total_out[2]) {
    if (!ctx) return NLX_E_INVAL;
    if (!trace || !gamma || !acc_out || !total_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_blocks > T::MAX_LOG_BLOCKS) return ctx->fail(NLX_E_RANGE, "log_blocks must be <= %u", T::MAX_LOG_BLOCKS);
    return bind_round(ctx, trace, 1u << log_blocks, 4, T::COLS, 1 + 24 * T::H, gamma, acc_out, total_out, k_sha2_bind_block<T>,
                      k_sha2_bind_rows<T>);
}

template <class T>
static int32_t sha2_trace(nlx_ctx* ctx, const typename T::word* blocks, const uint8_t* is_first, uint32_t log_blocks,
                          uint64_t* trace_out, uint64_t digest_out[8]) {
    using W = typename T::word;
    if (!ctx) return NLX_E_INVAL;
    if (!blocks || !is_first || !trace_out) return ctx->fail(NLX_E_INVAL, "NULL argument");
    if (log_blocks > T::MAX_LOG_BLOCKS) return ctx->fail(NLX_E_RANGE, "log_blocks must be <= %u", T::MAX_LOG_BLOCKS);
    (void)hipSetDevice(ctx->device);
    const uint32_t n_blocks = 1u << log_blocks;
    const size_t n = (size_t)n_blocks << 2;  // four rows per block
    Staged sb(ctx, blocks, (size_t)n_blocks * 16 * sizeof(W), true, false);
    if (sb.status) return sb.status;
    Staged sf(ctx, is_first, n_blocks, true, false);
    if (sf.status) return sf.status;
    Staged st(ctx, trace_out, (size_t)T::COLS * n * 8, false, true);
    if (st.status) return st.status;
    Scratch scratch(ctx);
    W* d_hin = scratch.alloc_as<W>((size_t)(n_blocks + 1) * 8 * sizeof(W));
    if (!d_hin) return NLX_E_NOMEM;
    hipLaunchKernelGGL(k_sha2_chain<T>, dim3((n_blocks + 63) / 64), dim3(64), 0, ctx->stream, sb.as<W>(), sf.as<uint8_t>(),
                       n_blocks, d_hin);
    hipLaunchKernelGGL(k_sha2_trace<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sb.as<W>(),
                       sf.as<uint8_t>(), d_hin, n_blocks, st.as<uint64_t>());
    int32_t rc = st.finish();
    if (!rc && digest_out) {
        W dg[8];
        rc = fetch(ctx, dg, d_hin + (size_t)n_blocks * 8, sizeof dg);
        for (int k = 0; !rc && k < 8; k++) digest_out[k] = dg[k];
    }
    return scratch.finish(rc);
}

}  // namespace nlx

using namespace nlx;

extern "C" int32_t nlx_sha256_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_blocks, const uint64_t gamma[2],
                                         uint64_t* acc_out, uint64_t total_out[2]) NLX_TRY {
    return sha2_bind_round<sha2::Sha256>(ctx, trace, log_blocks, gamma, acc_out, total_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_sha512_bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t log_blocks, const uint64_t gamma[2],
                                         uint64_t* acc_out, uint64_t total_out[2]) NLX_TRY {
    return sha2_bind_round<sha2::Sha512>(ctx, trace, log_blocks, gamma, acc_out, total_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_sha256_trace(nlx_ctx* ctx, const uint32_t* blocks, const uint8_t* is_first, uint32_t log_blocks,
                                    uint64_t* trace_out, uint64_t digest_out[8]) NLX_TRY {
    return sha2_trace<sha2::Sha256>(ctx, blocks, is_first, log_blocks, trace_out, digest_out);
} NLX_CATCH(ctx)

extern "C" int32_t nlx_sha512_trace(nlx_ctx* ctx, const uint64_t* blocks, const uint8_t* is_first, uint32_t log_blocks,
                                    uint64_t* trace_out, uint64_t digest_out[8]) NLX_TRY {
    return sha2_trace<sha2::Sha512>(ctx, blocks, is_first, log_blocks, trace_out, digest_out);
} NLX_CATCH(ctx)
