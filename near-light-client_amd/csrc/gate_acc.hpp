// The lazily reduced constraint accumulator of the quotient kernels (k_quotient, k_quotient_poseidon, k_fri_combine:
// prover_kernels.hip) and of the generated AIR kernels (csrc/airgen/, through air_vm.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gl.hpp"

namespace nlx {

// Running sums S_c = sum_k alpha_c^k * constraint_k of the gate being evaluated, for both challenges, with
// LAZY reduction: each 64x64 product is accumulated as four 32x32 partial products into four 64-bit columns
// (+ a carry counter each) - two instructions per partial product - and the 160-bit total is reduced once per
// gate.  A reduced multiply-add costs ~30 instructions; this costs 8 per challenge.
struct GateAcc {
    const uint64_t* __restrict__ ap0;  // alpha_0^(T0 + k), wave-uniform
    const uint64_t* __restrict__ ap1;
    uint64_t a[8];
    uint32_t kc[8];
    uint32_t k;
    uint64_t base[2];   // what stash() folded away so far (canonical)
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int i = 0; i < 8; i++) { a[i] = 0; kc[i] = 0; }
        k = 0;
        base[0] = base[1] = 0;
    }
    // the 24 registers of the columns -> two canonical sums (PoseidonGate's fused partial rounds need the registers for the
    // matrix pass between two groups of constraints); the constraint counter keeps running
    __device__ __forceinline__ void stash() {
        base[0] = gl::add(base[0], fold_columns(a, kc));
        base[1] = gl::add(base[1], fold_columns(a + 4, kc + 4));
#pragma unroll
        for (int i = 0; i < 8; i++) { a[i] = 0; kc[i] = 0; }
    }
    __device__ __forceinline__ void emit_at(uint32_t idx, uint64_t c) { mac(c, ap0[idx], ap1[idx]); }
    // sums 0 and 1 += c * b0, c * b1 (b0, b1 wave-uniform)
    __device__ __forceinline__ void mac(uint64_t c, uint64_t b0, uint64_t b1) {
        const uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32);
        asm("v_mad_u64_u32 %[a0], vcc, %[c0], %[p0], %[a0]\n\t"
            "v_addc_co_u32 %[k0], vcc, 0, %[k0], vcc\n\t"
            "v_mad_u64_u32 %[a1], vcc, %[c0], %[p1], %[a1]\n\t"
            "v_addc_co_u32 %[k1], vcc, 0, %[k1], vcc\n\t"
            "v_mad_u64_u32 %[a2], vcc, %[c1], %[p0], %[a2]\n\t"
            "v_addc_co_u32 %[k2], vcc, 0, %[k2], vcc\n\t"
            "v_mad_u64_u32 %[a3], vcc, %[c1], %[p1], %[a3]\n\t"
            "v_addc_co_u32 %[k3], vcc, 0, %[k3], vcc\n\t"
            "v_mad_u64_u32 %[a4], vcc, %[c0], %[q0], %[a4]\n\t"
            "v_addc_co_u32 %[k4], vcc, 0, %[k4], vcc\n\t"
            "v_mad_u64_u32 %[a5], vcc, %[c0], %[q1], %[a5]\n\t"
            "v_addc_co_u32 %[k5], vcc, 0, %[k5], vcc\n\t"
            "v_mad_u64_u32 %[a6], vcc, %[c1], %[q0], %[a6]\n\t"
            "v_addc_co_u32 %[k6], vcc, 0, %[k6], vcc\n\t"
            "v_mad_u64_u32 %[a7], vcc, %[c1], %[q1], %[a7]\n\t"
            "v_addc_co_u32 %[k7], vcc, 0, %[k7], vcc"
            : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [a4] "+v"(a[4]), [a5] "+v"(a[5]),
              [a6] "+v"(a[6]), [a7] "+v"(a[7]), [k0] "+v"(kc[0]), [k1] "+v"(kc[1]), [k2] "+v"(kc[2]), [k3] "+v"(kc[3]),
              [k4] "+v"(kc[4]), [k5] "+v"(kc[5]), [k6] "+v"(kc[6]), [k7] "+v"(kc[7])
            : [c0] "v"(c0), [c1] "v"(c1), [p0] "s"((uint32_t)b0), [p1] "s"((uint32_t)(b0 >> 32)), [q0] "s"((uint32_t)b1),
              [q1] "s"((uint32_t)(b1 >> 32))
            : "vcc");
    }
    __device__ __forceinline__ void emit(uint64_t c) { emit_at(k++, c); }
    // sum for challenge ch: A0 + (A1 + A2) 2^32 + A3 2^64 + K0 2^64 + (K1 + K2) 2^96 + K3 2^128 (mod p)
    __device__ __forceinline__ uint64_t finish(int ch) const { return gl::add(fold_columns(a + 4 * ch, kc + 4 * ch), base[ch]); }
    // The four 64-bit columns and their carry counts as ONE 160-bit integer (t4 : t3 : t2 : t1 : t0), reduced with
    // 2^64 = 2^32 - 1, 2^96 = -1, 2^128 = -2^32: (t1:t0) + t2 EPS - t3 - t4 2^32.  ~35 instructions (the first version
    // reduced every column on its own: ~110, twice per item of k_quotient).
    static __device__ __forceinline__ uint64_t fold_columns(const uint64_t* A, const uint32_t* K) {
        uint32_t t1, t2, t3, t4, m0, m1, cm;
        asm("v_add_co_u32 %[m0], vcc, %[a1l], %[a2l]\n\t"
            "v_addc_co_u32 %[m1], vcc, %[a1h], %[a2h], vcc\n\t"
            "v_addc_co_u32 %[cm], vcc, 0, 0, vcc\n\t"
            "v_add_co_u32 %[t1], vcc, %[a0h], %[m0]\n\t"
            "v_addc_co_u32 %[t2], vcc, %[m1], %[a3l], vcc\n\t"
            "v_addc_co_u32 %[t3], vcc, %[cm], %[a3h], vcc\n\t"
            "v_addc_co_u32 %[t4], vcc, 0, %[k3], vcc\n\t"
            "v_add_co_u32 %[t2], vcc, %[t2], %[k0]\n\t"
            "v_addc_co_u32 %[t3], vcc, %[t3], %[k1], vcc\n\t"
            "v_addc_co_u32 %[t4], vcc, 0, %[t4], vcc\n\t"
            "v_add_co_u32 %[t3], vcc, %[t3], %[k2]\n\t"
            "v_addc_co_u32 %[t4], vcc, 0, %[t4], vcc"
            : [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [m0] "=&v"(m0), [m1] "=&v"(m1), [cm] "=&v"(cm)
            : [a0h] "v"((uint32_t)(A[0] >> 32)), [a1l] "v"((uint32_t)A[1]), [a1h] "v"((uint32_t)(A[1] >> 32)), [a2l] "v"((uint32_t)A[2]),
              [a2h] "v"((uint32_t)(A[2] >> 32)), [a3l] "v"((uint32_t)A[3]), [a3h] "v"((uint32_t)(A[3] >> 32)), [k0] "v"(K[0]),
              [k1] "v"(K[1]), [k2] "v"(K[2]), [k3] "v"(K[3])
            : "vcc");
        return gl::reduce160((uint32_t)A[0], t1, t2, t3, t4);
    }
};

}  // namespace nlx
