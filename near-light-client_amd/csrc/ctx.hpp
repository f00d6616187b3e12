// Per-device context: stream, caching device allocator, twiddle / coset tables, error slot.
// One context per HIP device and per host thread (SURVEY.md §8b threading contract).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <vector>
#include "../../include/nlx.h"
#include "launch.hpp"

struct nlx_ctx {
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // stream in use (own_stream or a borrowed one)
    std::string err;

    // caching allocator: freed blocks are kept by size and reused (hipMalloc/hipFree synchronise)
    std::multimap<size_t, void*> free_blocks;
    std::map<void*, size_t> live_blocks;
    size_t bytes_reserved = 0;

    // twiddle tables, built lazily up to the largest transform seen
    nlx::NttTables tables{};
    std::vector<void*> table_allocs;
    // coset scale tables keyed by (log_n << 8 | rate_bits)
    std::map<uint32_t, uint64_t*> coset_scale;
    // shift^i (natural order) tables for nlx_ntt_batch keyed by (log_n, shift)
    std::map<std::pair<uint32_t, uint64_t>, uint64_t*> nat_scale;
    std::vector<std::pair<uint32_t, uint64_t>> nat_scale_order;   // oldest first: at most four tables are kept
    // BN254 Fr twiddle table (csrc/bn254.hip) keyed by 2 log_n + inverse: w_n^e for e < n/2
    std::map<uint32_t, void*> bn254_tables;

    // Optional per-kernel device timing (HIP events on `stream` around selected launches); used by
    // bench.py to report the dominant kernel's average duration from inside the timed region.
    struct KernelSample { const char* name; double alg_bytes; double units; hipEvent_t e0, e1; };
    bool kernel_timing = false;
    std::vector<KernelSample> samples;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t get_event();
    void begin_kernel(const char* name, double alg_bytes, double units = 0.0);  // units: work items other than bytes (Poseidon permutations)
    void end_kernel();

    // PoseidonBN128 Merkle levels (and FRI leaf layers) of at most this many parents run the lane-split kernels
    // (poseidon_bn128.hip); set at creation: NLX_PBN_QUAD_MAX_PARENTS overrides PBN_QUAD_MAX_PARENTS_DEFAULT, 0 = never
    size_t pbn_quad_max_parents = 0;

    // pinned staging buffer for small device->host reads
    void* pinned = nullptr;
    size_t pinned_bytes = 0;

    int32_t fail(int32_t code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    int32_t hip_fail(hipError_t e, const char* what) {
        return fail(e == hipErrorOutOfMemory ? NLX_E_NOMEM : NLX_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }

    void* alloc(size_t bytes);
    void release(void* p);
    void trim();
    int32_t ensure_tables(unsigned log_n);
    int32_t get_coset_scale(unsigned log_n, unsigned rate_bits, const uint64_t** out, bool inverse = false);
    int32_t get_nat_scale(unsigned log_n, uint64_t shift, const uint64_t** out);

};

// ---- the ABI never throws or aborts (include/nlx.h, SURVEY.md §8b: Rust / Go callers map return codes to their own errors) ----
// Host code behind the entry points uses std::vector / map / string / thread; every extern "C" definition is therefore a
// function-try-block:   int32_t nlx_foo(nlx_ctx* ctx, ...) NLX_TRY { ... } NLX_CATCH(ctx)
// std::bad_alloc -> NLX_E_NOMEM, anything else -> NLX_E_INVAL, with nlx_last_error set when the call has a context.
namespace nlx {
// T of the lane-split dispatch (nlx_ctx::pbn_quad_max_parents).  Measured on MI355X (tools/bench_prove_bn128.py, "levels" of
// profiles/bn128_prove_bench.json; both kernels interleaved in one process, median of 5): k_pbn_merkle_level_quad takes 158 us
// up to 2^8 parents, 181 us at 2^14 and 303 us at 2^15, k_pbn_merkle_level 368 - 379 us from 2^6 to 2^15 (spread within a size
// below 3 % there); at 2^16 the lane-split kernel is the slower one (560 against 396 us).  2^15 is the largest size at which it
// wins (1.24x; an earlier run of the same table gave 319 against 396 us there, and 613 against 431 us at 2^16).
constexpr size_t PBN_QUAD_MAX_PARENTS_DEFAULT = (size_t)1 << 15;
extern std::atomic<int> batch_spawn_fault_after;   // ctx.hip
inline void on_exception(nlx_ctx* ctx, const char* what) noexcept {
    if (!ctx) return;
    try {
        ctx->err = what;
    } catch (...) {
    }
}
}  // namespace nlx
#define NLX_TRY try
#define NLX_CATCH_BODY(ctx, ret_nomem, ret_other)                                                          \
    catch (const std::bad_alloc&) {                                                                       \
        nlx::on_exception(ctx, "out of host memory (std::bad_alloc)");                                     \
        return ret_nomem;                                                                                 \
    }                                                                                                     \
    catch (const std::exception& e__) {                                                                   \
        nlx::on_exception(ctx, e__.what());                                                               \
        return ret_other;                                                                                 \
    }                                                                                                     \
    catch (...) {                                                                                         \
        nlx::on_exception(ctx, "unknown C++ exception");                                                  \
        return ret_other;                                                                                 \
    }
#define NLX_CATCH(ctx) NLX_CATCH_BODY(ctx, NLX_E_NOMEM, NLX_E_INVAL)
#define NLX_CATCH_VOID(ctx) NLX_CATCH_BODY(ctx, , )
#define NLX_CATCH_VALUE(ctx, v) NLX_CATCH_BODY(ctx, v, v)

#define NLX_HIP(ctx, call)                                   \
    do {                                                     \
        hipError_t e__ = (call);                             \
        if (e__ != hipSuccess) return (ctx)->hip_fail(e__, #call); \
    } while (0)
// the same for a call that returns one of the library's own codes (the failing callee has set the error text)
#define NLX_RC(call)                     \
    do {                                 \
        const int32_t rc__ = (call);     \
        if (rc__) return rc__;           \
    } while (0)

namespace nlx {
bool is_device_ptr(const void* p);
// RAII device view of a caller buffer: device pointers are used in place, host pointers are
// staged through a context allocation (copied in on construction if `in`, out on finish()).
struct Staged {
    nlx_ctx* ctx;
    void* user;
    void* dev = nullptr;
    size_t bytes;
    bool owned = false;
    bool out;
    int32_t status = 0;
    Staged(nlx_ctx* c, const void* user_ptr, size_t nbytes, bool copy_in, bool copy_out);
    Staged(const Staged&) = delete;   // a copy would release the block twice
    Staged& operator=(const Staged&) = delete;
    ~Staged();
    int32_t finish();  // enqueue copy-out (if any); caller synchronises
    template <class T> T* as() { return reinterpret_cast<T*>(dev); }
};
// RAII device scratch of one call: blocks of the context's allocator that go back to it when the call returns, by whichever
// path - after the stream has been synchronised, so that nothing queued still works on them and no host local that a queued
// copy reads has left scope.
struct Scratch {
    nlx_ctx* ctx;
    std::vector<void*> blocks;
    explicit Scratch(nlx_ctx* c) : ctx(c) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { if (!blocks.empty()) (void)drain(); }   // nothing handed out: nothing to wait for
    void* alloc(size_t bytes);   // nullptr: out of device memory
    template <class T> T* alloc_as(size_t bytes) { return reinterpret_cast<T*>(alloc(bytes)); }
    hipError_t drain();          // synchronise the stream and give the blocks back now; the synchronise's status
    // The tail every call shares: drain(), then hipGetLastError().  `rc` is what the call's body returned; the first failure wins,
    // then the synchronise's, then a kernel launch's.
    int32_t finish(int32_t rc);
};
}  // namespace nlx
