// Crossover sweep for the sub-wave (quad) Poseidon kernels of csrc/hash_kernels.hip against the one-lane-per-state kernels:
// HIP-event times on an otherwise idle GPU, the figures behind MERKLE_WIDE_MAX_PARENTS, HASH_LEAVES_WIDE_MAX_ROWS and the FRI
// crossover in fri.hip.  The kernels are compiled into this program from the library's own source file; only the one-lane FRI
// leaf launcher comes from libnlx.so.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -I near-light-client_amd/csrc tools/poseidon_quad_sweep.hip \
//         -L near-light-client_amd -lnlx -Wl,-rpath,'$ORIGIN/../near-light-client_amd' -o tools/poseidon_quad_sweep
//   tools/poseidon_quad_sweep > profiles/<name>.txt
#include "hash_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

namespace nlx {
void launch_fri_leaves(hipStream_t st, const uint64_t* d_values, unsigned log_n, unsigned rate_bits, unsigned arity_bits, uint64_t* d_digests);
}

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static hipStream_t st;
static hipEvent_t e0, e1;

// median of `reps` event-timed runs after two warm-up runs, in microseconds
static double time_us(const std::function<void()>& f, int reps = 9) {
    f();
    f();
    std::vector<float> t(reps);
    for (int i = 0; i < reps; i++) {
        CK(hipEventRecord(e0, st));
        f();
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&t[i], e0, e1));
    }
    CK(hipGetLastError());
    std::sort(t.begin(), t.end());
    return 1000.0 * t[reps / 2];
}

__global__ void k_fill(uint64_t* p, size_t n) {   // canonical pseudo-random words
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    p[i] = x % 0xFFFFFFFF00000001ull;
}

int main() {
    using namespace nlx;
    CK(hipStreamCreate(&st));
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const size_t max_words = ((size_t)1955 << 15) + 4096;   // the largest leaf table; tree and FRI buffers are far smaller
    uint64_t *d_in, *d_dig;
    CK(hipMalloc(&d_in, max_words * 8));
    CK(hipMalloc(&d_dig, ((size_t)1 << 21) * 8 * 4));
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((max_words + 255) / 256)), dim3(256), 0, st, d_in, max_words);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((((size_t)1 << 23) + 255) / 256)), dim3(256), 0, st, d_dig, (size_t)1 << 23);
    CK(hipStreamSynchronize(st));

    // 1. a tree level of `parents` parents and everything above it (cap 2^4): the level with one lane per parent and the rest
    //    fused, against the level fused with the five above it - the choice launch_merkle_levels makes at that level
    printf("# tree tops: microseconds from a level of P parents down to a cap of 16 digests, n_trees trees per launch\n");
    printf("# %8s %7s %22s %22s\n", "parents", "n_trees", "one-lane level + fused", "fused from this level");
    for (uint32_t n_trees : {1u, 10u})
        for (unsigned lp = 10; lp <= 17; lp++) {
            const size_t children = (size_t)2 << lp, tree_words = children * 8;
            if (tree_words * n_trees > ((size_t)1 << 23)) continue;
            auto rest = [&](uint64_t* cur, size_t lvl) {   // fused launches down to the cap
                while (lvl > 16) {
                    unsigned K = 0;
                    while (K < MERKLE_FUSED_MAX_LEVELS && (lvl >> K) > 16) K++;
                    launch_merkle_fused(st, cur, lvl, K, n_trees, tree_words);
                    for (unsigned s = 0; s < K; s++) {
                        cur += lvl * 4;
                        lvl >>= 1;
                    }
                }
            };
            const double a = time_us([&] {
                hipLaunchKernelGGL(k_merkle_level, dim3((unsigned)(((children >> 1) + 255) / 256), n_trees), dim3(256), 0, st, d_dig,
                                   d_dig + children * 4, children >> 1, tree_words);
                rest(d_dig + children * 4, children >> 1);
            });
            const double b = time_us([&] { rest(d_dig, children); });
            printf("  %8zu %7u %22.1f %22.1f\n", children >> 1, n_trees, a, b);
        }

    // 2. leaves of short tables
    printf("# leaves: microseconds per launch, rate_bits 1\n");
    printf("# %8s %7s %14s %14s\n", "rows", "columns", "one lane/leaf", "quad/leaf");
    for (uint32_t cols : {135u, 512u, 1955u})
        for (unsigned lr = 10; lr <= 15; lr++) {
            const size_t rows = (size_t)1 << lr;
            const double a = time_us([&] {
                hipLaunchKernelGGL(k_hash_lde_leaves, dim3((unsigned)((rows + 255) / 256), 1), dim3(256), 0, st, d_in, rows, cols, lr - 1, 1u,
                                   d_dig, 0u, (size_t)0);
            });
            const double b = time_us([&] { launch_hash_lde_leaves_wide(st, d_in, rows, cols, lr - 1, 1, d_dig, 0, 0); });
            printf("  %8zu %7u %14.1f %14.1f\n", rows, cols, a, b);
        }

    // 3. FRI layer leaves (arity 16, rate_bits 3)
    printf("# FRI leaves: microseconds per launch, arity 16, rate_bits 3\n");
    printf("# %8s %14s %14s\n", "leaves", "one lane/leaf", "quad/leaf");
    for (unsigned ll = 8; ll <= 16; ll++) {
        const unsigned log_n = ll + 4 - 3;
        const double a = time_us([&] { launch_fri_leaves(st, d_in, log_n, 3, 4, d_dig); });
        const double b = time_us([&] { launch_fri_leaves_wide(st, d_in, log_n, 3, 4, d_dig); });
        printf("  %8zu %14.1f %14.1f\n", (size_t)1 << ll, a, b);
    }
    return 0;
}
