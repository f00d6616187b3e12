// What the plonky2 prover (prover.hip) and the STARK prover (stark.hip) share on the host: the stage clock, the opening-point
// power table and the batch provers' job pool.
#pragma once
#include <atomic>
#include <system_error>
#include <thread>
#include <vector>
#include "ctx.hpp"
#include "gl.hpp"

namespace nlx {

// Stage timing of one proof: an event at the start of every stage and one at the end of the last.  Lives in the circuit / STARK
// handle (the events are made once, at build).  A clock without events - a local one of a stage-level call - records nothing.
struct StageClock {
    hipEvent_t ev[NLX_MAX_STAGES + 1]{};
    const char* names[NLX_MAX_STAGES]{};
    uint32_t n = 0;
    bool timed = false;
    hipStream_t stream = nullptr;
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int32_t create(nlx_ctx* ctx) {
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return ctx->fail(NLX_E_HIP, "hipEventCreate failed");
        return NLX_OK;
    }
    void begin(hipStream_t st) { n = 0; timed = false; stream = st; }
    void stage(const char* name) {
        if (n < NLX_MAX_STAGES && ev[n]) {
            (void)hipEventRecord(ev[n], stream);
            names[n++] = name;
        }
    }
    void end() {
        stage("end");
        n--;   // "end" only closes the last interval
        timed = true;
    }
    int32_t times(uint32_t* n_stages, const char** names_out, float* ms_out) const {
        if (!n_stages) return NLX_E_INVAL;
        *n_stages = timed ? n : 0;
        for (uint32_t i = 0; i < *n_stages; i++) {
            if (names_out) names_out[i] = names[i];
            if (ms_out && hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]) != hipSuccess) ms_out[i] = -1.f;
        }
        return NLX_OK;
    }
};

// zeta, g zeta and their powers zeta^(2^k), (g zeta)^(2^k), k < log_n, computed on the host (zeta is known there) so that the
// evaluation kernels start at once.  `host` is the SOURCE of an asynchronous copy: the object is a member of what owns the
// call's Scratch and is declared before it, so it is still there when the stream is drained.
struct OpeningPoints {
    uint64_t host[4 + 2 * 2 * 32];
    const uint64_t* d = nullptr;
    const uint64_t* zeta() const { return d; }
    const uint64_t* gzeta() const { return d + 2; }
    const uint64_t* zeta_pows() const { return d + 4; }
    const uint64_t* gzeta_pows() const { return d + 4 + 64; }
    int32_t upload(Scratch& scratch, const uint64_t z[2], const uint64_t gz[2], unsigned log_n) {
        uint64_t* dev = scratch.alloc_as<uint64_t>(2048);
        if (!dev) return NLX_E_NOMEM;
        host[0] = z[0]; host[1] = z[1]; host[2] = gz[0]; host[3] = gz[1];
        gl::Ext za{z[0], z[1]}, zb{gz[0], gz[1]};
        for (unsigned k = 0; k < 32; k++) {
            host[4 + 2 * k] = za.a; host[4 + 2 * k + 1] = za.b;
            host[4 + 64 + 2 * k] = zb.a; host[4 + 64 + 2 * k + 1] = zb.b;
            if (k + 1 < log_n) { za = gl::mul(za, za); zb = gl::mul(zb, zb); }
        }
        NLX_HIP(scratch.ctx, hipMemcpyAsync(dev, host, sizeof host, hipMemcpyHostToDevice, scratch.ctx->stream));
        d = dev;
        return NLX_OK;
    }
};

// nlx_batch_prove / nlx_stark_batch_prove: n_jobs proofs over n_workers handles of distinct contexts, a host thread per worker;
// prove(handle, job) sets the job's status.  Returns the first failed job's status.
// A std::thread that is still joinable when it is destroyed calls std::terminate: if creating worker w fails (std::system_error:
// no more threads), the workers already started are left to drain the queue and are JOINED before anything leaves this function;
// if none started, the calling thread does the work.  The jobs proved keep their status.
// Test hook batch_spawn_fault_after (armed by nlx_abi_selftest kind 3 / 4, ctx.hip): pretend that starting worker thread
// number >= this fails; -1 = off.
template <class Handle, class Prove>
int32_t batch_prove(const char* who, Handle* const* workers, uint32_t n_workers, nlx_prove_job* jobs, size_t n_jobs, Prove prove) {
    if (!workers || n_workers == 0 || (!jobs && n_jobs)) return NLX_E_INVAL;
    for (uint32_t w = 0; w < n_workers; w++) {
        if (!workers[w]) return NLX_E_INVAL;
        for (uint32_t v = 0; v < w; v++)
            if (workers[v]->ctx == workers[w]->ctx) return workers[w]->ctx->fail(NLX_E_INVAL, "%s: workers must use distinct contexts", who);
    }
    std::atomic<size_t> next{0};
    auto run = [&](Handle* h) {
        (void)hipSetDevice(h->ctx->device);
        for (;;) {
            const size_t j = next.fetch_add(1);
            if (j >= n_jobs) return;
            jobs[j].proof_len = 0;
            jobs[j].status = prove(h, jobs[j]);
        }
    };
    if (n_workers == 1) {
        run(workers[0]);
    } else {
        std::vector<std::thread> threads;
        threads.reserve(n_workers);
        bool spawn_failed = false;
        for (uint32_t w = 0; w < n_workers; w++) {
            try {
                if (batch_spawn_fault_after >= 0 && (int)w >= batch_spawn_fault_after) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
                threads.emplace_back(run, workers[w]);
            } catch (...) {
                spawn_failed = true;
                break;
            }
        }
        if (spawn_failed && threads.empty()) run(workers[0]);
        for (auto& t : threads) t.join();
        if (spawn_failed) workers[0]->ctx->fail(NLX_OK, "%s: could not start every worker thread; the jobs were proved by the ones that started", who);
    }
    for (size_t j = 0; j < n_jobs; j++)
        if (jobs[j].status != NLX_OK) return jobs[j].status;
    return NLX_OK;
}

}  // namespace nlx
