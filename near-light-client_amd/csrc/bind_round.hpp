// The binding round (round 1) of a statement AIR, host side: one driver for the SHA-256, SHA-512 and Ed25519 AIRs.
// A trace is a sequence of units (compression blocks, signature slots) of `rows_per_unit` rows; the accumulator column is the
// running Horner fingerprint in F_p^2 of `unit_elems` elements per unit.  Two launches, one lane per unit, with a host prefix
// between them: k_fp gives every unit's own fingerprint (from 0), the host turns those into every unit's start value
// (acc_(u+1) = acc_u gamma^unit_elems + fp_u - a few thousand extension multiplications), k_rows writes the column from there.
#pragma once
#include "ctx.hpp"
#include "gl.hpp"
#include "transcript.hpp"
#include <vector>

namespace nlx {

using BindFpKernel = void (*)(const uint64_t* trace, uint32_t n_units, gl::Ext gamma, gl::Ext* unit_fp);
using BindRowsKernel = void (*)(const uint64_t* trace, uint32_t n_units, gl::Ext gamma, const gl::Ext* start, uint64_t* out);

// the caller has checked its arguments; gamma's words may be any 64-bit values
inline int32_t bind_round(nlx_ctx* ctx, const uint64_t* trace, uint32_t n_units, size_t rows_per_unit, size_t trace_cols,
                          uint32_t unit_elems, const uint64_t gamma[2], uint64_t* acc_out, uint64_t total_out[2],
                          BindFpKernel k_fp, BindRowsKernel k_rows) {
    (void)hipSetDevice(ctx->device);
    const size_t n = (size_t)n_units * rows_per_unit;
    Staged tr(ctx, trace, trace_cols * n * 8, true, false);
    if (tr.status) return tr.status;
    Staged so(ctx, acc_out, 2 * n * 8, false, true);
    if (so.status) return so.status;
    std::vector<gl::Ext> fp_h(n_units), start(n_units);   // `start` becomes the source of a queued copy: it outlives the scratch
    Scratch scratch(ctx);
    gl::Ext* d_fp = scratch.alloc_as<gl::Ext>((size_t)n_units * sizeof(gl::Ext));
    if (!d_fp) return NLX_E_NOMEM;
    const gl::Ext g{gamma[0] % gl::P, gamma[1] % gl::P};
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_fp, dim3((n_units + 63) / 64), dim3(64), 0, st, tr.as<uint64_t>(), n_units, g, d_fp);
    int32_t rc = fetch(ctx, fp_h.data(), d_fp, (size_t)n_units * sizeof(gl::Ext));
    if (!rc) {
        const gl::Ext g_unit = gl::pow(g, unit_elems);
        gl::Ext acc{0, 0};
        for (uint32_t u = 0; u < n_units; u++) {
            start[u] = acc;
            acc = gl::add(gl::mul(acc, g_unit), fp_h[u]);
        }
        total_out[0] = acc.a;
        total_out[1] = acc.b;
        hipError_t e = hipMemcpyAsync(d_fp, start.data(), (size_t)n_units * sizeof(gl::Ext), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) rc = ctx->hip_fail(e, "hipMemcpyAsync");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_rows, dim3((n_units + 63) / 64), dim3(64), 0, st, tr.as<uint64_t>(), n_units, g, d_fp,
                           so.as<uint64_t>());
        rc = so.finish();
    }
    return scratch.finish(rc);
}

}  // namespace nlx
