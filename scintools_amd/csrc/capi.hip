// capi.hip -- error plumbing and diagnostics of the C ABI (include/scint_hip.h).
#include <stdio.h>
#include <string.h>

#include "prof.hpp"

namespace scint {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int32_t hip_fail(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "scint: HIP error %d (%s) in `%s` at %s:%d", (int)e,
             hipGetErrorString(e), what, file, line);
    g_last_error = buf;
    return SCINT_E_HIP;
}

Profiler& profiler() {
    static Profiler p;
    return p;
}

}  // namespace scint

extern "C" int32_t scint_profile_begin(void) {
    scint::Profiler& p = scint::profiler();
    p.reset(nullptr);
    p.enabled = true;
    return SCINT_OK;
}

extern "C" int32_t scint_profile_end(double* ms_out, double* ms_sum_out, int64_t* launches_out, int32_t count) {
    scint::Profiler& p = scint::profiler();
    if (count < 0) { scint::set_error("scint: profile_end: negative count"); return SCINT_E_ARG; }
    if (hipDeviceSynchronize() != hipSuccess) return SCINT_E_HIP;
    p.collect();
    p.finish();
    p.enabled = false;
    for (int k = 0; k < scint::kProfCount && k < count; ++k) {       // never more than the caller's arrays hold
        if (ms_out) ms_out[k] = p.ms[k];
        if (ms_sum_out) ms_sum_out[k] = p.ms_sum[k];
        if (launches_out) launches_out[k] = p.launches[k];
    }
    return SCINT_OK;
}

extern "C" int32_t scint_version(void) { return SCINT_ABI_VERSION; }   // (its history: include/scint_hip.h)

extern "C" int32_t scint_last_error(char* buf, size_t n) {
    if (!buf || n == 0) return SCINT_E_ARG;
    strncpy(buf, scint::g_last_error.c_str(), n - 1);
    buf[n - 1] = '\0';
    return SCINT_OK;
}

extern "C" int32_t scint_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- the velocity and trapezoid rescalings of scale_dyn (kernels: scale.hpp, which switches floating-point contraction off) ----
#include "scale.hpp"

using namespace scint;

extern "C" int32_t scint_spline_resample_rows_workspace_bytes(int64_t nf, int64_t nt, int64_t block, int64_t warm, size_t* bytes) {
    SCINT_REQUIRE(bytes, "spline_resample_rows_workspace_bytes: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 4 && warm >= 0, "spline_resample_rows_workspace_bytes: need nf >= 1, nt >= 4, warm >= 0");
    int64_t blk; int rt, stride;
    spline_rows_tile(nt, block, warm, &blk, &rt, &stride);
    *bytes = rt > 0 ? 256 : sizeof(double) * (size_t)nf * (size_t)nt;
    return SCINT_OK;
}

extern "C" int32_t scint_spline_resample_rows(const double* dyn, int64_t nf, int64_t nt, const double* h, const double* sub,
                                              const double* inv, const double* sup, const double* end, int64_t block,
                                              int64_t warm, const int32_t* idx, const double* coef, int64_t nout, double* out,
                                              void* workspace, size_t workspace_bytes, void* stream_) {
    SCINT_REQUIRE(dyn && h && sub && inv && sup && end && idx && coef && out, "spline_resample_rows: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 4 && nout >= 1, "spline_resample_rows: need at least 4 knots");
    SCINT_REQUIRE(nf <= 65535 && nt < (int64_t(1) << 31) && nout < (int64_t(1) << 31),
                  "spline_resample_rows: too many rows or knots");
    SCINT_REQUIRE(warm >= 0, "spline_resample_rows: bad warm-up length");
    hipStream_t stream = (hipStream_t)stream_;
    RowSpline s{h, sub, inv, sup, end[0], end[1], end[2], end[3]};
    int64_t blk; int rt, stride;
    spline_rows_tile(nt, block, warm, &blk, &rt, &stride);
    if (blk == nt - 2) warm = 0;
    if (rt > 0) {
        const int64_t nblk = ceil_div(nt - 2, blk), ngrp = ceil_div(nf, rt);
        SCINT_REQUIRE(ngrp <= 65535, "spline_resample_rows: too many row groups");
        hipLaunchKernelGGL(spline_rows_kernel, dim3((unsigned)nblk, (unsigned)ngrp), dim3(kRowsThreads), 0, stream, dyn, nf, nt, s,
                           blk, warm, rt, stride, idx, coef, nout, out);
        SCINT_LAUNCH_CHECK();
        return SCINT_OK;
    }
    SCINT_REQUIRE(workspace, "spline_resample_rows: null workspace");
    if (workspace_bytes < sizeof(double) * (size_t)nf * (size_t)nt) {
        set_error("scint: spline_resample_rows workspace too small");
        return SCINT_E_WORKSPACE;
    }
    double* W = (double*)workspace;
    hipLaunchKernelGGL(spline_rows_seq_kernel, dim3((unsigned)ceil_div(nf, 64)), dim3(64), 0, stream, dyn, nf, nt, s, W);
    SCINT_LAUNCH_CHECK();
    hipLaunchKernelGGL(spline_rows_eval_kernel, dim3((unsigned)ceil_div(nout, 256), (unsigned)nf), dim3(256), 0, stream, dyn,
                       (const double*)W, nt, idx, coef, nout, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_trap_scale(const double* dyn, int64_t nf, int64_t nt, double mean, const double* cw, const double* sw,
                                    const double* times, const int32_t* nkeep, double* out, void* stream_) {
    SCINT_REQUIRE(dyn && times && nkeep && out, "trap_scale: null pointer");
    SCINT_REQUIRE((cw == nullptr) == (sw == nullptr), "trap_scale: pass both window tables or neither");
    SCINT_REQUIRE(nf >= 1 && nt >= 1 && nf <= 65535, "trap_scale: need 1 <= nf <= 65535, nt >= 1");
    hipLaunchKernelGGL(trap_scale_kernel, dim3((unsigned)ceil_div(nt, 256), (unsigned)nf), dim3(256), 0, (hipStream_t)stream_, dyn,
                       nf, nt, mean, cw, sw, times, nkeep, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}
