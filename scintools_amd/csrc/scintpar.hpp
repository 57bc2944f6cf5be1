// scintpar.hpp -- what the no-fit scintillation measurements read from the device (Dynspec.get_scint_params(method='nofit'),
// get_acf_tilt, cut_dyn: dynspec.py:2570-2648, 2358-2413, 3158-3271).  Included at the end of fft.hip, after scint_acf.
//
// The ACF [R][C] stays in HBM; the host arithmetic of the reference needs only
//   acf_cuts_kernel        the two half-cuts through the centre, acf[R/2:, C/2] and acf[R/2, C/2:]: a gather, the same bits;
//   dyn_moments_*          count, mean and population variance of the finite, non-zero pixels of dyn: two-stage sums in a fixed
//                          order (a thread's strided running sum, the wave butterfly, the four waves in order, the workgroups'
//                          partials in order), the variance from a second pass about the mean;
//   acf_row_peaks_kernel   per listed row the FIRST column of the row maximum (np.argmax) and the 7 samples around it;
//   segment_cut_kernel     the (fcuts + 1) x (tcuts + 1) segments of cut_dyn as one stack: a gather, the same bits.
// All of them are latency / launch bound: 256 threads, wave64 shuffles, no atomics (equal inputs give equal bits).
#pragma once
#include <math.h>

#include "common.hpp"

namespace scint {

constexpr int kParBlocks = 1024;       // most workgroups of a moments pass (= partials the finish kernels add)
constexpr int kPeakWindow = 7;         // acf[row, x - 3 : x + 4]

// out[0 .. R - R/2) = acf[R/2 + i][C/2], out[R - R/2 .. R - R/2 + C - C/2) = acf[R/2][C/2 + j]
__global__ void __launch_bounds__(256) acf_cuts_kernel(const double* acf, int64_t R, int64_t C, double* out) {
    const int64_t nfc = R - R / 2, ntc = C - C / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nfc) out[i] = acf[(R / 2 + i) * C + C / 2];
    else if (i < nfc + ntc) out[i] = acf[(R / 2) * C + C / 2 + (i - nfc)];
}

// the pixels the reference keeps: is_valid(dyn) * (dyn != 0)  (dynspec.py:2633)
__device__ inline bool moments_keep(double v) { return isfinite(v) && v != 0.0; }

// pass 1: partial[b] = sum of the kept pixels of workgroup b's stride, partial[kParBlocks + b] = their number
__global__ void __launch_bounds__(256) dyn_moments_sum_kernel(const double* x, int64_t n, double* partial) {
    __shared__ double red[4];
    double s = 0.0, c = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        if (moments_keep(v)) { s += v; c += 1.0; }
    }
    s = block_sum(s, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) { partial[blockIdx.x] = s; partial[kParBlocks + blockIdx.x] = c; }
}
// out[0] = count, out[1] = mean (NaN for an empty selection, as np.mean)
__global__ void __launch_bounds__(256) dyn_moments_mean_kernel(const double* partial, int nb, double* out) {
    __shared__ double red[4];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) { s += partial[i]; c += partial[kParBlocks + i]; }
    s = block_sum(s, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) { out[0] = c; out[1] = s / c; }
}
// pass 2: partial[b] = sum of (x - mean)^2 over the kept pixels
__global__ void __launch_bounds__(256) dyn_moments_dev_kernel(const double* x, int64_t n, const double* stats, double* partial) {
    __shared__ double red[4];
    const double mean = stats[1];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        if (moments_keep(v)) { const double d = v - mean; s += d * d; }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// out[2] = population variance (np.var, ddof = 0)
__global__ void __launch_bounds__(256) dyn_moments_var_kernel(const double* partial, int nb, double* out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[2] = s / out[0];
}

// (value, column) of a row maximum: the larger value wins, equal values resolve to the LOWER column (np.argmax's first occurrence)
__device__ inline void peak_take(double& v, int& c, double ov, int oc) {
    if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
}

// One workgroup per listed row.  col_out[k]: first column of the maximum of acf[rows[k], :]; win_out[k][0..6] =
// acf[rows[k], col - 3 : col + 4]; flag_out[k]: 0 ok, 1 the window would cross column 0 or C (win_out[k] is then zero: nothing
// outside the row is read), 2 rows[k] is no row of the ACF.  NaN never compares larger, so a NaN sample is never the maximum.
__global__ void __launch_bounds__(256) acf_row_peaks_kernel(const double* acf, int64_t R, int64_t C, const int32_t* rows,
                                                             int32_t* col_out, double* win_out, int32_t* flag_out) {
    __shared__ double red_v[4];
    __shared__ int red_c[4];
    const int k = blockIdx.x;
    const int64_t row = rows[k];
    if (row < 0 || row >= R) {                          // uniform over the workgroup
        if (threadIdx.x == 0) { col_out[k] = 0; flag_out[k] = 2; }
        if (threadIdx.x < kPeakWindow) win_out[(int64_t)k * kPeakWindow + threadIdx.x] = 0.0;
        return;
    }
    const double* a = acf + row * C;
    double v = -INFINITY;
    int c = 0x7fffffff;
    for (int64_t j = threadIdx.x; j < C; j += 256) {    // ascending columns: a strict > keeps the thread's first occurrence
        const double x = a[j];
        if (x > v) { v = x; c = (int)j; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oc = __shfl_xor(c, o, 64);
        peak_take(v, c, ov, oc);
    }
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_c[threadIdx.x >> 6] = c; }
    __syncthreads();
    v = red_v[0]; c = red_c[0];
    for (int w = 1; w < 4; ++w) peak_take(v, c, red_v[w], red_c[w]);
    if (c == 0x7fffffff) c = 0;                         // nothing above -inf: np.argmax of a constant row
    const bool inside = c - 3 >= 0 && (int64_t)c + 4 <= C;
    if (threadIdx.x == 0) { col_out[k] = c; flag_out[k] = inside ? 0 : 1; }
    if (threadIdx.x < kPeakWindow)
        win_out[(int64_t)k * kPeakWindow + threadIdx.x] = inside ? a[c - 3 + (int)threadIdx.x] : 0.0;
}

// out[(ii * ntseg + jj)][r][c] = dyn[ii * fnum + r][jj * tnum + c]  (dynspec.py:3201-3203)
__global__ void __launch_bounds__(256) segment_cut_kernel(const double* dyn, int64_t nt, int64_t fnum, int64_t tnum,
                                                           int64_t ntseg, int64_t total, double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t c = i % tnum, t = i / tnum;
    const int64_t r = t % fnum, s = t / fnum;
    const int64_t ii = s / ntseg, jj = s - ii * ntseg;
    out[i] = dyn[(ii * fnum + r) * nt + jj * tnum + c];
}

}  // namespace scint

extern "C" int32_t scint_acf_cuts(const double* acf, int64_t R, int64_t C, double* cuts_out, void* stream) {
    SCINT_REQUIRE(acf && cuts_out, "acf_cuts: null pointer");
    SCINT_REQUIRE(R >= 1 && C >= 1, "acf_cuts: bad shape");
    const int64_t n = (R - R / 2) + (C - C / 2);
    hipLaunchKernelGGL(scint::acf_cuts_kernel, dim3((unsigned)scint::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       acf, R, C, cuts_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_dyn_moments_workspace_bytes(size_t* bytes) {
    SCINT_REQUIRE(bytes != nullptr, "dyn_moments_workspace_bytes: null output");
    *bytes = sizeof(double) * 2 * scint::kParBlocks + 256;
    return SCINT_OK;
}

extern "C" int32_t scint_dyn_moments(const double* dyn, int64_t n, double* stats_out, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
    using namespace scint;
    SCINT_REQUIRE(dyn && stats_out && workspace, "dyn_moments: null pointer");
    SCINT_REQUIRE(n >= 1, "dyn_moments: bad size");
    size_t need = 0;
    scint_dyn_moments_workspace_bytes(&need);
    if (workspace_bytes < need) { set_error("scint: dyn_moments workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = (double*)workspace;
    const int blocks = (int)std::min<int64_t>(kParBlocks, std::max<int64_t>(1, ceil_div(n, 1024)));
    hipLaunchKernelGGL(dyn_moments_sum_kernel, dim3(blocks), dim3(256), 0, stream, dyn, n, partial);
    hipLaunchKernelGGL(dyn_moments_mean_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, stats_out);
    hipLaunchKernelGGL(dyn_moments_dev_kernel, dim3(blocks), dim3(256), 0, stream, dyn, n, stats_out, partial);
    hipLaunchKernelGGL(dyn_moments_var_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, stats_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_acf_row_peaks(const double* acf, int64_t R, int64_t C, const int32_t* rows, int64_t nrows,
                                       int32_t* col_out, double* win_out, int32_t* flag_out, void* stream) {
    SCINT_REQUIRE(acf && rows && col_out && win_out && flag_out, "acf_row_peaks: null pointer");
    SCINT_REQUIRE(R >= 1 && C >= 1 && C < ((int64_t)1 << 31), "acf_row_peaks: bad shape");
    SCINT_REQUIRE(nrows >= 1 && nrows < ((int64_t)1 << 31), "acf_row_peaks: bad number of rows");
    hipLaunchKernelGGL(scint::acf_row_peaks_kernel, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)stream, acf, R, C, rows,
                       col_out, win_out, flag_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_segment_cut(const double* dyn, int64_t nf, int64_t nt, int64_t fnum, int64_t tnum, int64_t nfseg,
                                     int64_t ntseg, double* segs_out, void* stream) {
    SCINT_REQUIRE(dyn && segs_out, "segment_cut: null pointer");
    SCINT_REQUIRE(nf >= 1 && nt >= 1 && fnum >= 1 && tnum >= 1 && nfseg >= 1 && ntseg >= 1, "segment_cut: bad shape");
    SCINT_REQUIRE(nfseg <= nf / fnum && ntseg <= nt / tnum, "segment_cut: the segments do not fit the dynamic spectrum");
    const int64_t total = nfseg * ntseg * fnum * tnum;          // <= nf * nt
    SCINT_REQUIRE(scint::ceil_div(total, 256) < ((int64_t)1 << 31), "segment_cut: too many pixels");
    hipLaunchKernelGGL(scint::segment_cut_kernel, dim3((unsigned)scint::ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       dyn, nt, fnum, tnum, ntseg, total, segs_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}
