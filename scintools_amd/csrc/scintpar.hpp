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

// ---- batched 1-D ACF fits: scint_acf1d_fit (Dynspec.fit_scint_params, dynspec.py:2575-2608, 2650-2702; scint_models.py:62-120) ----
// One WAVEFRONT per problem, kFitWaves problems per workgroup.  A cropped cut holds a few tens of samples, so a 256-thread workgroup
// per problem would idle three waves out of four and pay two barriers per reduction; a wavefront reduces the 15 sums of a pass by
// butterflies alone, needs no LDS and no barrier, and the waves of a workgroup never wait for each other (their iteration counts
// differ).  Sample j of a cut belongs to lane j % 64 from the first read to the last pass: a lane only re-reads what it wrote itself.
// The butterfly leaves the same bits in every lane, so the 3 x 3 / 4 x 4 solve and every decision of the loop are wave-uniform.
// No atomics: the per-lane running sums ascend in j, the butterfly and the scan are fixed trees -- equal inputs give equal bits.
namespace scint {

constexpr int kFitWaves = 4;           // problems per workgroup
constexpr int kFitSetup = 6;           // a row of setup_out: wn, amp, tau, dnu (the start values), then the two crop lengths n_t, n_f
constexpr int kFitNone = 0x7fffffff;
// status_out
constexpr int kFitConverged = 0, kFitIterCap = 1, kFitSingular = 2, kFitNonFiniteInput = 3, kFitNonFiniteStep = 4;

__device__ inline int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}

// first j with y[j] < thr (np.argwhere(y < thr)[0]); kFitNone without one.  NaN never compares below.
__device__ inline int acf1d_first_below(const double* y, int n, double thr, int lane) {
    int first = kFitNone;
    for (int j = lane; j < n; j += 64)
        if (y[j] < thr) { first = j; break; }
    return wave_min_int(first);
}

// number of samples x_j = step * j <= lim: the crop of dynspec.py:2598-2603 (x ascends, so the kept samples are the first ones)
__device__ inline int acf1d_count_within(int n, double step, double lim, int lane) {
    int c = 0;
    for (int j = lane; j < n; j += 64) c += (step * (double)j <= lim) ? 1 : 0;
    return wave_sum_int(c);
}

// The weights of one cropped cut y[0 .. n) (dynspec.py:2669-2687; `len` is the ACF's length along the cut, the reference's nt or
// nf): 1 / sqrt(len / 2) without bartlett; with it the variance 1 / (len / 2) times 1 + 2 cumsum(y[1:-1]^2) from the third sample
// on -- an exclusive scan, 64 samples at a time (Hillis-Steele inside the wave, a running carry across the chunks).  Ones when not
// weighted.  The first weight is zero in every case (scint_models.py:81, :105).
__device__ inline void acf1d_weights(const double* y, double* w, int n, double len, int weighted, int bartlett, int lane) {
    const double var0 = 1.0 / (len / 2.0);
    double carry = 0.0;
    for (int base = 0; base < n; base += 64) {          // wave-uniform trip count: the shuffles see every lane
        const int j = base + lane;
        double out = 1.0;
        if (weighted && bartlett) {
            double v = (j >= 1 && j < n) ? y[j] * y[j] : 0.0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            const double below = __shfl_up(v, 1, 64);
            const double excl = lane > 0 ? carry + below : carry;      // sum of y[1 .. j - 1]^2
            carry += __shfl(v, 63, 64);
            const double var = j >= 2 ? var0 * (1.0 + 2.0 * excl) : var0;
            out = 1.0 / sqrt(var);
        } else if (weighted) {
            out = 1.0 / (1.0 / sqrt(len / 2.0));
        }
        if (j < n) w[j] = j == 0 ? 0.0 : out;
    }
}

template <int NV>
struct FitSums {
    double cost, g[NV], a[NV][NV];      // sum r^2, J^T r, J^T J (lower triangle) in (log tau, log dnu, log amp[, alpha])
};

// One pass over the residuals at p = (tau, dnu, amp, alpha):
//   r_t = (y_t - amp exp(-(x_t / tau)^alpha) (1 - x_t / max x_t)) w_t,   r_f = (y_f - amp exp(-x_f ln2 / dnu) (1 - x_f / max x_f)) w_f
// and their derivatives by log tau, log dnu, log amp and alpha.  Sample 0 has weight zero and is skipped (its (x / tau)^alpha has
// no derivative by alpha).  s exp(-s) is taken as 0 where exp(-s) has underflowed, so an overflowing s gives no inf * 0.
template <int NV>
__device__ inline void acf1d_pass(const double* yt, const double* wt, int nt, const double* yf, const double* wf, int nf,
                                  double dt, double df, const double* p, int lane, FitSums<NV>& s) {
    const double tau = p[0], dnu = p[1], amp = p[2], alpha = p[3];
    const double xt_max = dt * (double)(nt - 1), xf_max = df * (double)(nf - 1);
    double cost = 0.0, g[NV], a[NV][NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) a[i][k] = 0.0;
    }
    for (int j = lane; j < nt; j += 64) {
        if (j == 0) continue;
        const double x = dt * (double)j, w = wt[j];
        const double u = x / tau, sp = pow(u, alpha), e = exp(-sp), tri = 1.0 - x / xt_max;
        const double se = sp < 700.0 ? sp * e : 0.0;
        const double r = (yt[j] - amp * e * tri) * w;
        double J[NV];
        J[0] = -w * amp * tri * alpha * se;
        J[1] = 0.0;
        J[2] = -w * amp * tri * e;
        if (NV == 4) J[NV - 1] = w * amp * tri * se * log(u);
        cost += r * r;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            g[i] += J[i] * r;
#pragma unroll
            for (int k = 0; k <= i; ++k) a[i][k] += J[i] * J[k];
        }
    }
    for (int j = lane; j < nf; j += 64) {
        if (j == 0) continue;
        const double x = df * (double)j, w = wf[j];
        const double v = x * 0.6931471805599453 / dnu, e = exp(-v), tri = 1.0 - x / xf_max;
        const double ve = v < 700.0 ? v * e : 0.0;
        const double r = (yf[j] - amp * e * tri) * w;
        const double J1 = -w * amp * tri * ve, J2 = -w * amp * tri * e;
        cost += r * r;
        g[1] += J1 * r;
        g[2] += J2 * r;
        a[1][1] += J1 * J1;
        a[2][1] += J2 * J1;
        a[2][2] += J2 * J2;
    }
    s.cost = wave_sum(cost);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        s.g[i] = wave_sum(g[i]);
#pragma unroll
        for (int k = 0; k <= i; ++k) s.a[i][k] = wave_sum(a[i][k]);
    }
}

// In-place Cholesky factor (lower triangle) of a matrix with a unit-scale diagonal; false when a pivot is not above rounding
// (a NaN fails the comparison too).
template <int NV>
__device__ inline bool acf1d_chol(double (&c)[NV][NV]) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double d = c[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= c[j][k] * c[j][k];
        if (!(d > 1e-15)) return false;
        d = sqrt(d);
        c[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < NV; ++i) {
            double t = c[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= c[i][k] * c[j][k];
            c[i][j] = t / d;
        }
    }
    return true;
}
template <int NV>
__device__ inline void acf1d_chol_solve(const double (&c)[NV][NV], double (&b)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= c[i][k] * b[k];
        b[i] = t / c[i][i];
    }
#pragma unroll
    for (int i = NV - 1; i >= 0; --i) {
        double t = b[i];
#pragma unroll
        for (int k = i + 1; k < NV; ++k) t -= c[k][i] * b[k];
        b[i] = t / c[i][i];
    }
}

// The scaled normal matrix a_ik / (d_i d_k) with d = sqrt(diag a), its diagonal 1 + lambda (Marquardt's scaling), factored.
// false: a parameter without any influence (d_i = 0) or a matrix that is singular to rounding.
template <int NV>
__device__ inline bool acf1d_factor(const FitSums<NV>& s, double lambda, double (&d)[NV], double (&c)[NV][NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        d[i] = sqrt(s.a[i][i]);
        if (!(d[i] > 0.0) || !isfinite(d[i])) return false;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int k = 0; k < i; ++k) c[i][k] = c[k][i] = s.a[i][k] / (d[i] * d[k]);
        c[i][i] = 1.0 + lambda;
    }
    return acf1d_chol<NV>(c);
}

// NV = 3: alpha fixed; NV = 4: alpha varies.  ws: per problem 2 (n_tc + n_fc) doubles -- the two half-cuts, then their weights.
template <int NV>
__global__ void __launch_bounds__(64 * kFitWaves)
acf1d_fit_kernel(const double* acf, int64_t B, int64_t R, int64_t C, double dt, double df, const double* bw, const double* tobs,
                 double nscale, int full_frame, int weighted, int bartlett, double alpha0, int max_iter, double* values,
                 double* errors, double* stats, int32_t* niter_out, int32_t* status_out, double* setup, double* ws) {
#pragma clang fp contract(off)          // start values and crop decisions round as the host's (no fused multiply-add)
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kFitWaves + (threadIdx.x >> 6);
    if (b >= B) return;                 // the whole wavefront: nothing below is shared between waves
    const int ntc = (int)(C - C / 2), nfc = (int)(R - R / 2);
    const int64_t L = (int64_t)ntc + nfc;
    const double* a = acf + b * R * C;
    double* yt = ws + b * 2 * L;
    double* yf = yt + ntc;
    double* wt = yt + L;
    double* wf = wt + ntc;
    const double nan = __builtin_nan("");

    // 1. the two half-cuts, each element read once; the strided column lands contiguous in the workspace
    int bad = 0;
    double first_t = 0.0, first_f = 0.0;
    for (int j = lane; j < ntc; j += 64) {
        const double v = a[(R / 2) * C + C / 2 + j];
        yt[j] = v;
        if (j == lane) first_t = v;
        bad |= isfinite(v) ? 0 : 1;
    }
    for (int j = lane; j < nfc; j += 64) {
        const double v = a[(R / 2 + j) * C + C / 2];
        yf[j] = v;
        if (j == lane) first_f = v;
        bad |= isfinite(v) ? 0 : 1;
    }
    bad = wave_sum_int(bad);
    const double yt0 = __shfl(first_t, 0, 64), yt1 = __shfl(first_t, 1, 64);
    const double yf0 = __shfl(first_f, 0, 64), yf1 = __shfl(first_f, 1, 64);

    int status = kFitIterCap, niter = 0, nt = ntc, nf = nfc;
    double p[4] = {nan, nan, nan, alpha0}, wn = nan;
    double val[4] = {nan, nan, nan, nan}, err[4] = {nan, nan, nan, nan}, chisqr = nan, redchi = nan;
    if (bad) {
        status = kFitNonFiniteInput;
    } else {
        // 2. start values and crop, in the reference's order (dynspec.py:2583-2608)
        const double dyf = yf0 - yf1, dyt = yt0 - yt1;
        wn = dyt < dyf ? dyt : dyf;                                     // min([f, t])
        const double af = yf0 - wn, at = yt0 - wn;
        const double amp = at > af ? at : af;                           // max([f, t])
        const int it = acf1d_first_below(yt, ntc, amp / 2.718281828459045, lane);
        const int jf = acf1d_first_below(yf, nfc, amp / 2.0, lane);
        const double tau = it == kFitNone ? (yt1 < 0.0 ? dt : tobs[b]) : dt * (double)it;
        const double dnu = jf == kFitNone ? (yf1 < 0.0 ? df : bw[b]) : df * (double)jf;
        if (!full_frame) {
            const double lim_t = nscale * tau <= 5.0 * dt ? 5.0 * dt : nscale * tau;
            const double lim_f = nscale * dnu <= 5.0 * df ? 5.0 * df : nscale * dnu;
            nt = acf1d_count_within(ntc, dt, lim_t, lane);
            nf = acf1d_count_within(nfc, df, lim_f, lane);
        }
        p[0] = tau; p[1] = dnu; p[2] = amp;
        // 3. weights
        acf1d_weights(yt, wt, nt, (double)C, weighted, bartlett, lane);
        acf1d_weights(yf, wf, nf, (double)R, weighted, bartlett, lane);
    }
    if (lane == 0 && setup) {
        double* so = setup + b * kFitSetup;
        so[0] = wn; so[1] = p[2]; so[2] = p[0]; so[3] = p[1]; so[4] = (double)nt; so[5] = (double)nf;
    }

    // 4. Levenberg-Marquardt in (log tau, log dnu, log amp[, alpha]): at most max_iter passes over the residuals
    if (!bad) {
        FitSums<NV> cur, tri;
        double d[NV], c[NV][NV];
        bool ok = p[0] > 0.0 && p[1] > 0.0 && p[2] > 0.0 && isfinite(p[0]) && isfinite(p[1]) && nt >= 2 && nf >= 2;
        if (!ok) {
            status = kFitSingular;      // a scale at zero has no logarithm: the normal matrix has a zero row there
        } else {
            acf1d_pass<NV>(yt, wt, nt, yf, wf, nf, dt, df, p, lane, cur);
            if (!isfinite(cur.cost)) { status = kFitNonFiniteStep; ok = false; }
        }
        double lambda = 1e-3, nu = 2.0;
        while (ok && niter < max_iter) {
            ++niter;
            if (!acf1d_factor<NV>(cur, lambda, d, c)) { status = kFitSingular; ok = false; break; }
            double dq[NV], gs = 0.0, step = 0.0;
#pragma unroll
            for (int i = 0; i < NV; ++i) { dq[i] = -cur.g[i] / d[i]; gs += dq[i] * dq[i]; }
            acf1d_chol_solve<NV>(c, dq);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                dq[i] /= d[i];
                fin = fin && isfinite(dq[i]);
                dq[i] = dq[i] > 3.0 ? 3.0 : (dq[i] < -3.0 ? -3.0 : dq[i]);      // at most e^3 per pass in a scale, 3 in alpha
                step = fabs(dq[i]) > step ? fabs(dq[i]) : step;
            }
            if (!fin) { status = kFitNonFiniteStep; ok = false; break; }
            double q[4] = {p[0] * exp(dq[0]), p[1] * exp(dq[1]), p[2] * exp(dq[2]), p[3]};
            if (NV == 4) q[3] = p[3] + dq[NV - 1];
            acf1d_pass<NV>(yt, wt, nt, yf, wf, nf, dt, df, q, lane, tri);
            if (!isfinite(tri.cost)) { status = kFitNonFiniteStep; ok = false; break; }
            // Downhill: taken, and the damping follows the gain ratio rho = actual / predicted reduction (Nielsen's rule) -- a
            // large-residual problem, where the full Gauss-Newton step overshoots, settles at the damping that makes it contract.
            // Flat to rounding (the cost cannot tell two points within ~1e-8 of the optimum apart): taken when the scaled gradient
            // shrinks, with the damping left alone.  Uphill: dropped, more damping.
            double gs_new = 0.0, pred = 0.0;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                gs_new += tri.a[i][i] > 0.0 ? tri.g[i] * tri.g[i] / tri.a[i][i] : 0.0;
                pred -= 2.0 * cur.g[i] * dq[i];
#pragma unroll
                for (int k = 0; k < NV; ++k) pred -= dq[i] * (k <= i ? cur.a[i][k] : cur.a[k][i]) * dq[k];
            }
            const bool flat = fabs(tri.cost - cur.cost) <= 1e-13 * cur.cost;
            const bool accept = flat ? gs_new < gs : tri.cost < cur.cost;
            if (accept && !flat) {
                const double rho = pred > 0.0 ? (cur.cost - tri.cost) / pred : 1.0, t = 2.0 * rho - 1.0;
                const double f = 1.0 - t * t * t;
                lambda *= f > 1.0 / 3.0 ? f : 1.0 / 3.0;
                lambda = lambda > 1e-15 ? lambda : 1e-15;
                nu = 2.0;
            } else if (!accept) {
                lambda *= nu;
                nu *= 2.0;
            }
            if (accept) {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = q[i];
                cur = tri;
            }
            // converged: the step of this pass moved no scale by more than 1e-12 of itself (alpha: by 1e-12) -- taken if it
            // passed the test above, dropped if not: then nothing smaller can be told from rounding either
            if (step <= 1e-12) { status = kFitConverged; break; }
        }
        // 5. covariance in the external parameters at the optimum: (J^T J)^-1 chi^2 / (N - nvary)
        if (ok && status == kFitConverged) {
            if (!acf1d_factor<NV>(cur, 0.0, d, c)) {
                status = kFitSingular;
            } else {
                chisqr = cur.cost;
                redchi = chisqr / (double)(nt + nf - NV);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    double unit[NV];
#pragma unroll
                    for (int k = 0; k < NV; ++k) unit[k] = k == i ? 1.0 : 0.0;
                    acf1d_chol_solve<NV>(c, unit);
                    const double scale = (i < 3 ? p[i] : 1.0) / d[i];            // d p / d log p = p
                    err[i] = sqrt(unit[i] * redchi) * scale;
                    val[i] = p[i];
                }
                if (NV == 3) { val[3] = p[3]; err[3] = 0.0; }
            }
        }
        if (status != kFitConverged) {
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] = err[i] = nan;
            chisqr = redchi = nan;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { values[b * 4 + i] = val[i]; errors[b * 4 + i] = err[i]; }
        stats[b * 2] = chisqr;
        stats[b * 2 + 1] = redchi;
        niter_out[b] = niter;
        status_out[b] = status;
    }
}

}  // namespace scint

extern "C" int32_t scint_acf1d_fit_workspace_bytes(int64_t B, int64_t R, int64_t C, size_t* bytes) {
    SCINT_REQUIRE(bytes != nullptr, "acf1d_fit_workspace_bytes: null output");
    SCINT_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && R >= 6 && C >= 6 && R < ((int64_t)1 << 30) && C < ((int64_t)1 << 30),
                  "acf1d_fit_workspace_bytes: bad shape");
    *bytes = sizeof(double) * 2 * (size_t)B * (size_t)((R - R / 2) + (C - C / 2)) + 256;
    return SCINT_OK;
}

extern "C" int32_t scint_acf1d_fit(const double* acf, int64_t B, int64_t R, int64_t C, double dt, double df, const double* bw,
                                   const double* tobs, double nscale, int32_t full_frame, int32_t weighted, int32_t bartlett,
                                   double alpha, int32_t alpha_varies, int32_t max_iter, double* values_out, double* errors_out,
                                   double* stats_out, int32_t* niter_out, int32_t* status_out, double* setup_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    using namespace scint;
    SCINT_REQUIRE(acf && bw && tobs && values_out && errors_out && stats_out && niter_out && status_out && workspace,
                  "acf1d_fit: null pointer");
    size_t need = 0;
    SCINT_REQUIRE(scint_acf1d_fit_workspace_bytes(B, R, C, &need) == SCINT_OK, "acf1d_fit: bad shape");
    SCINT_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(df) && df > 0.0, "acf1d_fit: dt and df must be positive");
    SCINT_REQUIRE(isfinite(nscale) && nscale > 0.0 && isfinite(alpha), "acf1d_fit: bad nscale or alpha");
    SCINT_REQUIRE(max_iter >= 1 && max_iter <= 100000, "acf1d_fit: max_iter must lie in [1, 100000]");
    if (workspace_bytes < need) { set_error("scint: acf1d_fit workspace too small"); return SCINT_E_WORKSPACE; }
    const dim3 grid((unsigned)ceil_div(B, kFitWaves)), block(64 * kFitWaves);
    if (alpha_varies)
        hipLaunchKernelGGL(acf1d_fit_kernel<4>, grid, block, 0, (hipStream_t)stream, acf, B, R, C, dt, df, bw, tobs, nscale,
                           (int)full_frame, (int)weighted, (int)bartlett, alpha, (int)max_iter, values_out, errors_out, stats_out,
                           niter_out, status_out, setup_out, (double*)workspace);
    else
        hipLaunchKernelGGL(acf1d_fit_kernel<3>, grid, block, 0, (hipStream_t)stream, acf, B, R, C, dt, df, bw, tobs, nscale,
                           (int)full_frame, (int)weighted, (int)bartlett, alpha, (int)max_iter, values_out, errors_out, stats_out,
                           niter_out, status_out, setup_out, (double*)workspace);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}
