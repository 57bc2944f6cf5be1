// acf2d.hpp -- the batched approximate 2-D ACF fit of tau, dnu and the phase gradient (the reference's
// get_scint_params(method='acf2d_approx'): dynspec.py:2710-2842, scint_models.py:123-161).  Included at the end of fft.hip, after
// scintpar.hpp, whose Cholesky helpers and status codes it reuses.
//
//   acf_argmax_kernel      per ACF of a stack the FIRST flat index of its maximum (np.argmax): the host centres the window on it;
//   acf2d_fit_kernel       one 256-thread WORKGROUP per problem, the whole Levenberg-Marquardt loop in one launch.  The window is a
//                          rectangle of the ACF chosen by the host; thread tid walks its points k = tid, tid + 256, ... in
//                          ascending order and reads acf directly (a window of <= 1e4 doubles stays in L2).  Weights are computed
//                          in place from the ticks and the sample, never stored.  A thread keeps the lower triangle of J^T J,
//                          J^T r and chi^2 in registers (15 + 5 + 1 doubles at most); they are reduced by the wave butterfly, then
//                          the four waves in index order through LDS -- every thread then holds the same bits, so the solve and
//                          every decision (and every barrier) is workgroup-uniform.  No atomics: equal inputs give equal bits;
//   acf2d_model_kernel     the residual (y - model) w of scint_acf_model_2d_approx for given parameters, one thread per point.
#pragma once
#include <math.h>

#include "common.hpp"
#include "scintpar.hpp"

namespace scint {

constexpr int kFitBadWindow = 5;       // status_out, after scintpar.hpp's kFit*: the host's rectangle is not centred / not odd
constexpr int kFit2dPar = 5;           // tau, dnu, amp, alpha, phasegrad
constexpr double kLn2 = 0.6931471805599453;

// idx_out[b] = np.argmax(acf[b]): the larger value wins, equal values resolve to the LOWER flat index, NaN never compares larger.
__global__ void __launch_bounds__(256) acf_argmax_kernel(const double* acf, int64_t n, int32_t* idx_out) {
    __shared__ double red_v[4];
    __shared__ int red_c[4];
    const double* a = acf + (int64_t)blockIdx.x * n;
    double v = -INFINITY;
    int c = 0x7fffffff;
    for (int64_t k = threadIdx.x; k < n; k += 256) {    // ascending: a strict > keeps the thread's first occurrence
        const double x = a[k];
        if (x > v) { v = x; c = (int)k; }
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
    if (threadIdx.x == 0) idx_out[blockIdx.x] = c == 0x7fffffff ? 0 : c;
}

// One problem's window: rows f0 .. f0 + nfw, columns t0 .. t0 + ntw of a[R][C]; its ticks are those of
// np.linspace(-tobs, tobs, C + 1)[:-1] and np.linspace(-bw, bw, R + 1)[:-1] (index * step + start, as NumPy rounds it).
struct Acf2dWin {
    const double* a;
    int64_t C;
    int f0, nfw, t0, ntw;
    double tobs, bw, tstep, fstep, tmaxv, fmaxv, nsn;
    int weighted;
};

__device__ inline double acf2d_t(const Acf2dWin& w, int j) {
#pragma clang fp contract(off)
    return (double)(w.t0 + j) * w.tstep + -w.tobs;
}
__device__ inline double acf2d_f(const Acf2dWin& w, int i) {
#pragma clang fp contract(off)
    return (double)(w.f0 + i) * w.fstep + -w.bw;
}
__device__ inline double acf2d_y(const Acf2dWin& w, int i, int j) { return w.a[(int64_t)(w.f0 + i) * w.C + w.t0 + j]; }

// W0 of window point (i, j) (dynspec.py:2716-2727, :2785): sqrt(nsub nchan (T / max tticks) (F / max fticks)) written as the
// reference writes it, 1 / (1 / sqrt(.)) with a non-finite error set to infinity (weight 0); 1 when not weighted; zero where
// y - 1 / W0 < 0.
__device__ inline double acf2d_w0(const Acf2dWin& w, int i, int j) {
#pragma clang fp contract(off)
    double wt = 1.0;
    if (w.weighted) {
        const double T = w.tobs - fabs(acf2d_t(w, j)), F = w.bw - fabs(acf2d_f(w, i));
        const double n2d = w.nsn * (T / w.tmaxv) * (F / w.fmaxv);
        double e = 1.0 / sqrt(n2d);
        if (!isfinite(e)) e = INFINITY;
        wt = 1.0 / e;
    }
    if (acf2d_y(w, i, j) - 1.0 / wt < 0.0) wt = 0.0;
    return wt;
}
// The weight the fit sees at (i, j): the reference's double fftshift (dynspec.py:2787-2789) rolls an odd window by -1 in both
// axes, and the model zeroes the centre (scint_models.py:156-158).
__device__ inline double acf2d_weight(const Acf2dWin& w, int i, int j) {
    if (i == w.nfw / 2 && j == w.ntw / 2) return 0.0;
    const int si = i + 1 == w.nfw ? 0 : i + 1, sj = j + 1 == w.ntw ? 0 : j + 1;
    return acf2d_w0(w, si, sj);
}

// model = amp exp(-(|(t - 60 phasegrad f) / tau|^(3 alpha / 2) + |f ln2 / dnu|^(3/2))^(2/3)) (1 - |t| / tobs) (1 - |f| / bw) and what its
// derivatives share: with S the inner sum and G = S^(2/3), d model = -K dS where K = model (2/3) G / S.  An exponent past 700 has
// underflowed: model and K are 0 there, so an overflowing S gives no inf * 0.
struct Acf2dTerms { double m, K, A, Bv, u, au; };
__device__ inline Acf2dTerms acf2d_terms(double t, double f, double tau, double dnu, double amp, double alpha, double pg,
                                         double tobs, double bw) {
    Acf2dTerms o;
    o.u = (t - 60.0 * pg * f) / tau;
    o.au = fabs(o.u);
    o.A = pow(o.au, 1.5 * alpha);
    const double v = fabs(f) * kLn2 / dnu;
    o.Bv = v * sqrt(v);
    const double S = o.A + o.Bv, G = cbrt(S * S);
    const bool live = G < 700.0;
    const double tri = (1.0 - fabs(t) / tobs) * (1.0 - fabs(f) / bw);
    o.m = live ? amp * exp(-G) * tri : 0.0;
    o.K = live && S > 0.0 ? o.m * (2.0 / 3.0) * G / S : 0.0;
    if (!live) o.A = o.Bv = 0.0;
    return o;
}

// which of p = (tau, dnu, amp, alpha, phasegrad) the i-th varying parameter is: [tau,] dnu, amp, phasegrad[, alpha]
__device__ constexpr int acf2d_pid(bool tau_varies, int i) {
    const int k = i + (tau_varies ? 0 : 1);
    return k < 3 ? k : (k == 3 ? 4 : 3);
}

// N sums of the workgroup: the wave butterfly, then the four waves in index order through red[4 * N].  Every thread gets the total.
template <int N>
__device__ inline void acf2d_block_sum(double (&v)[N], double* red) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                    // the readers of the previous reduction are done with red
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[wv * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
}

// One pass over the window at p: chi^2 = sum r^2, J^T r and J^T J (lower triangle) of r = (y - model) w in the varying ones of
// (log tau, log dnu, log amp, phasegrad, alpha).  A point of weight zero adds nothing and is skipped (the centre is one).
// A ln|u| and A / u are 0 at u = 0 (the exponent 3 alpha / 2 exceeds 1).
template <bool TAU, bool ALPHA>
__device__ inline void acf2d_pass(const Acf2dWin& w, const double* p, FitSums<3 + TAU + ALPHA>& s, double* red) {
    constexpr int NV = 3 + TAU + ALPHA, NS = 1 + NV + NV * (NV + 1) / 2;
    const double tau = p[0], dnu = p[1], amp = p[2], alpha = p[3], pg = p[4];
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    const int npts = w.nfw * w.ntw;
    for (int k = threadIdx.x; k < npts; k += 256) {
        const int i = k / w.ntw, j = k - i * w.ntw;
        const double wt = acf2d_weight(w, i, j);
        if (wt == 0.0) continue;
        const double t = acf2d_t(w, j), f = acf2d_f(w, i);
        const Acf2dTerms o = acf2d_terms(t, f, tau, dnu, amp, alpha, pg, w.tobs, w.bw);
        const double r = (acf2d_y(w, i, j) - o.m) * wt;
        const double ex = 1.5 * alpha, wk = wt * o.K;
        double J5[kFit2dPar];
        J5[0] = -wk * ex * o.A;
        J5[1] = -wk * 1.5 * o.Bv;
        J5[2] = -wt * o.m;
        J5[3] = o.au > 0.0 ? wk * 1.5 * o.A * log(o.au) : 0.0;
        J5[4] = o.au > 0.0 ? -wk * ex * (o.A / o.u) * 60.0 * f / tau : 0.0;
        double J[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) J[a] = J5[acf2d_pid(TAU, a)];
        acc[0] += r * r;
        int n = 1 + NV;
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            acc[1 + a] += J[a] * r;
#pragma unroll
            for (int b = 0; b <= a; ++b) acc[n++] += J[a] * J[b];
        }
    }
    acf2d_block_sum<NS>(acc, red);
    s.cost = acc[0];
    int n = 1 + NV;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        s.g[a] = acc[1 + a];
#pragma unroll
        for (int b = 0; b <= a; ++b) s.a[a][b] = acc[n++];
    }
}

// rect[b] = (f0, nfw, t0, ntw); start[b] = (tau, dnu, amp, alpha, phasegrad); status_in[b] != 0: the host has already given up on
// problem b (its status is passed on, its outputs are NaN).  setup: NULL, or per problem 2 R C doubles -- the window's y, row-major
// in the first nfw ntw of the first R C, its weights likewise in the second R C.
template <bool TAU, bool ALPHA>
__global__ void __launch_bounds__(256)
acf2d_fit_kernel(const double* acf, int64_t R, int64_t C, const int32_t* rect, const double* start, const int32_t* status_in,
                 const double* bw, const double* tobs, double nsn, int weighted, int max_iter, double* values, double* errors,
                 double* stats, int32_t* niter_out, int32_t* status_out, int32_t* nnz_out, double* setup) {
#pragma clang fp contract(off)
    constexpr int NV = 3 + TAU + ALPHA;
    __shared__ double red[4 * (1 + kFit2dPar + kFit2dPar * (kFit2dPar + 1) / 2)];
    const int64_t b = blockIdx.x;
    const double nan = __builtin_nan("");
    Acf2dWin w;
    w.a = acf + b * R * C;
    w.C = C;
    w.f0 = rect[b * 4]; w.nfw = rect[b * 4 + 1]; w.t0 = rect[b * 4 + 2]; w.ntw = rect[b * 4 + 3];
    w.tobs = tobs[b]; w.bw = bw[b];
    w.tstep = (w.tobs - -w.tobs) / (double)C;
    w.fstep = (w.bw - -w.bw) / (double)R;
    w.tmaxv = (double)(C - 1) * w.tstep + -w.tobs;      // max(tticks), max(fticks): the last ticks
    w.fmaxv = (double)(R - 1) * w.fstep + -w.bw;
    w.nsn = nsn;
    w.weighted = weighted;

    // everything below is uniform over the workgroup: the same rectangle, the same start, and after each reduction the same sums
    int status = status_in[b], niter = 0, nnz = 0;
    double p[kFit2dPar];
#pragma unroll
    for (int i = 0; i < kFit2dPar; ++i) p[i] = start[b * kFit2dPar + i];
    double val[kFit2dPar], err[kFit2dPar], chisqr = nan, redchi = nan;
#pragma unroll
    for (int i = 0; i < kFit2dPar; ++i) val[i] = err[i] = nan;

    const bool inside = w.nfw >= 1 && w.ntw >= 1 && w.f0 >= 0 && w.t0 >= 0 && (int64_t)w.f0 + w.nfw <= R && (int64_t)w.t0 + w.ntw <= C;
    if (status == kFitConverged && !(inside && (w.nfw & 1) && (w.ntw & 1))) status = kFitBadWindow;
    const bool go = status == kFitConverged;
    if (go) {
        const int npts = w.nfw * w.ntw;
        double cnt[1] = {0.0};
        double* ys = setup ? setup + b * 2 * R * C : nullptr;
        for (int k = threadIdx.x; k < npts; k += 256) {
            const int i = k / w.ntw, j = k - i * w.ntw;
            const double wt = acf2d_weight(w, i, j);
            cnt[0] += wt != 0.0 ? 1.0 : 0.0;
            if (ys) { ys[k] = acf2d_y(w, i, j); ys[R * C + k] = wt; }
        }
        acf2d_block_sum<1>(cnt, red);
        nnz = (int)cnt[0];

        FitSums<NV> cur, tri;
        double d[NV], c[NV][NV];
        status = kFitIterCap;
        bool ok = p[0] > 0.0 && p[1] > 0.0 && p[2] > 0.0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]) &&
                  isfinite(p[4]) && npts > NV;
        if (!ok) {
            status = kFitSingular;      // a scale at zero has no logarithm
        } else {
            acf2d_pass<TAU, ALPHA>(w, p, cur, red);
            if (!isfinite(cur.cost)) { status = kFitNonFiniteStep; ok = false; }
        }
        // Levenberg-Marquardt as the 1-D fit's (scintpar.hpp): Marquardt's scaling, the step limit of 3, Nielsen's gain-ratio
        // damping, the flat-cost rule, convergence when a pass moves no parameter by more than 1e-12
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
                dq[i] = dq[i] > 3.0 ? 3.0 : (dq[i] < -3.0 ? -3.0 : dq[i]);
                step = fabs(dq[i]) > step ? fabs(dq[i]) : step;
            }
            if (!fin) { status = kFitNonFiniteStep; ok = false; break; }
            double q[kFit2dPar];
#pragma unroll
            for (int i = 0; i < kFit2dPar; ++i) q[i] = p[i];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int id = acf2d_pid(TAU, i);
                q[id] = id < 3 ? p[id] * exp(dq[i]) : p[id] + dq[i];
            }
            acf2d_pass<TAU, ALPHA>(w, q, tri, red);
            if (!isfinite(tri.cost)) { status = kFitNonFiniteStep; ok = false; break; }
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
                for (int i = 0; i < kFit2dPar; ++i) p[i] = q[i];
                cur = tri;
            }
            if (step <= 1e-12) { status = kFitConverged; break; }
        }
        // covariance in the external parameters at the optimum: (J^T J)^-1 chi^2 / (N - nvary), N = every point of the window
        if (ok && status == kFitConverged) {
            if (!acf1d_factor<NV>(cur, 0.0, d, c)) {
                status = kFitSingular;
            } else {
                chisqr = cur.cost;
                redchi = chisqr / (double)(npts - NV);
#pragma unroll
                for (int i = 0; i < kFit2dPar; ++i) { val[i] = p[i]; err[i] = 0.0; }       // a fixed parameter has no error
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    double unit[NV];
#pragma unroll
                    for (int k = 0; k < NV; ++k) unit[k] = k == i ? 1.0 : 0.0;
                    acf1d_chol_solve<NV>(c, unit);
                    const int id = acf2d_pid(TAU, i);
                    err[id] = sqrt(unit[i] * redchi) * (id < 3 ? p[id] : 1.0) / d[i];      // d p / d log p = p
                }
            }
        }
        if (status != kFitConverged) {
#pragma unroll
            for (int i = 0; i < kFit2dPar; ++i) val[i] = err[i] = nan;
            chisqr = redchi = nan;
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kFit2dPar; ++i) { values[b * kFit2dPar + i] = val[i]; errors[b * kFit2dPar + i] = err[i]; }
        stats[b * 2] = chisqr;
        stats[b * 2 + 1] = redchi;
        niter_out[b] = niter;
        status_out[b] = status;
        nnz_out[b] = nnz;
    }
}

// out[i][j] = (y[i][j] - model(t_j, f_i)) w[i][j]; y NULL: 0, w NULL: 1; the weight at ((nf - 1) / 2, (nt - 1) / 2) is zero
// (fftshift, [-1, -1] = 0, ifftshift: scint_models.py:156-158)
__global__ void __launch_bounds__(256)
acf2d_model_kernel(const double* tdata, int64_t nt, const double* fdata, int64_t nf, const double* y, const double* wgt, double tau,
                   double dnu, double amp, double alpha, double pg, double tobs, double bw, double* out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nf * nt) return;
    const int64_t i = k / nt, j = k - i * nt;
    const Acf2dTerms o = acf2d_terms(tdata[j], fdata[i], tau, dnu, amp, alpha, pg, tobs, bw);
    double wt = wgt ? wgt[k] : 1.0;
    if (i == (nf - 1) / 2 && j == (nt - 1) / 2) wt = 0.0;
    out[k] = ((y ? y[k] : 0.0) - o.m) * wt;
}

}  // namespace scint

extern "C" int32_t scint_acf_argmax(const double* acf, int64_t B, int64_t R, int64_t C, int32_t* idx_out, void* stream) {
    SCINT_REQUIRE(acf && idx_out, "acf_argmax: null pointer");
    SCINT_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && R >= 1 && C >= 1 && R < ((int64_t)1 << 30) && C < ((int64_t)1 << 30) &&
                  R * C < ((int64_t)1 << 31), "acf_argmax: bad shape");
    hipLaunchKernelGGL(scint::acf_argmax_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, acf, R * C, idx_out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_acf2d_approx_fit_workspace_bytes(int64_t B, int64_t R, int64_t C, int32_t return_setup, size_t* bytes) {
    SCINT_REQUIRE(bytes != nullptr, "acf2d_approx_fit_workspace_bytes: null output");
    SCINT_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && R >= 6 && C >= 6 && R < ((int64_t)1 << 30) && C < ((int64_t)1 << 30) &&
                  R * C < ((int64_t)1 << 31), "acf2d_approx_fit_workspace_bytes: bad shape");
    *bytes = (return_setup ? sizeof(double) * 2 * (size_t)B * (size_t)(R * C) : 0) + 256;
    return SCINT_OK;
}

extern "C" int32_t scint_acf2d_approx_fit(const double* acf, int64_t B, int64_t R, int64_t C, const int32_t* rect, const double* start,
                                          const int32_t* status_in, const double* bw, const double* tobs, double nsub, double nchan,
                                          int32_t weighted, int32_t tau_varies, int32_t alpha_varies, int32_t max_iter,
                                          double* values_out, double* errors_out, double* stats_out, int32_t* niter_out,
                                          int32_t* status_out, int32_t* nnz_out, int32_t return_setup, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
    using namespace scint;
    SCINT_REQUIRE(acf && rect && start && status_in && bw && tobs && values_out && errors_out && stats_out && niter_out &&
                  status_out && nnz_out && workspace, "acf2d_approx_fit: null pointer");
    size_t need = 0;
    SCINT_REQUIRE(scint_acf2d_approx_fit_workspace_bytes(B, R, C, return_setup, &need) == SCINT_OK, "acf2d_approx_fit: bad shape");
    SCINT_REQUIRE(isfinite(nsub) && nsub > 0.0 && isfinite(nchan) && nchan > 0.0, "acf2d_approx_fit: nsub and nchan must be positive");
    SCINT_REQUIRE(max_iter >= 1 && max_iter <= 100000, "acf2d_approx_fit: max_iter must lie in [1, 100000]");
    if (workspace_bytes < need) { set_error("scint: acf2d_approx_fit workspace too small"); return SCINT_E_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    double* setup = return_setup ? (double*)workspace : nullptr;
    const double nsn = nsub * nchan;
    const dim3 grid((unsigned)B), block(256);
#define SCINT_ACF2D_LAUNCH(TAU, ALPHA)                                                                                          \
    hipLaunchKernelGGL((acf2d_fit_kernel<TAU, ALPHA>), grid, block, 0, stream, acf, R, C, rect, start, status_in, bw, tobs, nsn, \
                       (int)weighted, (int)max_iter, values_out, errors_out, stats_out, niter_out, status_out, nnz_out, setup)
    if (tau_varies && alpha_varies) SCINT_ACF2D_LAUNCH(true, true);
    else if (tau_varies) SCINT_ACF2D_LAUNCH(true, false);
    else if (alpha_varies) SCINT_ACF2D_LAUNCH(false, true);
    else SCINT_ACF2D_LAUNCH(false, false);
#undef SCINT_ACF2D_LAUNCH
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}

extern "C" int32_t scint_acf2d_approx_model(const double* tdata, int64_t nt, const double* fdata, int64_t nf, const double* ydata,
                                            const double* weights, double tau, double dnu, double amp, double alpha,
                                            double phasegrad, double tobs, double bw, double* out, void* stream) {
    SCINT_REQUIRE(tdata && fdata && out, "acf2d_approx_model: null pointer");
    SCINT_REQUIRE(nt >= 1 && nf >= 1 && nt < ((int64_t)1 << 30) && nf < ((int64_t)1 << 30) && nt * nf < ((int64_t)1 << 38),
                  "acf2d_approx_model: bad shape");
    SCINT_REQUIRE(isfinite(tau) && isfinite(dnu) && isfinite(amp) && isfinite(alpha) && isfinite(phasegrad) && isfinite(tobs) &&
                  isfinite(bw), "acf2d_approx_model: non-finite parameter");
    hipLaunchKernelGGL(scint::acf2d_model_kernel, dim3((unsigned)scint::ceil_div(nt * nf, 256)), dim3(256), 0, (hipStream_t)stream,
                       tdata, nt, fdata, nf, ydata, weights, tau, dnu, amp, alpha, phasegrad, tobs, bw, out);
    SCINT_LAUNCH_CHECK();
    return SCINT_OK;
}
