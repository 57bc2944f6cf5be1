// bright.hpp -- the brightness-distribution model of a secondary spectrum (scint_sim.py:768-958, Brightness; Yao et al. 2020).
// The entry points are in fft.hip (the two transforms of the model are its generic 2-D driver).  Every function that restates a
// NumPy expression switches floating-point contraction off: a fused multiply-add rounds differently from NumPy's two operations.
//
//   efield   Rho = exp(-0.5 (a X^2 + b Y^2 + c X Y)^(alpha/2)) on the [n][n] grid (calc_brightness, :855-857); a, b, c from the host
//   map      one thread per (itd, ifd) pixel, ifd along the lanes: the reference's three-branch loop body (:911-925) and the two
//            interpolations of B at (thetax, +thetay) and (thetax, -thetay) (:933-938).  scipy's griddata(method='linear') on a
//            regular grid is the piecewise-linear interpolant on a triangulation that splits every cell along ONE diagonal; which
//            one is a bit per cell, read from a packed bitmap (bit iy (n-1) + ix of a little-endian byte stream; 1 = the diagonal
//            from corner (ix, iy) to (ix+1, iy+1)) or taken as 1 everywhere when the pointer is null.  B (n^2 doubles: 2.9 MB at the
//            defaults) stays in the cache; the kernel's cost is its arithmetic and its writes.
//   fold     SS[1:, 1:] += flip(flip(SS0[1:, 1:])) and LSS = 10 log10(SS) (:947-950), out of place
//   max      np.max (NaN if any element is NaN) in two fixed-order stages, then the division (calc_acf, :956)
// No atomics: equal inputs give equal bits.
#pragma once
#include <math.h>

#include "common.hpp"

namespace scint {

struct BrightMapPar {
    const double* B; const double* x; int n;     // brightness [n][n] on the grid x[n] (ascending)
    const uint8_t* diag;                          // packed [n-1][n-1] bitmap or null (main diagonal everywhere)
    const double* fd; int nfd;                    // Doppler axis (lanes)
    const double* td; int ntd;                    // delay axis
    double thetagx, thetagy, thetarx, rx2, ry2;   // rx2 = thetarx**2, ry2 = thetary**2 as the host evaluates them
    double half_df, two_over_df, floor_amp;       // 0.5 * df, 2 / df, 10**(-6)
    double inv_step;                              // (n - 1) / (x[n-1] - x[0]): the first guess of a query's cell
    double* ss0; double* jac;                     // [ntd][nfd]
    double* thetax; double* thetay;               // [ntd][nfd] or null
};

__global__ void __launch_bounds__(256) bright_efield_kernel(const double* __restrict__ x, int n, double a, double b, double c,
                                                            double alpha2, double* __restrict__ rho) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int iy = (int)(idx / n), ix = (int)(idx - (int64_t)iy * n);
    const double X = x[ix], Y = x[iy];
    const double q = (a * (X * X) + b * (Y * Y)) + (c * X) * Y;
    rho[idx] = exp(-0.5 * pow(q, alpha2));
}

// The cell index i in [0, n-2] with x[i] <= q <= x[i+1] for x[0] <= q <= x[n-1]: a guess from the mean step, corrected against
// the grid's own values (np.arange accumulates no error, but start + i step rounds: the guess can be one off).
__device__ inline int bright_cell(const double* __restrict__ x, int n, double q, double inv_step) {
    int i = (int)floor((q - x[0]) * inv_step);
    i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
    while (i > 0 && q < x[i]) --i;
    while (i < n - 2 && q >= x[i + 1]) ++i;
    return i;
}

// B at (qx, qy): barycentric weights on the triangle of the cell that holds the point; NaN outside the grid (griddata's fill).
__device__ inline double bright_interp(const BrightMapPar& p, double qx, double qy) {
#pragma clang fp contract(off)
    const double* __restrict__ x = p.x;
    const int n = p.n;
    if (!(qx >= x[0] && qx <= x[n - 1] && qy >= x[0] && qy <= x[n - 1])) return NAN;
    const int ix = bright_cell(x, n, qx, p.inv_step), iy = bright_cell(x, n, qy, p.inv_step);
    const double u = (qx - x[ix]) / (x[ix + 1] - x[ix]);
    const double v = (qy - x[iy]) / (x[iy + 1] - x[iy]);
    const double* __restrict__ r0 = p.B + (int64_t)iy * n + ix;
    const double b00 = r0[0], b10 = r0[1], b01 = r0[n], b11 = r0[n + 1];
    bool main_diag = true;
    if (p.diag) {
        const int64_t bit = (int64_t)iy * (n - 1) + ix;
        main_diag = (p.diag[bit >> 3] >> (bit & 7)) & 1;
    }
    if (main_diag) {
        if (u >= v) return ((1.0 - u) * b00 + (u - v) * b10) + v * b11;
        return ((1.0 - v) * b00 + (v - u) * b01) + u * b11;
    }
    if (u + v <= 1.0) return (((1.0 - u) - v) * b00 + u * b10) + v * b01;
    return ((1.0 - v) * b10 + (1.0 - u) * b01) + ((u + v) - 1.0) * b11;
}

__global__ void __launch_bounds__(256) bright_map_kernel(BrightMapPar p) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)p.ntd * p.nfd) return;
    const int itd = (int)(idx / p.nfd), ifd = (int)(idx - (int64_t)itd * p.nfd);
    const double thx = (p.fd[ifd] - p.thetagx) + p.thetarx;
    const double t = thx + p.thetagx;
    const double sq = ((p.td[itd] - t * t) + p.rx2) + p.ry2;
    double thy = 0.0, amp;
    if (sq > 0.0) {
        const double thym = sqrt(sq);
        thy = 0.0 + (thym - p.thetagy);
        amp = thym < p.half_df ? p.two_over_df : 1.0 / thym;
    } else {
        amp = p.floor_amp;                       // on or outside the primary arc: thetay = 0 exactly, still interpolated
    }
    const double up = bright_interp(p, thx, thy), dn = bright_interp(p, thx, -thy);
    p.ss0[idx] = up * amp + dn * amp;
    p.jac[idx] = amp;
    if (p.thetax) p.thetax[idx] = thx;
    if (p.thetay) p.thetay[idx] = thy;
}

__global__ void __launch_bounds__(256) bright_fold_kernel(const double* __restrict__ ss0, int ntd, int nfd, double* __restrict__ ss,
                                                          double* __restrict__ lss) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)ntd * nfd) return;
    const int i = (int)(idx / nfd), j = (int)(idx - (int64_t)i * nfd);
    double v = ss0[idx];
    if (i >= 1 && j >= 1) v = v + ss0[(int64_t)(ntd - i) * nfd + (nfd - j)];
    ss[idx] = v;
    lss[idx] = 10.0 * log10(v);
}

__device__ inline double nanmax(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

__global__ void __launch_bounds__(256) bright_max_partial_kernel(const double* __restrict__ x, int64_t n, double* partial) {
    __shared__ double red[4];
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = nanmax(m, x[i]);
    for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
}
// partial[np] <- the maximum of partial[0 .. np): one workgroup, before the division reads it
__global__ void __launch_bounds__(64) bright_max_final_kernel(double* partial, int np) {
    double m = -INFINITY;
    for (int i = threadIdx.x; i < np; i += 64) m = nanmax(m, partial[i]);
    for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) partial[np] = m;
}
__global__ void __launch_bounds__(256) bright_divide_kernel(double* __restrict__ x, int64_t n, const double* __restrict__ m) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) x[idx] = x[idx] / m[0];
}

}  // namespace scint
